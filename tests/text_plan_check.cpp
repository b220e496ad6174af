// text_plan_check.cpp -- prints the text front end's plans (text_plan.hpp) as
// JSON lines for the cases on stdin, one case per line of name=value tokens:
// the record bound, grids and footprint of a chunk (bytes, lines, seps,
// approx, items, out_bytes, mis, num_cus), the chunk size (requested, free),
// the run bounds of the partition rule (k, parts), the cut of a buffer
// (buf=<hex bytes>, eof) and the verdict on one line (line=<hex bytes>, sep):
// the line's separators are found here by walking it, the verdict is
// text_verdict's.  Built and run by tests/test_text_plan_cpu.py; no GPU, no HIP.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../bsdb_amd/csrc/text_plan.hpp"

using namespace bsdb;

static void J(const char *k, unsigned long long v, const char *end = ",") { printf("\"%s\":%llu%s", k, v, end); }

static std::vector<uint8_t> unhex(const std::string &h) {
    std::vector<uint8_t> out;
    for (size_t i = 0; i + 1 < h.size(); i += 2) out.push_back((uint8_t)strtoul(h.substr(i, 2).c_str(), nullptr, 16));
    return out;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream ss(line);
        std::string tok;
        uint64_t bytes = 0, lines = 0, seps = 0, approx = 0, items = 0, out_bytes = 0, mis = 0, num_cus = 256, requested = 0,
                 free_b = 0, k = 0, parts = 1, eof = 0, sep = ' ';
        std::vector<uint8_t> buf, text;
        while (ss >> tok) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) return 2;
            const std::string key = tok.substr(0, eq);
            const uint64_t v = strtoull(tok.c_str() + eq + 1, nullptr, 10);
            if (key == "bytes") bytes = v;
            else if (key == "lines") lines = v;
            else if (key == "seps") seps = v;
            else if (key == "approx") approx = v;
            else if (key == "items") items = v;
            else if (key == "out_bytes") out_bytes = v;
            else if (key == "mis") mis = v;
            else if (key == "num_cus") num_cus = v;
            else if (key == "requested") requested = v;
            else if (key == "free") free_b = v;
            else if (key == "k") k = v;
            else if (key == "parts") parts = v;
            else if (key == "eof") eof = v;
            else if (key == "sep") sep = v;
            else if (key == "buf") buf = unhex(tok.substr(eq + 1));
            else if (key == "line") text = unhex(tok.substr(eq + 1));
            else return 2;
        }
        if (parts < 1 || parts > (uint64_t)TEXT_MAX_PARTS) return 2;
        const TextFootprint f = text_footprint(bytes, lines, seps, approx != 0);
        printf("{");
        J("max_records", text_max_records(bytes)), J("blocks", text_blocks(bytes)), J("count_grid", text_count_grid(bytes));
        J("lane_grid", text_lane_grid(items, (int)num_cus)), J("pieces", piece_count(out_bytes, (uint32_t)mis));
        J("pack_grid", piece_grid(out_bytes, (uint32_t)mis, (int)num_cus));
        J("image_max", text_image_max(bytes)), J("blob_max", text_blob_max(bytes));
        J("fp_split", f.split), J("fp_pack", f.pack), J("fp_total", f.total);
        J("chunk", text_chunk_bytes(requested, free_b)), J("bad_sep", text_bad_separator((int)(int64_t)sep));
        printf("\"bound\":[");
        for (uint64_t p = 0; p <= parts; ++p)
            printf("%s%llu", p ? "," : "", (unsigned long long)text_run_bound(k, (uint32_t)parts, (uint32_t)p));
        printf("],");
        J("cut", text_cut(buf.data(), buf.size(), eof != 0));
        uint32_t c = 0, s1 = 0, s2 = 0;
        for (uint32_t i = 0; i < text.size(); ++i)
            if (text[i] == (uint8_t)sep) {
                if (c == 0) s1 = i;
                if (c == 1) s2 = i;
                ++c;
            }
        const TextLine t = text_verdict(0, (uint32_t)text.size(), c, s1, s2);
        J("verdict", t.verdict), J("kpos", t.kpos), J("klen", t.klen), J("vpos", t.vpos), J("vlen", t.vlen, "}\n");
    }
    return 0;
}
