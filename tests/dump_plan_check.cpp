// dump_plan_check.cpp -- prints the plans of the enumeration of a resident
// database (dump_plan.hpp) as JSON lines for the cases on stdin, one case per
// line of name=value tokens: the line length and the length status of one
// record (status, klen, vlen), the grids (count, text_bytes, mis, num_cus), the
// text-chunk cap (chunk) and dump_cut over the scan of the line lengths given
// as llen=a,b,c shifted by loff0, against `cap`.  The scan sits in a heap
// allocation of exactly count + 1 words, so a read past it is a report.  Built
// and run by tests/test_dump_plan_cpu.py; no GPU, no HIP.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../bsdb_amd/csrc/dump_plan.hpp"

using namespace bsdb;

static void J(const char *k, unsigned long long v, const char *end = ",") { printf("\"%s\":%llu%s", k, v, end); }

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream ss(line);
        std::string tok;
        uint64_t status = 0, klen = 0, vlen = 0, count = 0, text_bytes = 0, mis = 0, num_cus = 256, chunk = 0, cap = 0, loff0 = 0;
        std::vector<uint64_t> llen;
        while (ss >> tok) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) return 2;
            const std::string k = tok.substr(0, eq);
            const char *val = tok.c_str() + eq + 1;
            const uint64_t v = strtoull(val, nullptr, 10);
            if (k == "status") status = v;
            else if (k == "klen") klen = v;
            else if (k == "vlen") vlen = v;
            else if (k == "count") count = v;
            else if (k == "text_bytes") text_bytes = v;
            else if (k == "mis") mis = v;
            else if (k == "num_cus") num_cus = v;
            else if (k == "chunk") chunk = v;
            else if (k == "cap") cap = v;
            else if (k == "loff0") loff0 = v;
            else if (k == "llen") {
                for (const char *s = val; *s;) {
                    char *end;
                    llen.push_back(strtoull(s, &end, 10));
                    if (*end != ',') break;
                    s = end + 1;
                }
            } else return 2;
        }
        uint64_t *loff = (uint64_t *)malloc(8 * (llen.size() + 1));  // exactly the scan
        if (!loff) return 3;
        loff[0] = loff0;
        for (size_t i = 0; i < llen.size(); ++i) loff[i + 1] = loff[i] + llen[i];
        printf("{");
        J("line_len", dump_line_len((int)status, (uint32_t)klen, (uint32_t)vlen));
        J("length_status", (unsigned)dump_length_status((int)status, (uint32_t)klen, (uint32_t)vlen));
        J("status_in", (unsigned)dump_status_in((uint8_t)status));
        J("lane_grid", dump_lane_grid(count, (int)num_cus)), J("text_grid", dump_text_grid(text_bytes, (uint32_t)mis, (int)num_cus));
        J("bad_chunk", dump_bad_chunk(chunk)), J("chunk_bytes", dump_chunk_bytes(chunk)), J("max_line", DUMP_MAX_LINE);
        J("cut", dump_cut(loff, llen.size(), cap), "}\n");
        free(loff);
    }
    return 0;
}
