// get_plan_check.cpp -- prints the batched reader's plans (get_plan.hpp) as
// JSON lines for the cases on stdin, one case per line of name=value tokens:
// the image layout of `parts` partition files (size0.. sizeK), the open
// footprint (n, approx, free), the host chunk (batch, key_len), the locate and
// gather grids (nq, value_bytes, mis, num_cus) and the decode of one address
// (addr, format, against the same sizes).  Built and run by
// tests/test_get_plan_cpu.py; no GPU, no HIP.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "../bsdb_amd/csrc/get_plan.hpp"

using namespace bsdb;

static void J(const char *k, unsigned long long v, const char *end = ",") { printf("\"%s\":%llu%s", k, v, end); }

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream ss(line);
        std::string tok;
        uint64_t parts = 1, n = 0, approx = 0, free_b = 0, batch = 0, key_len = 0, nq = 0, value_bytes = 0, mis = 0,
                 num_cus = 256, addr = 0, format = 0, dparts = UINT64_MAX;
        uint64_t sizes[GET_MAX_PARTS + 1] = {};
        while (ss >> tok) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) return 2;
            const std::string k = tok.substr(0, eq);
            const uint64_t v = strtoull(tok.c_str() + eq + 1, nullptr, 10);
            if (k == "parts") parts = v;
            else if (k == "n") n = v;
            else if (k == "approx") approx = v;
            else if (k == "free") free_b = v;
            else if (k == "batch") batch = v;
            else if (k == "key_len") key_len = v;
            else if (k == "nq") nq = v;
            else if (k == "value_bytes") value_bytes = v;
            else if (k == "mis") mis = v;
            else if (k == "num_cus") num_cus = v;
            else if (k == "addr") addr = v;
            else if (k == "format") format = v;
            else if (k == "dparts") dparts = v;  // partitions the decode sees (default: parts)
            else if (k.rfind("size", 0) == 0 && strtoull(k.c_str() + 4, nullptr, 10) < GET_MAX_PARTS)
                sizes[strtoull(k.c_str() + 4, nullptr, 10)] = v;
            else return 2;
        }
        const GetLayout l = get_layout(sizes, (int)parts);
        if (dparts == UINT64_MAX) dparts = parts <= GET_MAX_PARTS ? parts : 0;
        const GetRecord r = get_decode(addr, (int)format, sizes, (uint32_t)dparts);
        printf("{");
        J("layout_ok", l.ok), J("total", l.total);
        printf("\"base\":[");
        for (int p = 0; p < l.partitions; ++p) printf("%s%llu", p ? "," : "", (unsigned long long)l.base[p]);
        printf("],");
        J("open_bytes", get_open_bytes(l.total, n, approx != 0)), J("fits", get_open_fits(l.total, n, approx != 0, free_b));
        J("chunk", get_host_chunk(batch, (uint32_t)key_len));
        J("locate_grid", get_locate_grid(nq, (int)num_cus)), J("pieces", piece_count(value_bytes, (uint32_t)mis));
        J("gather_grid", piece_grid(value_bytes, (uint32_t)mis, (int)num_cus));
        J("ok", r.ok), J("part", r.part), J("pos", r.pos), J("limit", r.limit, "}\n");
    }
    return 0;
}
