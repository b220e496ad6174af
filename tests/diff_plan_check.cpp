// diff_plan_check.cpp -- prints what bsdb_amd/csrc/diff_plan.hpp decides for
// the cases on stdin, one "key=value ..." line each, as one JSON line per case.
// Built under ASan + UBSan and run by tests/test_diff_plan_cpu.py as a program
// of its own; no GPU, no HIP.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

#include "../bsdb_amd/csrc/diff_plan.hpp"

using namespace bsdb;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream ss(line);
        std::string tok;
        std::map<std::string, unsigned long long> kv;
        while (ss >> tok) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) return 2;
            kv[tok.substr(0, eq)] = strtoull(tok.c_str() + eq + 1, nullptr, 10);
        }
        const uint64_t count = kv["count"];
        const int cus = (int)kv["num_cus"];
        printf("{\"lane_grid\":%u,\"values_grid\":%u,\"bad_mask\":%d,\"words\":%d,\"same\":%d,\"bad_slot\":%d,\"first_diff\":%d,"
               "\"compared_bytes\":%d,\"selectable\":%u,\"mask_absent\":%u,\"mask_upsert\":%u,\"max_count\":%llu}\n",
               diff_lane_grid(count, cus), diff_values_grid(count, cus), (int)diff_bad_mask((uint32_t)kv["mask"]), (int)FW_WORDS,
               (int)DIFF_SAME, (int)DIFF_BAD_SLOT, (int)FW_FIRST_DIFF, (int)FW_COMPARED_BYTES, DIFF_SELECTABLE, DIFF_MASK_ABSENT,
               DIFF_MASK_UPSERT, (unsigned long long)DIFF_MAX_COUNT);
    }
    return 0;
}
