// check_plan_check.cpp -- prints what bsdb_amd/csrc/check_plan.hpp decides for
// the cases on stdin, one "key=value ..." line each, as one JSON line per case.
// Built under ASan + UBSan and run by tests/test_check_plan_cpu.py as a program
// of its own; no GPU, no HIP.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

#include "../bsdb_amd/csrc/check_plan.hpp"

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
        const uint64_t bytes = kv["bytes"], count = kv["count"];
        const int cus = (int)kv["num_cus"];
        const CheckFootprint f = check_footprint(bytes);
        printf("{\"split\":%llu,\"blob\":%llu,\"check\":%llu,\"total\":%llu,\"chunk\":%llu,\"lane_grid\":%u,\"values_grid\":%u,"
               "\"words\":%d,\"value_len\":%d,\"value_bytes\":%d,\"record_bytes\":%llu,\"max_value\":%u}\n",
               (unsigned long long)f.split, (unsigned long long)f.blob, (unsigned long long)f.check, (unsigned long long)f.total,
               (unsigned long long)check_chunk_bytes(kv["requested"], kv["free"]), check_lane_grid(count, cus),
               check_values_grid(bytes, cus), (int)CW_WORDS, (int)CHECK_VALUE_LEN, (int)CHECK_VALUE_BYTES,
               (unsigned long long)CHECK_RECORD_BYTES, CHECK_MAX_VALUE);
    }
    return 0;
}
