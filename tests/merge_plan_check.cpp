// merge_plan_check.cpp -- prints what bsdb_amd/csrc/merge_plan.hpp decides for
// the cases on stdin, one "key=value ..." line each, as one JSON line per case.
// sizes=a,b,c: the sizes of a selection's records, scanned here for merge_cut.
// Built under ASan + UBSan and run by tests/test_merge_plan_cpu.py as a program
// of its own; no GPU, no HIP.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../bsdb_amd/csrc/merge_plan.hpp"

using namespace bsdb;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream ss(line);
        std::string tok;
        std::map<std::string, unsigned long long> kv;
        std::vector<uint64_t> roff{0};  // exactly count + 1 entries: a read past the scan is ASan's to report
        while (ss >> tok) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) return 2;
            const std::string key = tok.substr(0, eq);
            if (key == "sizes") {
                const char *s = tok.c_str() + eq + 1;
                while (*s) {
                    char *end;
                    roff.push_back(roff.back() + strtoull(s, &end, 10));
                    s = *end == ',' ? end + 1 : end;
                }
                continue;
            }
            kv[key] = strtoull(tok.c_str() + eq + 1, nullptr, 10);
        }
        const uint64_t count = kv["count"], cap = kv["cap"];
        const int cus = (int)kv["num_cus"], parts = (int)kv["parts"];
        const uint32_t B = (uint32_t)kv["B"], mis = (uint32_t)kv["mis"];
        const MergePlan p = merge_plan(count, cap, parts, B, kv["approx"] != 0, cus);
        const uint64_t record_cap = merge_record_cap(cap, parts, B);
        roff.shrink_to_fit();
        const uint64_t cut = merge_cut(roff.data(), roff.size() - 1, record_cap);
        printf("{\"lane_grid\":%u,\"pack_grid\":%u,\"record_cap\":%llu,\"image_max\":%llu,\"blob_max\":%llu,\"workspace\":%llu,"
               "\"plan_pack_grid\":%u,\"cut\":%llu,\"cut_bytes\":%llu,\"image_of_cut\":%llu,\"second_trip\":%llu,"
               "\"grid_at_second_trip\":%u,\"grid_before\":%u,\"pieces_at\":%llu,\"status\":%d,\"locate_in\":%d,"
               "\"words\":%d,\"kept\":%d,\"replaced\":%d,\"removed\":%d,\"bad_slot\":%d,\"bad_addr\":%d,\"mask_kept\":%u,"
               "\"out_records\":%d,\"max_record\":%u,\"max_count\":%llu}\n",
               merge_lane_grid(count, cus), merge_pack_grid(kv["out_bytes"], mis, cus), (unsigned long long)record_cap,
               (unsigned long long)p.image_max, (unsigned long long)p.blob_max, (unsigned long long)p.workspace, p.pack_grid,
               (unsigned long long)cut, (unsigned long long)(roff[cut] - roff[0]),
               (unsigned long long)merge_image_max(roff[cut] - roff[0], parts, B),
               (unsigned long long)merge_second_trip_bytes(mis, cus), merge_pack_grid(merge_second_trip_bytes(mis, cus), mis, cus),
               merge_pack_grid(merge_second_trip_bytes(mis, cus) - 1, mis, cus),
               (unsigned long long)piece_count(merge_second_trip_bytes(mis, cus), mis),
               merge_status_of((uint8_t)kv["scan"], (uint8_t)kv["delta"], (uint8_t)kv["removed"]), merge_locate_in((uint8_t)kv["delta"]),
               (int)MW_WORDS, (int)MERGE_KEPT, (int)MERGE_REPLACED, (int)MERGE_REMOVED, (int)MERGE_BAD_SLOT, (int)MERGE_BAD_ADDR,
               MERGE_MASK_KEPT, (int)MW_OUT_RECORDS, MERGE_MAX_RECORD, (unsigned long long)MERGE_MAX_COUNT);
    }
    return 0;
}
