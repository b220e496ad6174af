// dup_plan_check.cpp -- prints the duplicate finder's plans (dup_plan.hpp) as
// JSON lines for the cases on stdin, one case per line of name=value tokens:
// the pass plan of n keys (passes, free, source_bpk), the collect plan of one
// pass (nb, n_local, nbig, num_cus), the chunks of one bucket of `count` keys,
// the over plan for `listed` chunks, and the list plan (found, cap).  Built
// and run by tests/test_dup_plan_cpu.py; no GPU, no HIP.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "../bsdb_amd/csrc/dup_plan.hpp"

using namespace bsdb;

static void J(const char *k, unsigned long long v, const char *end = ",") { printf("\"%s\":%llu%s", k, v, end); }

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream ss(line);
        std::string tok;
        uint64_t n = 0, passes = 0, free_b = 0, source_bpk = 0, nb = 1, n_local = 0, nbig = 0, num_cus = 256, count = 0,
                 listed = 0, found = 0, cap = 0;
        while (ss >> tok) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) return 2;
            const std::string k = tok.substr(0, eq);
            const uint64_t v = strtoull(tok.c_str() + eq + 1, nullptr, 10);
            if (k == "n") n = v;
            else if (k == "passes") passes = v;
            else if (k == "free") free_b = v;
            else if (k == "source_bpk") source_bpk = v;
            else if (k == "nb") nb = v;
            else if (k == "n_local") n_local = v;
            else if (k == "nbig") nbig = v;
            else if (k == "num_cus") num_cus = v;
            else if (k == "count") count = v;
            else if (k == "listed") listed = v;
            else if (k == "found") found = v;
            else if (k == "cap") cap = v;
            else return 2;
        }
        const DupPassPlan pp = dup_pass_plan(n, (uint32_t)passes, free_b, source_bpk);
        const DupCollectPlan cp = dup_collect_plan(nb, n_local, (uint32_t)nbig, (int)num_cus);
        const DupOverPlan op = dup_over_plan(listed, cp.chunk_cap, (int)num_cus);
        const DupListPlan lp = dup_list_plan(found, cap, (int)num_cus);
        printf("{");
        J("m", pp.m), J("passes", pp.passes), J("bytes_per_key", dup_pass_bytes_per_key(source_bpk));
        J("collect_grid", cp.collect_grid), J("big_sort_grid", cp.big_sort_grid), J("slabs_bytes", cp.slabs_bytes);
        J("over_cap", cp.over_cap), J("chunk_cap", cp.chunk_cap), J("over_bytes", cp.over_bytes), J("over_grid", cp.over_grid);
        J("bucket_chunks", dup_bucket_chunks(count));
        J("chunks", op.chunks), J("over_sort_grid", op.sort_grid), J("over_collect_grid", op.collect_grid);
        J("over_slabs_bytes", op.slabs_bytes);
        J("listed", lp.listed), J("list_full", lp.list_full), J("pairs_bytes", lp.pairs_bytes), J("kinds_bytes", lp.kinds_bytes);
        J("classify_grid", lp.classify_grid, "}\n");
    }
    return 0;
}
