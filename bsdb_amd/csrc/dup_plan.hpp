// dup_plan.hpp -- what the duplicate finder (capi_dup.hip, dup_kernels.hip)
// allocates and launches, decided on the host from plain numbers: the passes
// over the bucket ranges (dup_pass_plan), one pass's collect and big-sort
// launches once its key count is known (dup_collect_plan), the chunks of the
// buckets over GB_CMAX keys (dup_over_plan) and the pair list and the classify
// launch (dup_list_plan).  The grouping itself is the build's (gov_group,
// planned by gov_plan.hpp).  Host-only C++17: no HIP, no getenv, so the
// arithmetic runs (and is checked, tests/dup_plan_check.cpp) without a GPU.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "gov_geometry.hpp"

namespace bsdb {

constexpr uint64_t DUP_GRID_MAX = 0xFFFFFFFFull;  // a launch's workgroups stay below 2^32

// device bytes per key of one pass: the sorted signature and its position
// (the build's 16 + 8), plus what the pass's source holds (spill mode)
inline uint64_t dup_pass_bytes_per_key(uint64_t source_bytes_per_key) { return 16 + 8 + source_bytes_per_key; }

struct DupPassPlan {
    uint64_t m = 1;       // buckets of the key set
    uint32_t passes = 1;  // pass p covers buckets [p m / passes, (p + 1) m / passes)
};

// passes = 0: the fewest passes whose working set fits 85 % of the free HBM,
// as the build's passes_build chooses them, without the 12 GB it keeps for
// the solver; at most 64, and never more than there are buckets.
inline DupPassPlan dup_pass_plan(uint64_t n, uint32_t passes, uint64_t free_bytes, uint64_t source_bytes_per_key) {
    DupPassPlan p;
    p.m = n / BUCKET_SIZE + 1;
    if (passes == 0) {
        const double room = 0.85 * (double)free_bytes - 1e9;
        const double need = 1.05 * (double)n * (double)dup_pass_bytes_per_key(source_bytes_per_key);
        passes = room <= 0 ? 64u : (uint32_t)std::min(64.0, std::max(1.0, std::ceil(need / room)));
    }
    p.passes = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(passes, p.m));
    return p;
}

// One pass over nb buckets holding n_local keys, nbig of them listed for the
// big sort (1 665 .. GB_CMAX keys).
struct DupCollectPlan {
    uint32_t collect_grid = 1;   // k_dup_collect: a workgroup per bucket, grid-stride
    uint32_t big_sort_grid = 1;  // k_bucket_sort_big over the listed buckets (launched when there are any)
    size_t slabs_bytes = 0;      // its per-workgroup slabs (signatures + positions)
    uint32_t over_cap = 1;       // buckets over GB_CMAX keys, at most
    uint32_t chunk_cap = 2;      // their chunks, at most
    size_t over_bytes = 0;       // chunk boundaries (u64) + chunk list (u32) + 2 counters
    uint32_t over_grid = 1;      // k_dup_over_list: a thread per bucket
};

inline DupCollectPlan dup_collect_plan(uint64_t nb, uint64_t n_local, uint32_t nbig, int num_cus) {
    DupCollectPlan p;
    const uint64_t cus = (uint64_t)std::max(1, num_cus);
    p.collect_grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(nb, cus * 8));
    p.big_sort_grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(nbig, cus));
    p.slabs_bytes = (size_t)p.big_sort_grid * GB_CMAX * (16 + 8);
    // a bucket over GB_CMAX keys holds at least GB_CMAX + 1 of the pass's keys;
    // its chunks are full but the last: floor(count / GB_CMAX) + 1 at most
    const uint64_t over = n_local / ((uint64_t)GB_CMAX + 1) + 1;
    const uint64_t chunks = n_local / (uint64_t)GB_CMAX + over;
    p.over_cap = (uint32_t)std::min<uint64_t>(over, DUP_GRID_MAX);
    p.chunk_cap = (uint32_t)std::min<uint64_t>(chunks, DUP_GRID_MAX);
    // boundaries: one more than its chunks per bucket
    p.over_bytes = ((size_t)p.chunk_cap + p.over_cap) * 8 + (size_t)p.chunk_cap * 4 + 64;
    p.over_grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((nb + 255) / 256, cus * 16));
    return p;
}

// chunks of one bucket of `count` keys: consecutive slices of at most GB_CMAX
inline uint64_t dup_bucket_chunks(uint64_t count) { return (count + (uint64_t)GB_CMAX - 1) / (uint64_t)GB_CMAX; }

// The chunks the device listed (clamped to what the plan reserved).
struct DupOverPlan {
    uint32_t chunks = 0;                        // (0: nothing to launch)
    uint32_t sort_grid = 1, collect_grid = 1;
    size_t slabs_bytes = 0;
};

inline DupOverPlan dup_over_plan(uint64_t listed_chunks, uint32_t chunk_cap, int num_cus) {
    DupOverPlan p;
    const uint64_t cus = (uint64_t)std::max(1, num_cus);
    p.chunks = (uint32_t)std::min<uint64_t>(listed_chunks, chunk_cap);
    p.sort_grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(p.chunks, cus));
    p.collect_grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(p.chunks, cus * 8));
    p.slabs_bytes = (size_t)p.sort_grid * GB_CMAX * (16 + 8);
    return p;
}

// The caller's pair list and the classify launch over its listed pairs.
struct DupListPlan {
    uint64_t listed = 0;        // min(found, cap); 0: nothing to classify
    bool list_full = false;     // found > cap
    size_t pairs_bytes = 0;     // 2 u64 a pair
    size_t kinds_bytes = 0;     // a byte a pair
    uint32_t classify_grid = 1; // k_dup_classify: a pair per lane, grid-stride
};

inline DupListPlan dup_list_plan(uint64_t found, uint64_t cap, int num_cus) {
    DupListPlan p;
    const uint64_t cus = (uint64_t)std::max(1, num_cus);
    p.listed = std::min(found, cap);
    p.list_full = found > cap;
    p.pairs_bytes = (size_t)cap * 16;
    p.kinds_bytes = (size_t)cap;
    p.classify_grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((p.listed + 255) / 256, cus * 16));
    return p;
}

}  // namespace bsdb
