// gov_geometry.hpp -- workgroup, bucket and range geometry of the GOV build
// kernels, shared by the kernels (gov_kernels.hip) and the host's plan
// (gov_plan.hpp).  Plain C++: no HIP.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace bsdb {

constexpr size_t CU_LDS_BYTES = 160 * 1024;  // LDS of one CU (gfx950)

#ifndef BSDB_PROBE_BUCKET_SIZE
constexpr uint32_t BUCKET_SIZE = 1500;          // keys per bucket on average (GOV:281)
#else
// (measurement builds only, tools/build_variant.sh: a different mean bucket
// to price the solver's LDS footprint; never the product library)
constexpr uint32_t BUCKET_SIZE = BSDB_PROBE_BUCKET_SIZE;
#endif

#ifndef GOV_THREADS
#define GOV_THREADS 512  // workgroup size of the solver
#endif
constexpr int GS_THREADS = GOV_THREADS;
// Two solver workgroups per CU (LDS <= 80 KiB each): one's single-wave
// phases (greedy, BFS, FVS selection) overlap the other's.  4.2 sigma above
// the mean bucket; larger buckets (~1e-5 of them) take the global-slab path.
#ifndef GOV_PER_CU
#define GOV_PER_CU 2
#endif
#ifndef GOV_CMAX
#define GOV_CMAX 1664
#endif
// (GOV_PER_CU / GOV_CMAX other than 2 / 1664: measurement builds only,
// tools/build_variant.sh, with BSDB_PROBE_BUCKET_SIZE)
constexpr int GS_PER_CU = GOV_PER_CU;
constexpr int GS_CMAX = GOV_CMAX;    // keys per bucket solved in LDS (expected ~1500, sigma ~39)
// Oversized buckets (adversarial or skewed key sets: > GS_CMAX keys, 14 sigma
// above the mean for random keys) are solved by the same code with its state
// in a per-workgroup slab of global memory, up to GB_CMAX keys.
constexpr int GB_CMAX = 16384;  // a power of two (the bitonic sort's padding)
// Oversized buckets up to GM_CMAX keys (every one of a random key set: the
// largest of C4's 8.8 M buckets holds ~1 720) are solved with their state in
// LDS by k_gov_solve_mid, one workgroup per CU; only larger (adversarial)
// buckets take the global-slab kernel, whose every state access goes to L2.
constexpr int GM_CMAX = 2048;
// FVS: most heavy hinges of a block (a larger set falls back to Gauss-Jordan
// over the whole block).  SolveArgs::fvs_max may lower it (tests force the
// fallback with it); the result is the block's unique solution either way.
constexpr uint32_t FVS_NH_MAX = 380;

// grouping by bucket: a range of at most SMALL_NB buckets is counted in LDS
// by chunks of SMALL_CHUNK keys, one of at most MID_NB buckets by 16-bit LDS
// counters per workgroup (the kernels' comments in gov_kernels.hip)
constexpr uint32_t SMALL_NB = 4096, SMALL_KPT = 16, SMALL_CHUNK = 256 * SMALL_KPT;
constexpr uint32_t MID_NB = 80000, MID_THREADS = 1024;

constexpr int OWN_MAXR = 64;  // owners (ranks) of k_owner_count / k_owner_scatter at most

}  // namespace bsdb
