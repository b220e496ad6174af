// hist_geometry.hpp -- tile and bin geometry of the histogram kernels, shared
// by the kernels (hash_kernels.hip) and the host's launch planner
// (hist_plan.hpp).  Plain C++: no HIP.
#pragma once
#include <stdint.h>

namespace bsdb {

constexpr int P1_THREADS = 512;
constexpr int P1_KEYS_PER_THREAD = 16;
constexpr int P1_TILE = P1_THREADS * P1_KEYS_PER_THREAD;  // 8192 keys per workgroup
constexpr int PART_SHIFT = 15;                            // 32768 buckets per partition
constexpr int PART_BUCKETS = 1 << PART_SHIFT;
constexpr int MAX_PARTS = 512;
constexpr int NCOPY = 8;                                  // cursor/region copies (one per XCD)

// P1Args::scratch: words before the per-workgroup part, workgroups at most
constexpr uint32_t P1_SCRATCH_WG = 10240;
constexpr uint32_t P1_SCRATCH_MAXWG = 2048;

// k_pass1_d13 (13-byte keys past k_pass1_d13e's bins)
constexpr int D13_NT = 512;

// k_pass1_d13e
constexpr int D13E_NT = 1024;
constexpr int D13E_TILE = D13E_NT * P1_KEYS_PER_THREAD;  // 16384
constexpr int D13E_BIN_IDS = 36864;  // ids per bin buffer: nparts * capb (72 KiB, two buffers)
constexpr int D13E_MAXP = 288;       // bins (capb >= 128 ids: tile share 57 +- 7.5 at 288 bins)

// k_pass1_vare
constexpr int VARE_NT = 512;
constexpr int VARE_NG = 8;                         // groups of 128 keys per wave per tile
constexpr int VARE_TILE = VARE_NT * 2 * VARE_NG;   // 8192 keys
constexpr int VARE_BIN_IDS = 18432;                // ids in the bins (36 KiB)
constexpr int VARE_MAXP = 144;

}  // namespace bsdb
