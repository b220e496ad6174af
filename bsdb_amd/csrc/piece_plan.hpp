// piece_plan.hpp -- the launch of an output-driven copy (piece_copy.hpp: the
// get gather and the text packs): a thread per aligned 16-byte piece of the
// destination, grid-stride.  `misalign` = the destination pointer's low 4
// bits: the pieces start at the aligned address below it.  C++17 without HIP,
// shared by get_plan.hpp and text_plan.hpp (and checked with them).
#pragma once
#include <algorithm>
#include <cstdint>

#if defined(__HIPCC__)
#define BSDB_HD __host__ __device__
#else
#define BSDB_HD
#endif

namespace bsdb {

constexpr uint64_t PIECE_GRID_MAX = 0xFFFFFFFFull;  // a launch's workgroups stay below 2^32

BSDB_HD inline uint64_t piece_count(uint64_t out_bytes, uint32_t misalign) {
    // ceil((out_bytes + misalign) / 16) without a sum that could wrap
    return out_bytes ? (out_bytes >> 4) + (((out_bytes & 15) + (misalign & 15) + 15) >> 4) : 0;
}

inline uint32_t piece_grid(uint64_t out_bytes, uint32_t misalign, int num_cus) {
    const uint64_t cus = (uint64_t)std::max(1, num_cus);
    const uint64_t pieces = piece_count(out_bytes, misalign);
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>({(pieces >> 8) + ((pieces & 255) != 0), cus * 32, PIECE_GRID_MAX}));
}

}  // namespace bsdb
