// diff_plan.hpp -- what the diff of two resident databases (capi_diff.hip,
// diff_kernels.hip) launches, decided on the host from plain numbers: the
// status codes and the report's words, the mask a selection may carry, and the
// grids (a record per lane; the compare's is piece_grid over the most bytes
// `count` records can hold, because the bytes it compares are known only on
// the device).  C++17 without HIP or getenv, so the arithmetic runs (and is
// checked, tests/diff_plan_check.cpp) without a GPU.
//   The reference has no diff: the nearest it has is Builder's verify
//   (tools/Builder.java:184-228), one getAsBytes per line of the input.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "check_plan.hpp"  // 1 .. 5: the get's and the check's statuses, CHECK_MAX_VALUE
#include "dump_plan.hpp"   // the scan's statuses (DUMP_BAD_ADDR: a slot of A that names no record)

namespace bsdb {

// a slot's status after the diff: 1 .. 3 are the get's, 4 and 5 the check's
enum DiffStatus { DIFF_SAME = 0, DIFF_BAD_SLOT = 6 };
enum DiffWord {
    FW_SLOTS = 0, FW_SAME, FW_REJECTED, FW_KEY_MISMATCH, FW_BAD_ADDR, FW_VALUE_LEN, FW_VALUE_BYTES, FW_BAD_SLOT, FW_FIRST_DIFF,
    FW_COMPARED_BYTES, FW_WORDS
};
constexpr uint64_t DIFF_NONE = ~0ull;  // first_diff when every slot is SAME
// the statuses a selection may name: a BAD_SLOT has no record to write
constexpr uint32_t DIFF_SELECTABLE = (1u << DIFF_BAD_SLOT) - 1;
// bsdb_db_diff's two selections: present in the other side or not, and what it holds there differs
constexpr uint32_t DIFF_MASK_ABSENT = 1u << GET_REJECTED | 1u << GET_KEY_MISMATCH;
constexpr uint32_t DIFF_MASK_UPSERT = DIFF_MASK_ABSENT | 1u << CHECK_VALUE_LEN | 1u << CHECK_VALUE_BYTES;
constexpr uint64_t DIFF_MAX_COUNT = 1ull << 40;  // records of one call: count * 65 535 stays far below 2^64

inline bool diff_bad_mask(uint32_t mask) { return (mask & ~DIFF_SELECTABLE) != 0; }

// k_diff_lengths / k_diff_report / k_diff_select_*: a record per lane, grid-stride
inline uint32_t diff_lane_grid(uint64_t count, int num_cus) { return get_locate_grid(count, num_cus); }

// k_diff_values: a thread per 16 bytes to compare, grid-stride.  How many
// there are (coff[count]) stays on the device; no record compares more than
// CHECK_MAX_VALUE bytes, so `count` of them size the launch, and the stride
// covers whatever the sum is.
inline uint32_t diff_values_grid(uint64_t count, int num_cus) {
    return piece_grid(std::min(count, DIFF_MAX_COUNT) * CHECK_MAX_VALUE, 0, num_cus);
}

}  // namespace bsdb
