// check_plan.hpp -- what the check of a database against text input
// (capi_check.hip, check_kernels.hip) allocates and launches, decided on the
// host from plain numbers: the status codes and the report's words, the grids
// (a record per lane; the compare's is piece_grid over the chunk, because the
// bytes it compares are known only on the device), a chunk's device footprint
// (check_footprint) and the chunk size (check_chunk_bytes).  C++17 without HIP
// or getenv, so the arithmetic runs (and is checked, tests/check_plan_check.cpp)
// without a GPU.
//   tools/Builder.java:184-228 (the second read of the input, getAsBytes per record)
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "get_plan.hpp"   // the statuses the locate leaves (GET_*)
#include "text_plan.hpp"  // the split's footprint, the chunk limits

namespace bsdb {

// a record's status after the check: 0 .. 3 are the get's, then the value's
enum CheckStatus { CHECK_OK = 0, CHECK_VALUE_LEN = 4, CHECK_VALUE_BYTES = 5 };
enum CheckWord {
    CW_RECORDS = 0, CW_OK, CW_REJECTED, CW_KEY_MISMATCH, CW_BAD_ADDR, CW_VALUE_LEN, CW_VALUE_BYTES, CW_FIRST_BAD, CW_WORDS
};
constexpr uint64_t CHECK_NONE = ~0ull;       // first_bad when every record is OK
constexpr uint64_t CHECK_RECORD_BYTES = 25;  // src u64, dbvlen u32, status u8, cmp_len u32, coff u64
constexpr uint32_t CHECK_MAX_VALUE = 65535;  // the record header's vLen is a u16: no located value is longer

// k_check_lengths / k_check_approx / k_check_report: a record per lane, grid-stride
inline uint32_t check_lane_grid(uint64_t count, int num_cus) { return text_lane_grid(count, num_cus); }

// k_check_values: a thread per 16 bytes to compare, grid-stride.  How many
// there are (coff[count]) stays on the device; they are value bytes of the
// chunk, so the chunk's length sizes the launch and the stride covers a sum
// that is larger (descriptors that overlap).
inline uint32_t check_values_grid(uint64_t text_bytes, int num_cus) { return piece_grid(text_bytes, 0, num_cus); }

// Device bytes of one chunk of `bytes` text bytes (< 2^32, so every sum stays
// below 2^40): the text and its split at the worst case (every byte a line and
// a separator) with the descriptors; the key blob with its offsets and the
// pack's two size arrays and size scan; CHECK_RECORD_BYTES per record at the
// most records the chunk can hold, and the scan's last entry.
struct CheckFootprint {
    uint64_t split = 0;  // text (+16 B of slack), the split's workspace, the descriptors
    uint64_t blob = 0;   // key blob + offsets, the records' sizes and their scan
    uint64_t check = 0;  // src, dbvlen, status, cmp_len, coff
    uint64_t total = 0;
};

inline CheckFootprint check_footprint(uint64_t bytes) {
    CheckFootprint f;
    const uint64_t r = text_max_records(bytes);
    f.split = bytes + 16 + text_footprint(bytes, bytes, bytes, false).split + 4 * 4 * r;
    f.blob = text_blob_max(bytes) + 8 * (r + 1) + 2 * 4 * r + 8 * (r + 1);
    f.check = CHECK_RECORD_BYTES * r + 8;
    f.total = f.split + f.blob + f.check;
    return f;
}

// The chunk size: what bsdb_text_set_chunk asked for (0 = default), at least
// TEXT_MIN_CHUNK, below 2^32, and halved until its footprint fits half of
// `free_bytes`, the device memory that is free beside the resident image (the
// figure is taken with the database open, so the image's size does not enter).
inline uint64_t check_chunk_bytes(uint64_t requested, uint64_t free_bytes) {
    uint64_t c = requested ? requested : TEXT_DEFAULT_CHUNK;
    c = std::min<uint64_t>(std::max<uint64_t>(c, TEXT_MIN_CHUNK), TEXT_MAX_BYTES & ~15ull);
    while (c > TEXT_MIN_CHUNK && check_footprint(c).total > free_bytes / 2) c = std::max<uint64_t>(TEXT_MIN_CHUNK, c / 2);
    return c;
}

}  // namespace bsdb
