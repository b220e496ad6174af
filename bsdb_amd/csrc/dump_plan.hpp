// dump_plan.hpp -- what the enumeration of a resident database by slot
// (capi_dump.hip, dump_kernels.hip) allocates and launches, decided on the
// host from plain numbers: the status codes and the report's words, a
// record's line length and the length part of the text test (both called by
// the kernels too), the grids, the text-chunk cap and the cut of a chunk of
// records to it (dump_cut).  C++17 without HIP or getenv, so the arithmetic
// runs (and is checked, tests/dump_plan_check.cpp) without a GPU.
//   write/kv/KVWriter.java forEach / partitionForEach is the nearest the
//   reference has (file order, for buildIndex); it has no dump.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "get_plan.hpp"   // the record-per-lane grid (get_locate_grid), piece_grid
#include "text_plan.hpp"  // what a line may hold to read back: TEXT_MAX_KEY, TEXT_MAX_VALUE

namespace bsdb {

enum DumpStatus { DUMP_OK = 0, DUMP_BAD_ADDR = 1, DUMP_NOT_TEXT = 2 };
enum DumpWord { DW_SLOTS = 0, DW_OK, DW_BAD_ADDR, DW_NOT_TEXT, DW_KEY_BYTES, DW_VALUE_BYTES, DW_TEXT_BYTES, DW_FIRST_BAD, DW_WORDS };
constexpr uint64_t DUMP_NONE = ~0ull;            // first_bad when every slot is OK
constexpr uint32_t DUMP_MAX_KEY = 255;           // the record header's kLen is a u8,
constexpr uint32_t DUMP_MAX_VALUE = 65535;       // its vLen a u16
constexpr uint64_t DUMP_MAX_LINE = DUMP_MAX_KEY + DUMP_MAX_VALUE + 2;  // key, separator, value, '\n'
constexpr uint64_t DUMP_DEFAULT_CHUNK = 256ull << 20;

// The lengths the text kernels work with: a descriptor's, cut to what a
// header can hold, so that a line's length and the bytes copied always agree.
BSDB_HD inline uint32_t dump_klen(uint32_t klen) { return klen < DUMP_MAX_KEY ? klen : DUMP_MAX_KEY; }
BSDB_HD inline uint32_t dump_vlen(uint32_t vlen) { return vlen < DUMP_MAX_VALUE ? vlen : DUMP_MAX_VALUE; }

// A status byte that is none of the three counts as BAD_ADDR: a report's sum holds for any input.
BSDB_HD inline int dump_status_in(uint8_t s) { return s == DUMP_OK || s == DUMP_NOT_TEXT ? (int)s : (int)DUMP_BAD_ADDR; }

// Bytes of a record's line "key<sep>value\n"; a BAD_ADDR slot writes nothing.
BSDB_HD inline uint32_t dump_line_len(int status, uint32_t klen, uint32_t vlen) {
    return status == DUMP_BAD_ADDR ? 0 : dump_klen(klen) + 1 + dump_vlen(vlen) + 1;
}

// The length part of the text test: a line with an empty key, an empty value
// or a value over the text front end's limit does not read back as its record
// (text_line_verdict: EMPTY_KEY, NOT_TWO_FIELDS, TOO_LARGE).  A key over 255
// bytes is none a header holds.  The bytes' part is k_dump_text's.
BSDB_HD inline int dump_length_status(int status, uint32_t klen, uint32_t vlen) {
    if (status == DUMP_BAD_ADDR) return status;
    return klen == 0 || klen > TEXT_MAX_KEY || vlen == 0 || vlen > TEXT_MAX_VALUE ? (int)DUMP_NOT_TEXT : (int)DUMP_OK;
}

// k_db_records / k_dump_lengths / k_dump_report: a record per lane, grid-stride
inline uint32_t dump_lane_grid(uint64_t count, int num_cus) { return get_locate_grid(count, num_cus); }

// k_dump_text: a thread per aligned 16-byte piece of the text
inline uint32_t dump_text_grid(uint64_t text_bytes, uint32_t misalign, int num_cus) { return piece_grid(text_bytes, misalign, num_cus); }

// bsdb_db_set_text_chunk: 0 is the default; a cap must hold the longest line
inline bool dump_bad_chunk(uint64_t bytes) { return bytes != 0 && bytes < DUMP_MAX_LINE; }
inline uint64_t dump_chunk_bytes(uint64_t requested) { return requested ? requested : DUMP_DEFAULT_CHUNK; }

// The records of a chunk that the host form writes in one step: the largest
// k <= count whose lines, h_loff[k] - h_loff[0] bytes (h_loff: the scan of
// the line lengths, count + 1 entries), fit `cap`; at least 1, so the form
// advances whatever the cap (0 when the chunk is empty).
inline uint64_t dump_cut(const uint64_t *h_loff, uint64_t count, uint64_t cap) {
    if (!count) return 0;
    uint64_t lo = 1, hi = count;  // the answer lies in [lo, hi]; h_loff does not decrease
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (h_loff[mid] - h_loff[0] <= cap) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

}  // namespace bsdb
