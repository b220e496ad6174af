// merge_plan.hpp -- what the merge of resident databases (capi_merge.hip,
// merge_kernels.hip) allocates and launches, decided on the host from plain
// numbers: the status codes and the report's words, the status rule itself
// (merge_status_of, which the kernel calls too), the grids, how many record
// bytes one chunk's image may hold under the text-chunk cap and the cut of a
// chunk's selected records to it (merge_cut), the image's bound per layout,
// the device bytes a chunk needs, and the smallest output at which a
// workgroup of the pack goes round its piece loop a second time.  C++17
// without HIP or getenv, so the arithmetic runs (and is checked,
// tests/merge_plan_check.cpp) without a GPU.
//   The reference has no merge: a changed data set is built again from its
//   text (tools/Builder.java:144-176).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "diff_plan.hpp"  // the get's and the scan's statuses, dump_cut, the text plan's bounds

namespace bsdb {

// a slot of `base` after the merge's status kernel
enum MergeStatus { MERGE_KEPT = 0, MERGE_REPLACED = 1, MERGE_REMOVED = 2, MERGE_BAD_SLOT = 3, MERGE_BAD_ADDR = 4 };
enum MergeWord {
    MW_BASE_SLOTS = 0, MW_KEPT, MW_REPLACED, MW_REMOVED, MW_BAD_SLOT, MW_BAD_ADDR, MW_DELTA_SLOTS, MW_DELTA_WRITTEN,
    MW_DELTA_BAD_SLOT, MW_OUT_RECORDS, MW_OUT_KEY_BYTES, MW_OUT_VALUE_BYTES, MW_WORDS
};
// the selection of the records that go on: bsdb_dev_db_select's mask (a subset of DIFF_SELECTABLE)
constexpr uint32_t MERGE_MASK_KEPT = 1u << MERGE_KEPT;
static_assert((MERGE_MASK_KEPT & ~DIFF_SELECTABLE) == 0 && (int)MERGE_BAD_ADDR < (int)DIFF_BAD_SLOT, "the selection reads the merge's statuses");
constexpr uint64_t MERGE_MAX_COUNT = DIFF_MAX_COUNT;
// the longest record an image holds: the lengths are cut as the text pack cuts them
constexpr uint32_t MERGE_MAX_RECORD = TEXT_MAX_RECORD;

// A status byte of locate that is none of its four counts as BAD_ADDR.
BSDB_HD inline int merge_locate_in(uint8_t s) { return s <= GET_BAD_ADDR ? (int)s : (int)GET_BAD_ADDR; }

// The rule.  scan: the slot's own status (k_db_records'); in_delta / in_removed:
// locate's status of the slot's key in that database, GET_REJECTED when there
// is none.  A slot that names no record has no key: nothing else is looked at.
// A damaged delta or removed database (BAD_ADDR) wins over every answer the
// other one gives: the merge stops on it.  REJECTED and KEY_MISMATCH both mean
// absent.
BSDB_HD inline int merge_status_of(uint8_t scan, uint8_t in_delta, uint8_t in_removed) {
    if (dump_status_in(scan) == DUMP_BAD_ADDR) return MERGE_BAD_SLOT;
    const int d = merge_locate_in(in_delta), r = merge_locate_in(in_removed);
    if (d == GET_BAD_ADDR || r == GET_BAD_ADDR) return MERGE_BAD_ADDR;
    if (d == GET_FOUND) return MERGE_REPLACED;
    return r == GET_FOUND ? MERGE_REMOVED : MERGE_KEPT;
}

// k_merge_status / k_rec_sizes / k_rec_outputs: a record per lane, grid-stride
inline uint32_t merge_lane_grid(uint64_t count, int num_cus) { return get_locate_grid(count, num_cus); }

// k_rec_pack / k_rec_pack_blocked: a thread per aligned 16-byte piece of the destination
inline uint32_t merge_pack_grid(uint64_t out_bytes, uint32_t misalign, int num_cus) { return piece_grid(out_bytes, misalign, num_cus); }

// The smallest destination (at `misalign`) at which some workgroup of the pack
// takes a second trip of its piece loop: one piece more than the largest grid holds.
inline uint64_t merge_second_trip_bytes(uint32_t misalign, int num_cus) {
    const uint64_t pieces = (uint64_t)std::max(1, num_cus) * 32 * 256;  // (piece_grid's cap x 256 threads)
    return pieces * 16 - (misalign & 15) + 1;
}

// An upper bound of the image of records that take `record_bytes` bytes
// (headers included) in `partitions` runs.  Compact: the records themselves.
// Blocked, by text_image_max_blocked's reasoning: two consecutive blocks of a
// run hold more than B bytes together, so all but the last block of a run cost
// at most twice what they hold and the last at most B; a large record (size >
// B >= 4096) gets less than size + 4096 < 2 x size.  Together < 2 R + P x B.
inline uint64_t merge_image_max(uint64_t record_bytes, int partitions, uint32_t B) {
    return B ? 2 * record_bytes + (uint64_t)std::max(1, partitions) * B + 16 : record_bytes + 16;
}

// The record bytes a chunk may hold so that its image stays under `cap` (the
// cap of bsdb_db_set_text_chunk): merge_image_max inverted.  0 when the cap
// holds no such image: a record then goes alone (merge_cut).
inline uint64_t merge_record_cap(uint64_t cap, int partitions, uint32_t B) {
    if (!B) return cap > 16 ? cap - 16 : 0;
    const uint64_t fixed = (uint64_t)std::max(1, partitions) * B + 16;
    return cap > fixed ? (cap - fixed) / 2 : 0;
}

// The records of a chunk's selection that one pack writes: the largest k <=
// count whose sizes, h_roff[k] - h_roff[0] (the scan of 3 + kLen + vLen, count
// + 1 entries), fit record_cap; at least 1, so a single record above the cap
// goes alone and the form advances whatever the cap.  dump_cut's rule.
inline uint64_t merge_cut(const uint64_t *h_roff, uint64_t count, uint64_t record_cap) { return dump_cut(h_roff, count, record_cap); }

// What one chunk of nk slots holds on the device besides the context's
// workspace, when the pack writes `cut_records` records of `record_bytes`
// bytes: the descriptors and statuses of the slots and of the selection, the
// packed keys for locate (<= 255 x nk), locate's answers in two databases, the
// cut's sizes and scan, and the pack's outputs.
struct MergePlan {
    uint32_t lane_grid = 1;       // a slot per lane
    uint32_t pack_grid = 1;       // the image pack at image_max bytes
    uint64_t record_cap = 0;      // merge_record_cap
    uint64_t image_max = 0;       // the image buffer of one pack
    uint64_t blob_max = 0;        // the key blob of one pack
    uint64_t workspace = 0;       // device bytes of one chunk
};

inline MergePlan merge_plan(uint64_t nk, uint64_t text_cap, int partitions, uint32_t B, bool approximate, int num_cus) {
    MergePlan p;
    nk = std::min(nk, MERGE_MAX_COUNT);  // (a call holds no more: the products below stay under 2^60)
    p.lane_grid = merge_lane_grid(nk, num_cus);
    p.record_cap = merge_record_cap(text_cap, partitions, B);
    // a pack holds at most nk records, and at most record_cap bytes unless one record goes alone
    const uint64_t records = std::min<uint64_t>(nk * MERGE_MAX_RECORD, std::max<uint64_t>(p.record_cap, MERGE_MAX_RECORD));
    p.image_max = merge_image_max(records, partitions, B);
    p.blob_max = std::min<uint64_t>(nk * TEXT_MAX_KEY, records) + 16;
    p.pack_grid = merge_pack_grid(p.image_max, 0, num_cus);
    const uint64_t slots = 2 * (2 * 8 + 2 * 4) * nk + 8 * nk + 3 * nk;           // descriptors twice, sel, three status arrays
    const uint64_t locate = 8 * (nk + 1) + TEXT_MAX_KEY * nk + 16 + 2 * (8 + 4 + 1) * nk;  // key offsets, keys, two answers
    const uint64_t cut = 4 * 2 * nk + 8 * (nk + 1);                                // sizes and their scan
    const uint64_t outs = p.image_max + p.blob_max + 8 * (nk + 1) + 8 * nk + (approximate ? 9 * nk : 0);
    p.workspace = slots + locate + cut + outs + (B ? text_place_workspace(nk) : 8 * (nk + 1)) + 8 * MW_WORDS + 64;
    return p;
}

}  // namespace bsdb
