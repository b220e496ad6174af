// diff_kernels.hip -- two resident databases (get_kernels.hip) compared on
// gfx950: for every slot of database A, what database B holds for that slot's
// key.  k_db_records gave A's descriptors (dump_kernels.hip), k_get_gather
// packed A's keys and k_get_locate gave, per key, where B's value lies (src),
// how long it is and a status:
//   k_diff_lengths  a record per lane: a slot of A that names no record is
//                   BAD_SLOT; FOUND with two different lengths becomes
//                   VALUE_LEN; cmp_len = the bytes to compare (the value's
//                   length when FOUND with equal lengths, else 0)
//   (k_scan_*)      cmp_len -> coff[count + 1]
//   k_diff_values   driven by the bytes to compare, [0, coff[count]), as
//                   k_check_values is: a thread owns 16 of them, finds the
//                   records they belong to in coff (the searches of
//                   piece_copy.hpp) and compares image A and image B in place,
//                   8 bytes a step; a difference stores VALUE_BYTES into the
//                   record's status.  Both positions are u64 at any alignment,
//                   each bounded by its own image.  It has no destination:
//                   nothing else is written.
//   k_diff_report   a record per lane: SAME and VALUE_BYTES counted, the bytes
//                   compared summed, the lowest slot that is not SAME by atomicMin
//   k_diff_select_flags / (k_scan_*) / k_diff_select_scatter
//                   the records whose status bit is set in a mask, in slot
//                   order: a flag per record, the scan of the flags, and the
//                   record's index and four descriptors to position scan[i].
//                   No cursor atomics: the output is deterministic.
// No lane walks a value: a 65 535-byte value is shared by 4 096 threads, a run
// of one-byte values costs what the search costs.  Every read of either image
// goes through the bounded reader sel_gload64, and offsets that are no scan end
// a piece (piece_runs): descriptors, positions and offsets are data, not
// trusted.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "diff_plan.hpp"
#include "check_kernels.hip"  // piece_read_loop, check_status_in

namespace bsdb {

struct DiffArgs {
    const uint8_t *image_a;  // database A's image (GetDb::image)
    uint64_t bytes_a;
    const uint8_t *image_b;  // database B's
    uint64_t bytes_b;
    const uint64_t *vsrc_a;    // [count] k_db_records' on A: the value's position in image A
    const uint32_t *vlen_a;    // [count] its length
    const uint8_t *status_a;   // [count] k_db_records' status
    const uint64_t *src_b;     // [count] locate's on B: the value's position in image B
    const uint32_t *vlen_b;    // [count] its length
    uint8_t *status;           // [count] in: locate's, out: the diff's
    uint64_t count;
    uint32_t *cmp_len;         // [count] bytes to compare
    const uint64_t *coff;      // [count + 1] their scan
    uint64_t slot_base;        // A's slot of record 0 (first_diff is a slot)
    unsigned long long *out;   // the report (FW_WORDS), accumulated
};

// A record per lane; the loop is uniform per wave so the ballots see all
// lanes.  The counts that are final before any byte is compared go out with
// one atomic per wave and counter.
__global__ __launch_bounds__(256) void k_diff_lengths(DiffArgs a) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    uint64_t seen = 0, rejected = 0, mismatch = 0, bad_addr = 0, value_len = 0, bad_slot = 0;  // wave totals
    for (uint64_t base = (uint64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); base < a.count; base += stride) {
        const uint64_t r = base + lane;
        int st = -1;
        if (r < a.count) {
            uint32_t len = 0;
            if (dump_status_in(a.status_a[r]) == DUMP_BAD_ADDR) {
                st = DIFF_BAD_SLOT;  // (no key was looked up: whatever the status array held is not read)
            } else {
                st = check_status_in(a.status[r]);
                if (st == GET_FOUND) {
                    // (a length over 65 535 is none a record's header can hold: never compared)
                    if (a.vlen_a[r] != a.vlen_b[r] || a.vlen_b[r] > CHECK_MAX_VALUE) st = CHECK_VALUE_LEN;
                    else len = a.vlen_b[r];
                }
            }
            a.status[r] = (uint8_t)st;
            a.cmp_len[r] = len;
        }
        seen += __popcll(__ballot(st >= 0));
        rejected += __popcll(__ballot(st == GET_REJECTED));
        mismatch += __popcll(__ballot(st == GET_KEY_MISMATCH));
        bad_addr += __popcll(__ballot(st == GET_BAD_ADDR));
        value_len += __popcll(__ballot(st == CHECK_VALUE_LEN));
        bad_slot += __popcll(__ballot(st == DIFF_BAD_SLOT));
    }
    if (lane != 0) return;
    if (seen) atomicAdd(a.out + FW_SLOTS, (unsigned long long)seen);
    if (rejected) atomicAdd(a.out + FW_REJECTED, (unsigned long long)rejected);
    if (mismatch) atomicAdd(a.out + FW_KEY_MISMATCH, (unsigned long long)mismatch);
    if (bad_addr) atomicAdd(a.out + FW_BAD_ADDR, (unsigned long long)bad_addr);
    if (value_len) atomicAdd(a.out + FW_VALUE_LEN, (unsigned long long)value_len);
    if (bad_slot) atomicAdd(a.out + FW_BAD_SLOT, (unsigned long long)bad_slot);
}

// Whether the n <= 16 bytes at `apos` of image A and at `bpos` of image B
// differ, 8 bytes a step, the last step masked to the bytes that are left.  A
// position past its image reads as 0; one that wraps reads inside the image.
__device__ __forceinline__ bool diff_differ(const DiffArgs &a, uint64_t apos, uint64_t bpos, uint32_t n) {
    uint64_t diff = 0;
    for (uint32_t x = 0; x < n; x += 8) {
        const uint64_t ap = apos + x, bp = bpos + x;
        const uint64_t va = ap < a.bytes_a ? sel_gload64(a.image_a, a.bytes_a, ap) : 0;
        const uint64_t vb = bp < a.bytes_b ? sel_gload64(a.image_b, a.bytes_b, bp) : 0;
        diff |= (va ^ vb) & low_bytes_mask(n - x < 8 ? n - x : 8);
    }
    return diff != 0;
}

// The bytes to compare are coff[count] (read here: the launch does not wait
// for the scan); a piece's owners are the records whose values overlap it.
// Every lane that finds a difference in record q stores the same byte.
__global__ __launch_bounds__(256) void k_diff_values(DiffArgs a) {
    uint64_t qlo, qhi;
    piece_read_loop(
        a.coff[a.count], [&](uint64_t w0, uint64_t w1) { piece_wave_owners(a.coff, a.count, w0, w1, qlo, qhi); },
        [&](const Piece &pc) {
            piece_runs(pc, a.coff, qlo, qhi, [&](uint64_t q, uint64_t start, uint64_t o, uint64_t e) {
                const uint64_t at = o - start;
                // (cmp_len 0: a record that is not FOUND, reached only through offsets that are no scan; it keeps
                // its status, which k_diff_lengths has counted)
                if (a.cmp_len[q] && diff_differ(a, a.vsrc_a[q] + at, a.src_b[q] + at, (uint32_t)(e - o))) a.status[q] = (uint8_t)CHECK_VALUE_BYTES;
            });
        });
}

// The final statuses: SAME and VALUE_BYTES counted (the others were, before
// the compare), the bytes compared, and the lowest slot that is not SAME.
__global__ __launch_bounds__(256) void k_diff_report(DiffArgs a) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    uint64_t same = 0, value_bytes = 0;  // wave totals
    uint64_t bytes = 0;                  // this lane's
    uint64_t first = DIFF_NONE;
    for (uint64_t base = (uint64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); base < a.count; base += stride) {
        const uint64_t r = base + lane;
        int st = -1;
        if (r < a.count) {
            st = (int)a.status[r];
            bytes += a.cmp_len[r];
            if (st != DIFF_SAME && first == DIFF_NONE) first = a.slot_base + r;
        }
        same += __popcll(__ballot(st == DIFF_SAME));
        value_bytes += __popcll(__ballot(st == CHECK_VALUE_BYTES));
    }
    for (int d = 32; d; d >>= 1) {
        bytes += __shfl_xor(bytes, d, 64);
        const uint64_t o = __shfl_xor(first, d, 64);
        first = o < first ? o : first;
    }
    if (lane != 0) return;
    if (same) atomicAdd(a.out + FW_SAME, (unsigned long long)same);
    if (value_bytes) atomicAdd(a.out + FW_VALUE_BYTES, (unsigned long long)value_bytes);
    if (bytes) atomicAdd(a.out + FW_COMPARED_BYTES, (unsigned long long)bytes);
    if (first != DIFF_NONE) atomicMin(a.out + FW_FIRST_DIFF, (unsigned long long)first);
}

struct SelectArgs {
    const uint8_t *status;  // [count] the diff's
    uint64_t count;
    uint32_t mask;          // bit s selects status s (a subset of DIFF_SELECTABLE)
    const uint64_t *ksrc, *vsrc;  // [count] the records' descriptors (k_db_records')
    const uint32_t *klen, *vlen;
    uint32_t *flag;         // [count] 1: selected
    const uint64_t *soff;   // [count + 1] the flags' scan
    uint64_t *sel;          // [count] out: the selected records' indices, ascending
    uint64_t *ksrc_out, *vsrc_out;  // [count] out: their descriptors
    uint32_t *klen_out, *vlen_out;
    uint64_t *nsel;         // out: how many there are
};

__global__ __launch_bounds__(256) void k_diff_select_flags(SelectArgs a) {
    const uint64_t step = (uint64_t)gridDim.x * 256;
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < a.count; r += step) {
        const uint32_t st = a.status[r];
        a.flag[r] = st < DIFF_BAD_SLOT ? (a.mask >> st) & 1u : 0u;  // (a byte that is no code selects nothing)
    }
}

// Record i goes to position soff[i]: positions rise with i, so the order is
// slot order.  A position that is none (offsets that are no scan) moves nothing.
__global__ __launch_bounds__(256) void k_diff_select_scatter(SelectArgs a) {
    const uint64_t step = (uint64_t)gridDim.x * 256;
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < a.count; r += step) {
        if (r == 0) {
            const uint64_t total = a.soff[a.count];
            *a.nsel = total < a.count ? total : a.count;
        }
        const uint64_t p = a.soff[r];
        if (!a.flag[r] || p >= a.count) continue;
        a.sel[p] = r;
        a.ksrc_out[p] = a.ksrc[r], a.vsrc_out[p] = a.vsrc[r];
        a.klen_out[p] = a.klen[r], a.vlen_out[p] = a.vlen[r];
    }
}

}  // namespace bsdb
