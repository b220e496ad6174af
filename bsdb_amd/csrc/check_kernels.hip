// check_kernels.hip -- a database checked against text input on gfx950: for
// every record of a chunk of text resident in HBM, what the resident database
// (get_kernels.hip) returns for its key against the value the text holds.  What
// Builder's verify does one getAsBytes per line (tools/Builder.java:184-228),
// after the split (text_kernels.hip) gave the descriptors and k_get_locate gave,
// per key, where the database's value lies (src), how long it is (dbvlen) and
// a status:
//   k_check_lengths  a record per lane: FOUND with two different lengths
//                    becomes VALUE_LEN; cmp_len = the bytes to compare (the
//                    value's length when FOUND with equal lengths, else 0)
//   (k_scan_*)       cmp_len -> coff[count + 1]
//   k_check_values   driven by the bytes to compare, [0, coff[count]), as
//                    k_get_gather is by its output: a thread owns 16 of them,
//                    finds the records they belong to in coff (the searches of
//                    piece_copy.hpp) and compares text and image in place, 8
//                    bytes a step; a difference stores VALUE_BYTES into the
//                    record's status.  It has no destination: nothing else is
//                    written, and no value is gathered.
//   k_check_approx   approximate mode instead of the three above: the slot's 8
//                    bytes against the value head the text front end stores
//                    (text_value_head); no length status
//   k_check_report   a record per lane: OK and VALUE_BYTES counted, the first
//                    record that is not OK by atomicMin
// No lane walks a value: a 32 510-byte value is shared by 2 032 threads, a run
// of one-byte values costs what the search costs.  Every read of the text and
// of the image goes through the bounded reader sel_gload64, and offsets that
// are no scan end a piece (piece_runs): descriptors, positions and offsets are
// data, not trusted.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "check_plan.hpp"
#include "get_kernels.hip"
#include "text_kernels.hip"

namespace bsdb {

struct CheckArgs {
    const uint8_t *text;       // the chunk
    uint64_t text_bytes;       // < 2^32
    const uint8_t *image;      // the database's (GetDb::image)
    uint64_t image_bytes;
    const uint32_t *vpos, *vlen;  // [count] the split's value descriptors
    const uint64_t *src;          // [count] locate's: the value's position in the image (approximate: the slot)
    const uint32_t *dbvlen;       // [count] locate's: its length
    uint8_t *status;              // [count] in: locate's, out: the check's
    uint64_t count;
    uint32_t *cmp_len;            // [count] bytes to compare
    const uint64_t *coff;         // [count + 1] their scan
    uint64_t record_base;         // input-order index of record 0 (first_bad is global)
    unsigned long long *out;      // the report (CW_WORDS), accumulated
};

// The wave's counts of the statuses that are final before any byte is
// compared, one atomic per wave and counter; st < 0: no record in this lane.
struct CheckCounts {
    uint64_t seen = 0, rejected = 0, mismatch = 0, bad_addr = 0, value_len = 0;
    __device__ __forceinline__ void add(int st) {
        seen += __popcll(__ballot(st >= 0));
        rejected += __popcll(__ballot(st == GET_REJECTED));
        mismatch += __popcll(__ballot(st == GET_KEY_MISMATCH));
        bad_addr += __popcll(__ballot(st == GET_BAD_ADDR));
        value_len += __popcll(__ballot(st == CHECK_VALUE_LEN));
    }
    __device__ __forceinline__ void flush(unsigned long long *out) const {
        if ((threadIdx.x & 63) != 0) return;
        if (seen) atomicAdd(out + CW_RECORDS, (unsigned long long)seen);
        if (rejected) atomicAdd(out + CW_REJECTED, (unsigned long long)rejected);
        if (mismatch) atomicAdd(out + CW_KEY_MISMATCH, (unsigned long long)mismatch);
        if (bad_addr) atomicAdd(out + CW_BAD_ADDR, (unsigned long long)bad_addr);
        if (value_len) atomicAdd(out + CW_VALUE_LEN, (unsigned long long)value_len);
    }
};

// A status byte that is none of the get's counts as BAD_ADDR: the report's sum holds for any input.
__device__ __forceinline__ int check_status_in(uint8_t s) { return s <= GET_BAD_ADDR ? (int)s : (int)GET_BAD_ADDR; }

// A record per lane; the loop is uniform per wave so the ballots see all lanes.
__global__ __launch_bounds__(256) void k_check_lengths(CheckArgs a) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    CheckCounts n;
    for (uint64_t base = (uint64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); base < a.count; base += stride) {
        const uint64_t r = base + lane;
        int st = -1;
        if (r < a.count) {
            st = check_status_in(a.status[r]);
            uint32_t len = 0;
            if (st == GET_FOUND) {
                // (a length over 65 535 is none a record's header can hold: never compared, whatever the text says)
                if (a.vlen[r] != a.dbvlen[r] || a.dbvlen[r] > CHECK_MAX_VALUE) st = CHECK_VALUE_LEN;
                else len = a.dbvlen[r];
            }
            a.status[r] = (uint8_t)st;
            a.cmp_len[r] = len;
        }
        n.add(st);
    }
    n.flush(a.out);
}

// The piece loop of piece_copy.hpp without a destination: piece k is bytes
// [16 k, 16 k + 16) of the `bytes` to read, cut to them (the misalignment is
// 0), and nothing is stored when it is done.  wave(w0, w1) runs on every lane
// before the lanes without a piece leave; piece(pc) runs no wave-wide operation.
template <class Wave, class Read>
__device__ __forceinline__ void piece_read_loop(uint64_t bytes, const Wave &wave, const Read &piece) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t pieces = piece_count(bytes, 0);
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    auto end_of = [&](uint64_t kk) -> uint64_t { return bytes - kk * 16 < 16 ? bytes : kk * 16 + 16; };
    for (uint64_t wbase = (uint64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); wbase < pieces; wbase += stride) {
        const uint64_t k = wbase + lane;
        const uint64_t klast = pieces - wbase > 63 ? wbase + 63 : pieces - 1;
        wave(wbase * 16, end_of(klast));
        if (k >= pieces) continue;  // (no wave-wide operation below)
        Piece pc;
        pc.o0 = k * 16, pc.o1 = end_of(k);
        pc.j0 = 0;
        piece(pc);
    }
}

// Whether the n <= 16 bytes at `tpos` of the text and at `ipos` of the image
// differ, 8 bytes a step, the last step masked to the bytes that are left.
__device__ __forceinline__ bool check_differ(const CheckArgs &a, uint64_t tpos, uint64_t ipos, uint32_t n) {
    uint64_t diff = 0;
    for (uint32_t x = 0; x < n; x += 8) {
        const uint64_t tp = tpos + x, ip = ipos + x;
        const uint64_t t = tp < a.text_bytes ? sel_gload64(a.text, a.text_bytes, tp) : 0;
        const uint64_t d = ip < a.image_bytes ? sel_gload64(a.image, a.image_bytes, ip) : 0;
        diff |= (t ^ d) & low_bytes_mask(n - x < 8 ? n - x : 8);
    }
    return diff != 0;
}

// The bytes to compare are coff[count] (read here: the launch does not wait
// for the scan); a piece's owners are the records whose values overlap it.
// Every lane that finds a difference in record q stores the same byte.
__global__ __launch_bounds__(256) void k_check_values(CheckArgs a) {
    uint64_t qlo, qhi;
    piece_read_loop(
        a.coff[a.count], [&](uint64_t w0, uint64_t w1) { piece_wave_owners(a.coff, a.count, w0, w1, qlo, qhi); },
        [&](const Piece &pc) {
            piece_runs(pc, a.coff, qlo, qhi, [&](uint64_t q, uint64_t start, uint64_t o, uint64_t e) {
                const uint64_t at = o - start;
                if (check_differ(a, a.vpos[q] + at, a.src[q] + at, (uint32_t)(e - o))) a.status[q] = (uint8_t)CHECK_VALUE_BYTES;
            });
        });
}

// Approximate mode, a record per lane: src is the slot, the slot holds the
// value head (false positives of absent keys differ from it, or do not).
__global__ __launch_bounds__(256) void k_check_approx(CheckArgs a) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    CheckCounts n;
    for (uint64_t base = (uint64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); base < a.count; base += stride) {
        const uint64_t r = base + lane;
        int st = -1;
        if (r < a.count) {
            st = check_status_in(a.status[r]);
            if (st == GET_FOUND) {
                uint32_t l;
                const uint64_t head = text_value_head(a.text, a.text_bytes, a.vpos[r], a.vlen[r], l);
                const uint64_t slot = a.src[r];
                const bool inside = slot < a.image_bytes / 8;
                if (!inside || sel_gload64(a.image, a.image_bytes, slot * 8) != head) st = CHECK_VALUE_BYTES;
            }
            a.status[r] = (uint8_t)st;
        }
        n.add(st == CHECK_VALUE_BYTES ? (int)CHECK_OK : st);  // (OK and VALUE_BYTES are k_check_report's)
    }
    n.flush(a.out);
}

// The final statuses: OK and VALUE_BYTES counted (the others were, before the
// compare), and the first record in input order that is not OK.
__global__ __launch_bounds__(256) void k_check_report(const uint8_t *status, uint64_t count, uint64_t record_base,
                                                      unsigned long long *out) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    uint64_t ok = 0, value_bytes = 0;  // wave totals
    uint64_t first = CHECK_NONE;       // this lane's
    for (uint64_t base = (uint64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); base < count; base += stride) {
        const uint64_t r = base + lane;
        const int st = r < count ? (int)status[r] : -1;
        ok += __popcll(__ballot(st == CHECK_OK));
        value_bytes += __popcll(__ballot(st == CHECK_VALUE_BYTES));
        if (st > 0 && first == CHECK_NONE) first = record_base + r;
    }
    for (int d = 32; d; d >>= 1) {
        const uint64_t o = __shfl_xor(first, d, 64);
        first = o < first ? o : first;
    }
    if (lane == 0) {
        if (ok) atomicAdd(out + CW_OK, (unsigned long long)ok);
        if (value_bytes) atomicAdd(out + CW_VALUE_BYTES, (unsigned long long)value_bytes);
        if (first != CHECK_NONE) atomicMin(out + CW_FIRST_BAD, (unsigned long long)first);
    }
}

}  // namespace bsdb
