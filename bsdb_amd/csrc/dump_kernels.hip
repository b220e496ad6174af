// dump_kernels.hip -- a resident database (get_kernels.hip) enumerated by slot
// on gfx950: index.db is n slots and every slot is the address of one record,
// so rank r of [first, first + count) is a record descriptor per lane with no
// hash, no MPHF lookup and no key to compare.
//   k_db_records    a slot per lane: the address decoded and bounds-tested, the
//                   header read (get_slot, the front of k_get_locate); writes
//                   where key and value lie in the image and how long they are
//   (k_scan_* + k_get_gather over klen / vlen give the packed keys and values)
//   k_dump_lengths  a record per lane: the length of its line "key<sep>value\n"
//                   (0 for a BAD_ADDR slot), and NOT_TEXT when its lengths alone
//                   stop the line from reading back (dump_length_status)
//   (k_scan_*)      llen -> loff[count + 1]
//   k_dump_text     the piece loop of piece_copy.hpp over the text, the inverse
//                   of k_text_pack<true>: a thread owns an aligned 16-byte piece
//                   of the output, finds the records it overlaps in loff and
//                   assembles key bytes, separator, value bytes and '\n'.  The
//                   key and value bytes it handles are tested for the separator,
//                   0x0A and 0x0D on the way: a find stores NOT_TEXT into that
//                   record's status (every finder stores the same byte)
//   k_dump_report   a record per lane: the final statuses counted, the bytes
//                   summed, the lowest slot that is not OK by atomicMin
// No lane walks a value: a 65 535-byte value is shared by 4 096 threads, a run
// of BAD_ADDR slots (length 0) is stepped over by the search.  index.db and
// every descriptor are data, not trusted: every read of the image goes through
// the bounded reader sel_gload64, offsets that are no scan end a piece
// (piece_runs), and nothing is written outside [text, text + text_bytes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dump_plan.hpp"
#include "get_kernels.hip"
#include "piece_copy.hpp"

namespace bsdb {

struct RecordsArgs {
    uint64_t first, count;   // slots [first, first + count) of db.index (the caller's: first + count <= n)
    uint64_t *ksrc, *vsrc;   // [count] byte position of key and value in the image
    uint32_t *klen, *vlen;   // [count] their lengths (u32: k_scan_* scans them)
    uint8_t *status;         // [count] DUMP_OK or DUMP_BAD_ADDR
    unsigned long long *out;  // the report (DW_WORDS), accumulated
};

// A slot per lane; the loop is uniform per wave so the ballots see all lanes.
__global__ __launch_bounds__(256) void k_db_records(GetDb db, RecordsArgs a) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    uint64_t seen = 0, ok = 0, bad_addr = 0;  // wave totals
    uint64_t kbytes = 0, vbytes = 0;          // this lane's
    uint64_t first_bad = DUMP_NONE;
    for (uint64_t base = (uint64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); base < a.count; base += stride) {
        const uint64_t i = base + lane;
        int st = -1;
        if (i < a.count) {
            const GetSlot rec = get_slot(db, __builtin_bswap64(db.index[a.first + i]));
            st = rec.ok ? DUMP_OK : DUMP_BAD_ADDR;
            a.ksrc[i] = rec.ok ? rec.p + 3 : 0;
            a.vsrc[i] = rec.ok ? rec.p + 3 + rec.kl : 0;
            a.klen[i] = rec.ok ? rec.kl : 0;
            a.vlen[i] = rec.ok ? rec.vb : 0;
            a.status[i] = (uint8_t)st;
            if (rec.ok) kbytes += rec.kl, vbytes += rec.vb;
            else if (first_bad == DUMP_NONE) first_bad = a.first + i;
        }
        seen += __popcll(__ballot(st >= 0));
        ok += __popcll(__ballot(st == DUMP_OK));
        bad_addr += __popcll(__ballot(st == DUMP_BAD_ADDR));
    }
    for (int d = 32; d; d >>= 1) {
        kbytes += __shfl_xor(kbytes, d, 64);
        vbytes += __shfl_xor(vbytes, d, 64);
        const uint64_t o = __shfl_xor(first_bad, d, 64);
        first_bad = o < first_bad ? o : first_bad;
    }
    if (lane == 0) {
        if (seen) atomicAdd(a.out + DW_SLOTS, (unsigned long long)seen);
        if (ok) atomicAdd(a.out + DW_OK, (unsigned long long)ok);
        if (bad_addr) atomicAdd(a.out + DW_BAD_ADDR, (unsigned long long)bad_addr);
        if (kbytes) atomicAdd(a.out + DW_KEY_BYTES, (unsigned long long)kbytes);
        if (vbytes) atomicAdd(a.out + DW_VALUE_BYTES, (unsigned long long)vbytes);
        if (first_bad != DUMP_NONE) atomicMin(a.out + DW_FIRST_BAD, (unsigned long long)first_bad);
    }
}

struct DumpArgs {
    const uint8_t *image;  // the database's (GetDb::image)
    uint64_t image_bytes;
    const uint64_t *ksrc, *vsrc;  // [count] k_db_records'
    const uint32_t *klen, *vlen;
    uint8_t *status;       // [count] in: k_db_records', out: with NOT_TEXT
    uint64_t count;
    uint32_t *llen;        // [count] line lengths
    const uint64_t *loff;  // [count + 1] their scan
    uint32_t sep;          // the separator byte
    uint8_t *text;         // the output, text_bytes = loff[count] long, at any alignment
    uint64_t text_bytes;
    uint64_t first;        // the slot of record 0 (first_bad is a slot)
    unsigned long long *out;  // the report (DW_WORDS), accumulated
};

__global__ __launch_bounds__(256) void k_dump_lengths(DumpArgs a) {
    const uint64_t step = (uint64_t)gridDim.x * 256;
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < a.count; r += step) {
        const int st = dump_status_in(a.status[r]) == DUMP_BAD_ADDR ? (int)DUMP_BAD_ADDR : (int)DUMP_OK;
        a.llen[r] = dump_line_len(st, a.klen[r], a.vlen[r]);
        a.status[r] = (uint8_t)dump_length_status(st, a.klen[r], a.vlen[r]);
    }
}

// 0x80 in every byte of x that equals the byte repeated in `pattern`, exact
// per byte (no carry crosses a byte)
__device__ __forceinline__ uint64_t dump_bytes_equal(uint64_t x, uint64_t pattern) {
    const uint64_t y = x ^ pattern, m = 0x7F7F7F7F7F7F7F7Full;
    return ~(((y & m) + m) | y | m);
}

// 0xFF in bytes [b, e) of a register, b <= e <= 8
__device__ __forceinline__ uint64_t dump_byte_range(uint32_t b, uint32_t e) { return low_bytes_mask(e) & ~low_bytes_mask(b); }

// Bytes [x0, x1) of record q's line, whose lengths are kl and vl, to the piece
// from byte jr; `lo` / `hi` collect the piece bytes that came from the image.
__device__ __forceinline__ void dump_put_line(Piece &pc, const DumpArgs &a, uint64_t q, uint32_t kl, uint32_t vl, uint32_t x0,
                                              uint32_t x1, uint32_t jr, uint64_t &lo, uint64_t &hi) {
    // the key's and the value's part of [x0, x1)
    for (int seg = 0; seg < 2; ++seg) {
        const uint32_t s0 = seg ? kl + 1 : 0, s1 = seg ? kl + 1 + vl : kl;
        const uint64_t src = seg ? a.vsrc[q] : a.ksrc[q];
        const uint32_t b = x0 > s0 ? x0 : s0, e = x1 < s1 ? x1 : s1;
        if (b < e) {
            const uint32_t j = jr + (b - x0), je = j + (e - b);  // piece bytes [j, je), je <= 16
            pc.copy(a.image, a.image_bytes, src + (b - s0), j, e - b);
            lo |= dump_byte_range(j < 8 ? j : 8, je < 8 ? je : 8);
            hi |= dump_byte_range(j > 8 ? j - 8 : 0, je > 8 ? je - 8 : 0);
        }
    }
    if (x0 <= kl && kl < x1) pc.put(a.sep, jr + (kl - x0), 1);
    const uint32_t t = kl + 1 + vl;  // the terminator
    if (x0 <= t && t < x1) pc.put('\n', jr + (t - x0), 1);
}

// The piece loop of piece_copy.hpp over the text: a piece's owners are the
// records whose lines overlap it, found in the scan of their lengths.  The
// text test reads no byte twice: it looks at the assembled registers, under
// the mask of the bytes this record's key and value gave.
__global__ __launch_bounds__(256) void k_dump_text(DumpArgs a) {
    uint64_t qlo, qhi;
    const uint64_t ones = 0x0101010101010101ull;
    piece_loop(
        a.text, a.text_bytes, [&](uint64_t w0, uint64_t w1) { piece_wave_owners(a.loff, a.count, w0, w1, qlo, qhi); },
        [&](Piece &pc) {
            piece_runs(pc, a.loff, qlo, qhi, [&](uint64_t q, uint64_t rs, uint64_t o, uint64_t e) {
                uint64_t mlo = 0, mhi = 0;
                dump_put_line(pc, a, q, dump_klen(a.klen[q]), dump_vlen(a.vlen[q]), (uint32_t)(o - rs), (uint32_t)(e - rs),
                              pc.j0 + (uint32_t)(o - pc.o0), mlo, mhi);
                auto found = [&](uint64_t c) { return (dump_bytes_equal(pc.lo, c * ones) & mlo) | (dump_bytes_equal(pc.hi, c * ones) & mhi); };
                if (found(a.sep) | found('\n') | found('\r')) a.status[q] = (uint8_t)DUMP_NOT_TEXT;
            });
        });
}

// The final statuses counted, the bytes of the records that have any summed,
// and the lowest slot that is not OK.
__global__ __launch_bounds__(256) void k_dump_report(DumpArgs a) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    uint64_t seen = 0, ok = 0, bad_addr = 0, not_text = 0;  // wave totals
    uint64_t kbytes = 0, vbytes = 0, tbytes = 0;            // this lane's
    uint64_t first_bad = DUMP_NONE;
    for (uint64_t base = (uint64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); base < a.count; base += stride) {
        const uint64_t r = base + lane;
        int st = -1;
        if (r < a.count) {
            st = dump_status_in(a.status[r]);
            if (st != DUMP_BAD_ADDR) kbytes += dump_klen(a.klen[r]), vbytes += dump_vlen(a.vlen[r]);
            tbytes += a.llen[r];
            if (st != DUMP_OK && first_bad == DUMP_NONE) first_bad = a.first + r;
        }
        seen += __popcll(__ballot(st >= 0));
        ok += __popcll(__ballot(st == DUMP_OK));
        bad_addr += __popcll(__ballot(st == DUMP_BAD_ADDR));
        not_text += __popcll(__ballot(st == DUMP_NOT_TEXT));
    }
    for (int d = 32; d; d >>= 1) {
        kbytes += __shfl_xor(kbytes, d, 64);
        vbytes += __shfl_xor(vbytes, d, 64);
        tbytes += __shfl_xor(tbytes, d, 64);
        const uint64_t o = __shfl_xor(first_bad, d, 64);
        first_bad = o < first_bad ? o : first_bad;
    }
    if (lane == 0) {
        if (seen) atomicAdd(a.out + DW_SLOTS, (unsigned long long)seen);
        if (ok) atomicAdd(a.out + DW_OK, (unsigned long long)ok);
        if (bad_addr) atomicAdd(a.out + DW_BAD_ADDR, (unsigned long long)bad_addr);
        if (not_text) atomicAdd(a.out + DW_NOT_TEXT, (unsigned long long)not_text);
        if (kbytes) atomicAdd(a.out + DW_KEY_BYTES, (unsigned long long)kbytes);
        if (vbytes) atomicAdd(a.out + DW_VALUE_BYTES, (unsigned long long)vbytes);
        if (tbytes) atomicAdd(a.out + DW_TEXT_BYTES, (unsigned long long)tbytes);
        if (first_bad != DUMP_NONE) atomicMin(a.out + DW_FIRST_BAD, (unsigned long long)first_bad);
    }
}

}  // namespace bsdb
