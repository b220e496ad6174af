// merge_kernels.hip -- resident databases (get_kernels.hip) merged on gfx950:
// the records of a database that go on into a new kv.db image, read where
// they lie in the resident image.  k_db_records listed a side by slot
// (dump_kernels.hip), k_get_gather packed its keys, k_get_locate looked them
// up in the delta and in the removed database, and the selection is the
// diff's (k_diff_select_flags / scan / k_diff_select_scatter, mask 1 << KEPT):
//   k_merge_status  a record per lane: the slot's own status and locate's two
//                   answers into one merge status byte (merge_status_of,
//                   merge_plan.hpp); the counts go out with one atomic per
//                   wave and counter
//   k_rec_sizes     a record per lane: its bytes in the image and in the key
//                   blob (and, for the blocked layout, as a small record); the
//                   records, key bytes and value bytes written are counted here
//   (k_scan_*, and for the blocked layout k_blk_tile / chase / flags / place:
//    the text front end's placement works on sizes alone)
//   k_rec_pack      driven by the output, by the piece loop of piece_copy.hpp:
//                   the text pack's loop with a record writer, rec_put_record,
//                   whose source is a resident image through u64 positions
//   k_rec_pack_blocked   the same writer under k_text_pack_blocked's search in
//                   the two position lists
//   k_rec_outputs   a record per lane: its address (compact) and its value head
// The text pack (text_kernels.hip) reads one chunk of text through u32
// positions; an image has tens of GB.  What differs here: positions are u64
// at any alignment, and every position and length is data, not trusted: the
// lengths are cut by text_klen / text_vlen everywhere, so sizes, header and
// copied bytes always agree; a position at or past the image's end reads as 0,
// which also keeps pos + x from wrapping; and nothing is written outside
// [dst, dst + out_bytes) (the piece loop's).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "merge_plan.hpp"
#include "text_blocked_kernels.hip"  // text_klen / text_vlen, TextRuns, text_run_of, the placement kernels

namespace bsdb {

struct MergeStatusArgs {
    const uint8_t *status_base;     // [count] k_db_records' of the side that is listed
    const uint8_t *status_delta;    // [count] locate's of those records' keys in `delta`, or null: none is there
    const uint8_t *status_removed;  // [count] locate's in `removed`, or null
    uint8_t *status;                // [count] out: MergeStatus
    uint64_t count;
    uint32_t delta_side;            // 1: the side listed is `delta` itself (no lookups; its own words of the report)
    unsigned long long *out;        // the report (MW_WORDS), accumulated
};

// A record per lane; the loop is uniform per wave so the ballots see all lanes.
__global__ __launch_bounds__(256) void k_merge_status(MergeStatusArgs a) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    uint64_t seen = 0, kept = 0, replaced = 0, removed = 0, bad_slot = 0, bad_addr = 0;  // wave totals
    const bool lookups = !a.delta_side;
    for (uint64_t base = (uint64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); base < a.count; base += stride) {
        const uint64_t r = base + lane;
        int st = -1;
        if (r < a.count) {
            const uint8_t d = lookups && a.status_delta ? a.status_delta[r] : (uint8_t)GET_REJECTED;
            const uint8_t m = lookups && a.status_removed ? a.status_removed[r] : (uint8_t)GET_REJECTED;
            st = merge_status_of(a.status_base[r], d, m);
            a.status[r] = (uint8_t)st;
        }
        seen += __popcll(__ballot(st >= 0));
        kept += __popcll(__ballot(st == MERGE_KEPT));
        replaced += __popcll(__ballot(st == MERGE_REPLACED));
        removed += __popcll(__ballot(st == MERGE_REMOVED));
        bad_slot += __popcll(__ballot(st == MERGE_BAD_SLOT));
        bad_addr += __popcll(__ballot(st == MERGE_BAD_ADDR));
    }
    if (lane != 0) return;
    if (a.delta_side) {
        if (seen) atomicAdd(a.out + MW_DELTA_SLOTS, (unsigned long long)seen);
        if (kept) atomicAdd(a.out + MW_DELTA_WRITTEN, (unsigned long long)kept);
        if (bad_slot) atomicAdd(a.out + MW_DELTA_BAD_SLOT, (unsigned long long)bad_slot);
        return;
    }
    if (seen) atomicAdd(a.out + MW_BASE_SLOTS, (unsigned long long)seen);
    if (kept) atomicAdd(a.out + MW_KEPT, (unsigned long long)kept);
    if (replaced) atomicAdd(a.out + MW_REPLACED, (unsigned long long)replaced);
    if (removed) atomicAdd(a.out + MW_REMOVED, (unsigned long long)removed);
    if (bad_slot) atomicAdd(a.out + MW_BAD_SLOT, (unsigned long long)bad_slot);
    if (bad_addr) atomicAdd(a.out + MW_BAD_ADDR, (unsigned long long)bad_addr);
}

// record r's bytes in the image (header + key + value) and in the key blob;
// ssize (the blocked layout, else null): its bytes as a SMALL record of blocks
// of B bytes, 0 for a large one.  out (may be null): the records and their key
// and value bytes, as the image will hold them, added to the report.
__global__ __launch_bounds__(256) void k_rec_sizes(const uint32_t *klen, const uint32_t *vlen, uint64_t count, uint32_t B,
                                                   uint32_t *rsize, uint32_t *ksize, uint32_t *ssize, unsigned long long *out) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    uint64_t kbytes = 0, vbytes = 0, records = 0;  // this lane's
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < count; r += stride) {
        const uint32_t kl = text_klen(klen[r]), vl = text_vlen(vlen[r]), sz = 3 + kl + vl;
        rsize[r] = sz;
        ksize[r] = kl;
        if (ssize) ssize[r] = sz > B ? 0 : sz;
        kbytes += kl, vbytes += vl, ++records;
    }
    if (!out) return;  // (uniform)
    for (int d = 32; d; d >>= 1) {
        kbytes += __shfl_xor(kbytes, d, 64);
        vbytes += __shfl_xor(vbytes, d, 64);
        records += __shfl_xor(records, d, 64);
    }
    if (lane != 0 || !records) return;
    atomicAdd(out + MW_OUT_RECORDS, (unsigned long long)records);
    atomicAdd(out + MW_OUT_KEY_BYTES, (unsigned long long)kbytes);
    atomicAdd(out + MW_OUT_VALUE_BYTES, (unsigned long long)vbytes);
}

struct RecPack {
    const uint8_t *image;  // the resident image the records lie in (GetDb::image)
    uint64_t bytes;
    const uint64_t *ksrc, *vsrc;  // [count] byte position of key and value in the image (k_db_records', or a selection's)
    const uint32_t *klen, *vlen;  // [count] their lengths
    uint64_t count;       // records, >= 1
    const uint64_t *off;  // [count + 1] the scan of the records' sizes in this destination
    uint8_t *dst;         // out_bytes = off[count] bytes, at any alignment
    uint64_t out_bytes;
};

// Bytes [x0, x1) of record q, whose lengths are kl and vl, to the piece from
// byte jr.  IMAGE: the record is [kLen u8][vLen u16 BE][key][value]
// (SimpleCompactKVWriter.java:36-42); otherwise its key alone.  A source
// position at or past the image's end copies nothing (the bytes stay 0): below
// it, pos + x cannot wrap, and Piece::copy reads past the end as 0.
template <bool IMAGE>
__device__ __forceinline__ void rec_put_record(Piece &pc, const RecPack &a, uint64_t q, uint32_t kl, uint32_t vl, uint32_t x0,
                                               uint32_t x1, uint32_t jr) {
    const uint32_t hdr = IMAGE ? 3 : 0;
    if (IMAGE && x0 < 3) {
        const uint64_t h = (uint64_t)kl | (uint64_t)(vl >> 8) << 8 | (uint64_t)(vl & 0xFF) << 16;
        const uint32_t e = x1 < 3 ? x1 : 3;
        pc.put(h >> (8 * x0), jr, e - x0);
    }
    // the key's and the value's part of [x0, x1)
    for (int seg = 0; seg < (IMAGE ? 2 : 1); ++seg) {
        const uint32_t s0 = seg ? hdr + kl : hdr, s1 = seg ? hdr + kl + vl : hdr + kl;
        const uint32_t b = x0 > s0 ? x0 : s0, e = x1 < s1 ? x1 : s1;
        if (b >= e) continue;
        const uint64_t src = seg ? a.vsrc[q] : a.ksrc[q];
        if (src < a.bytes) pc.copy(a.image, a.bytes, src + (b - s0), jr + (b - x0), e - b);
    }
}

// The piece loop of piece_copy.hpp over the destination: a piece's owners are
// the records whose bytes overlap it, found in the scan of their sizes.
template <bool IMAGE>
__global__ __launch_bounds__(256) void k_rec_pack(RecPack a) {
    uint64_t qlo, qhi;
    piece_loop(
        a.dst, a.out_bytes, [&](uint64_t w0, uint64_t w1) { piece_wave_owners(a.off, a.count, w0, w1, qlo, qhi); },
        [&](Piece &pc) {
            piece_runs(pc, a.off, qlo, qhi, [&](uint64_t q, uint64_t rs, uint64_t o, uint64_t e) {
                rec_put_record<IMAGE>(pc, a, q, text_klen(a.klen[q]), text_vlen(a.vlen[q]), (uint32_t)(o - rs), (uint32_t)(e - rs),
                                      pc.j0 + (uint32_t)(o - pc.o0));
            });
        });
}

struct RecPackBlocked {
    RecPack t;           // off unused; dst / out_bytes: the chunk's blocked image
    const uint64_t *PS;  // [count + 1] k_blk_place's: a small record's first byte in the image
    const uint64_t *PL;  // [count + 1] a large record's
    uint32_t B;
};

// k_text_pack_blocked's search with rec_put_record: the owner of output byte o
// is the last small record with PS <= o if o lies within its bytes, else the
// last large record with PL <= o if o lies within its bytes, else nobody: the
// byte is 0 up to the next entry of either list.
__global__ __launch_bounds__(256) void k_rec_pack_blocked(RecPackBlocked b) {
    const RecPack &a = b.t;
    uint64_t slo, shi, llo, lhi;
    piece_loop(
        a.dst, a.out_bytes,
        [&](uint64_t w0, uint64_t w1) {
            piece_wave_owners(b.PS, a.count, w0, w1, slo, shi);
            piece_wave_owners(b.PL, a.count, w0, w1, llo, lhi);
        },
        [&](Piece &pc) {
            uint64_t hint = a.count;  // the record after the small one just written
            for (uint64_t o = pc.o0; o < pc.o1;) {
                uint64_t q = hint, rs = 0;
                uint32_t kl = 0, vl = 0, sz = 0;
                auto load = [&](const uint64_t *list) {
                    rs = list[q];
                    kl = text_klen(a.klen[q]), vl = text_vlen(a.vlen[q]), sz = 3 + kl + vl;
                };
                // record q, which starts at rs <= o, owns o: its bytes up to the piece's end
                auto emit = [&]() {
                    const uint64_t e = sz < pc.o1 - rs ? rs + sz : pc.o1;
                    rec_put_record<true>(pc, a, q, kl, vl, (uint32_t)(o - rs), (uint32_t)(e - rs), pc.j0 + (uint32_t)(o - pc.o0));
                    o = e;
                };
                if (q < a.count) load(b.PS);
                if (q >= a.count || rs != o || sz > b.B) {  // (a small record that starts at o is the last entry at or before o)
                    q = get_owner(b.PS, slo, shi, o);
                    load(b.PS);
                }
                hint = a.count;
                if (sz <= b.B && rs <= o && o - rs < sz) {
                    hint = q + 1;
                    emit();
                    continue;
                }
                uint64_t nearest = rs > o ? rs : b.PS[q + 1];  // the next list entry past o (PS[count] ends the image)
                q = get_owner(b.PL, llo, lhi, o);
                load(b.PL);
                if (sz > b.B && rs <= o && o - rs < sz) {
                    emit();
                    continue;
                }
                const uint64_t nl = rs > o ? rs : b.PL[q + 1];
                nearest = nl < nearest ? nl : nearest;
                o = nearest > o && nearest < pc.o1 ? nearest : pc.o1;  // zeros up to there
            }
        });
}

// The value head index.approximate stores, read from the image: the first
// l = min(vlen, 8) value bytes, the rest 0 (BSDBWriter.java:140-142).
__device__ __forceinline__ uint64_t rec_value_head(const uint8_t *image, uint64_t bytes, uint64_t vsrc, uint32_t vlen, uint32_t &l) {
    const uint32_t vl = text_vlen(vlen);
    l = vl < 8 ? vl : 8;
    return (vsrc < bytes ? sel_gload64(image, bytes, vsrc) : 0) & low_bytes_mask(l);
}

// A record per lane: addr = p << 56 | offset for the compact layout (the
// blocked addresses are k_blk_place's) and, for index.approximate, the value
// head and its length.
__global__ __launch_bounds__(256) void k_rec_outputs(TextRuns runs, const uint8_t *image, uint64_t bytes, const uint64_t *vsrc,
                                                     const uint32_t *vlen, const uint64_t *roff, uint64_t count, uint64_t *addr,
                                                     uint64_t *value8, uint8_t *value_len) {
    const uint64_t step = (uint64_t)gridDim.x * 256;
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < count; r += step) {
        if (addr) {
            const uint32_t p = text_run_of(runs, r);
            addr[r] = (uint64_t)p << 56 | (runs.file_base[p] + roff[r]);
        }
        if (value8) {
            uint32_t l;
            value8[r] = rec_value_head(image, bytes, vsrc[r], vlen[r], l);
            value_len[r] = (uint8_t)l;
        }
    }
}

}  // namespace bsdb
