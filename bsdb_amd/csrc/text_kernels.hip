// text_kernels.hip -- the text front end on gfx950: "key<sep>value" lines of
// one chunk of text resident in HBM (< 2^32 bytes) into record descriptors,
// and the kept records into the compact kv.db layout.  What Builder's put
// loop does one line per call on one thread per file
// (tools/Builder.java:144-176: BufferedReader.lines, String.split(sep), put;
// write/kv/SimpleCompactKVWriter.java:36-42 for the record layout), as
//   k_text_count      per 16-byte piece: which bytes start a line, which are
//                     separators; per-workgroup counts of both
//   k_text_positions  the same classification again, scattered into two sorted
//                     u32 position lists (offsets: k_scan_* over the counts)
//   k_text_records    a line per lane: its end from the next line start, its
//                     separators by two searches in the separator list, the
//                     verdict by arithmetic (text_verdict, text_plan.hpp);
//                     pass 0 counts and flags, pass 1 (after the scan of the
//                     flags) writes the kept lines' descriptors in input order
//   k_text_sizes      a record per lane: its bytes in the image and in the blob
//                     (and, for the blocked layout, as a small record)
//   k_text_pack       driven by the output, by the piece loop k_get_gather
//                     runs (piece_copy.hpp): the owners of a 16-byte piece of
//                     the destination are found in the size scan; what the
//                     kernel adds is the record writer, text_put_record
//   k_text_outputs    a record per lane: its address and its value head
// No lane walks a line: a 32 KB value or a 1 MB junk line costs what a
// 20-byte line costs.  Every read of the text in the pack goes through the
// bounded reader sel_gload64 with the chunk as its limit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "piece_copy.hpp"
#include "text_plan.hpp"

namespace bsdb {

// The 16-byte piece k of the text: bit j of `starts` = byte 16 k + j starts a
// line (it is byte 0, or follows a '\n', or follows a '\r' and is no '\n'),
// bit j of `seps` = it is the separator.  Bytes past the text are neither.
__device__ __forceinline__ void text_classify(const uint8_t *text, uint64_t bytes, uint64_t k, uint32_t sep, uint32_t &starts,
                                              uint32_t &seps) {
    starts = seps = 0;
    const uint64_t p0 = k * 16;
    if (p0 >= bytes) return;
    uint32_t w[4];
    if (p0 + 16 <= bytes) {
        const uint4 v = *reinterpret_cast<const uint4 *>(text + p0);  // (the text is 16-byte aligned)
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
    } else {
        w[0] = w[1] = w[2] = w[3] = 0;
        for (uint32_t j = 0; p0 + j < bytes; ++j) w[j >> 2] |= (uint32_t)text[p0 + j] << (8 * (j & 3));
    }
    const uint32_t nvalid = bytes - p0 < 16 ? (uint32_t)(bytes - p0) : 16;
    uint32_t prev = p0 ? text[p0 - 1] : '\n';  // (byte 0 starts a line)
#pragma unroll
    for (uint32_t j = 0; j < 16; ++j) {
        const uint32_t b = (w[j >> 2] >> (8 * (j & 3))) & 0xFF;
        const bool valid = j < nvalid;
        if (valid && (prev == '\n' || (prev == '\r' && b != '\n'))) starts |= 1u << j;
        if (valid && b == sep) seps |= 1u << j;
        prev = b;
    }
}

// exclusive scan of one u32 per thread over a 256-thread workgroup
__device__ __forceinline__ uint32_t text_block_scan(uint32_t v, uint32_t *wsum, uint32_t &total) {
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    uint32_t x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d, 64);
        if (lane >= (uint32_t)d) x += y;
    }
    if (lane == 63) wsum[wid] = x;
    __syncthreads();
    uint32_t pre = 0, tot = 0;
    for (uint32_t w = 0; w < 4; ++w) {
        const uint32_t s = wsum[w];
        pre += w < wid ? s : 0;
        tot += s;
    }
    total = tot;
    __syncthreads();
    return pre + x - v;
}

// Workgroup g classifies text bytes [4096 g, 4096 g + 4096).
__global__ __launch_bounds__(256) void k_text_count(const uint8_t *text, uint64_t bytes, uint32_t sep, uint32_t *cnt_starts,
                                                    uint32_t *cnt_seps) {
    __shared__ uint32_t wsum[4];
    uint32_t st, sp, tot_st, tot_sp;
    text_classify(text, bytes, (uint64_t)blockIdx.x * 256 + threadIdx.x, sep, st, sp);
    text_block_scan(__popc(st), wsum, tot_st);
    text_block_scan(__popc(sp), wsum, tot_sp);
    if (threadIdx.x == 0) {
        cnt_starts[blockIdx.x] = tot_st;
        cnt_seps[blockIdx.x] = tot_sp;
    }
}

// off_*: the exclusive scans of k_text_count's counts (off[blocks] = totals);
// ls / sp receive the positions in increasing order.
__global__ __launch_bounds__(256) void k_text_positions(const uint8_t *text, uint64_t bytes, uint32_t sep,
                                                        const uint64_t *off_starts, const uint64_t *off_seps, uint32_t *ls,
                                                        uint64_t ls_cap, uint32_t *sp, uint64_t sp_cap) {
    __shared__ uint32_t wsum[4];
    uint32_t st, se, tot;
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    text_classify(text, bytes, k, sep, st, se);
    uint64_t at = off_starts[blockIdx.x] + text_block_scan(__popc(st), wsum, tot);
    for (uint32_t m = st; m; m &= m - 1, ++at)
        if (at < ls_cap) ls[at] = (uint32_t)(k * 16) + (uint32_t)__builtin_ctz(m);
    at = off_seps[blockIdx.x] + text_block_scan(__popc(se), wsum, tot);
    for (uint32_t m = se; m; m &= m - 1, ++at)
        if (at < sp_cap) sp[at] = (uint32_t)(k * 16) + (uint32_t)__builtin_ctz(m);
}

// the first index in [0, n) with list[index] >= x (n when there is none)
__device__ __forceinline__ uint64_t text_lower_bound(const uint32_t *list, uint64_t n, uint32_t x) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (list[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

struct TextSplit {
    const uint8_t *text;
    uint64_t bytes;            // < 2^32
    const uint32_t *ls;        // line starts, `lines` of them
    uint64_t lines;
    const uint32_t *sp;        // separator positions, `seps` of them
    uint64_t seps;
    uint32_t *keep;            // [lines] pass 0: 1 for a kept line
    const uint64_t *keep_off;  // [lines + 1] pass 1: the scan of keep
    uint32_t *kpos, *klen, *vpos, *vlen;  // pass 1: the kept lines' descriptors
    uint64_t cap;              // descriptors the caller's arrays hold
    unsigned long long *out;   // pass 0: the report (TW_WORDS), accumulated
};

// The verdict on line j.  Its end is the next line's start (the text's end
// for the last line) minus its terminator: "\n", "\r" or "\r\n"; only the
// last line of a text can have none.
__device__ __forceinline__ TextLine text_line(const TextSplit &a, uint64_t j) {
    const uint32_t start = a.ls[j];
    const uint32_t next = j + 1 < a.lines ? a.ls[j + 1] : (uint32_t)a.bytes;  // > start
    const uint32_t last = a.text[next - 1];
    uint32_t end = next;
    if (last == '\n') end = next - 1 > start && a.text[next - 2] == '\r' ? next - 2 : next - 1;
    else if (last == '\r') end = next - 1;
    const uint64_t lo = text_lower_bound(a.sp, a.seps, start), hi = lo + text_lower_bound(a.sp + lo, a.seps - lo, end);
    const uint32_t c = (uint32_t)(hi - lo);
    return text_verdict(start, end, c, c >= 1 ? a.sp[lo] : 0, c >= 2 ? a.sp[lo + 1] : 0);
}

// A line per lane; the loop is uniform per wave so the ballots see all lanes.
template <bool EMIT>
__global__ __launch_bounds__(256) void k_text_records(TextSplit a) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    uint64_t lines = 0, kept = 0, not_two = 0, empty_key = 0, too_large = 0;  // wave totals
    uint64_t kbytes = 0, vbytes = 0;                                          // this lane's
    uint32_t kmax = 0, vmax = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); base < a.lines; base += stride) {
        const uint64_t j = base + lane;
        const bool active = j < a.lines;
        int v = -1;
        if (active) {
            const TextLine t = text_line(a, j);
            v = (int)t.verdict;
            if (EMIT) {
                const uint64_t r = a.keep_off[j];
                if (v == TV_KEPT && r < a.cap) {
                    a.kpos[r] = t.kpos;
                    a.klen[r] = t.klen;
                    a.vpos[r] = t.vpos;
                    a.vlen[r] = t.vlen;
                }
            } else {
                a.keep[j] = v == TV_KEPT;
                if (v == TV_KEPT) {
                    kbytes += t.klen;
                    vbytes += t.vlen;
                    kmax = t.klen > kmax ? t.klen : kmax;
                    vmax = t.vlen > vmax ? t.vlen : vmax;
                }
            }
        }
        if (!EMIT) {
            lines += __popcll(__ballot(active));
            kept += __popcll(__ballot(v == TV_KEPT));
            not_two += __popcll(__ballot(v == TV_NOT_TWO_FIELDS));
            empty_key += __popcll(__ballot(v == TV_EMPTY_KEY));
            too_large += __popcll(__ballot(v == TV_TOO_LARGE));
        }
    }
    if (EMIT) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(a.out + TW_CHUNKS, 1ull);
    for (int d = 32; d; d >>= 1) {
        kbytes += __shfl_xor(kbytes, d, 64);
        vbytes += __shfl_xor(vbytes, d, 64);
        const uint32_t ko = __shfl_xor(kmax, d, 64), vo = __shfl_xor(vmax, d, 64);
        kmax = ko > kmax ? ko : kmax;
        vmax = vo > vmax ? vo : vmax;
    }
    if (lane == 0) {
        if (lines) atomicAdd(a.out + TW_LINES, (unsigned long long)lines);
        if (kept) atomicAdd(a.out + TW_RECORDS, (unsigned long long)kept);
        if (not_two) atomicAdd(a.out + TW_NOT_TWO_FIELDS, (unsigned long long)not_two);
        if (empty_key) atomicAdd(a.out + TW_EMPTY_KEY, (unsigned long long)empty_key);
        if (too_large) atomicAdd(a.out + TW_TOO_LARGE, (unsigned long long)too_large);
        if (kbytes) atomicAdd(a.out + TW_KEY_BYTES, (unsigned long long)kbytes);
        if (vbytes) atomicAdd(a.out + TW_VALUE_BYTES, (unsigned long long)vbytes);
        if (kmax) atomicMax(a.out + TW_MAX_KEY_LEN, (unsigned long long)kmax);
        if (vmax) atomicMax(a.out + TW_MAX_VALUE_LEN, (unsigned long long)vmax);
    }
}

// The lengths the pack works with: a descriptor's, cut to what a record can
// hold, so that the sizes, the header and the copied bytes always agree.
__device__ __forceinline__ uint32_t text_klen(uint32_t klen) { return klen < TEXT_MAX_KEY ? klen : TEXT_MAX_KEY; }
__device__ __forceinline__ uint32_t text_vlen(uint32_t vlen) { return vlen < TEXT_MAX_VALUE ? vlen : TEXT_MAX_VALUE; }

// record r's bytes in the image (header + key + value) and in the key blob;
// ssize (the blocked layout, else null): its bytes as a SMALL record of blocks
// of B bytes, 0 for a large one
__global__ __launch_bounds__(256) void k_text_sizes(const uint32_t *klen, const uint32_t *vlen, uint64_t count, uint32_t B,
                                                    uint32_t *rsize, uint32_t *ksize, uint32_t *ssize) {
    const uint64_t step = (uint64_t)gridDim.x * 256;
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < count; r += step) {
        const uint32_t kl = text_klen(klen[r]), sz = 3 + kl + text_vlen(vlen[r]);
        rsize[r] = sz;
        ksize[r] = kl;
        if (ssize) ssize[r] = sz > B ? 0 : sz;
    }
}

struct TextPack {
    const uint8_t *text;
    uint64_t bytes;
    const uint32_t *kpos, *klen, *vpos, *vlen;
    uint64_t count;       // records, >= 1
    const uint64_t *off;  // [count + 1] the scan of the records' sizes in this destination
    uint8_t *dst;         // out_bytes = off[count] bytes, at any alignment
    uint64_t out_bytes;
};

// Bytes [x0, x1) of record q, whose lengths are kl and vl, to the piece from
// byte jr.  IMAGE: the record is [kLen u8][vLen u16 BE][key][value]
// (SimpleCompactKVWriter.java:36-42); otherwise its key alone (the blob the
// hash kernels read).
template <bool IMAGE>
__device__ __forceinline__ void text_put_record(Piece &pc, const TextPack &a, uint64_t q, uint32_t kl, uint32_t vl, uint32_t x0,
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
        const uint64_t src = seg ? a.vpos[q] : a.kpos[q];
        const uint32_t b = x0 > s0 ? x0 : s0, e = x1 < s1 ? x1 : s1;
        if (b < e) pc.copy(a.text, a.bytes, src + (b - s0), jr + (b - x0), e - b);
    }
}

// The piece loop of piece_copy.hpp over the destination: a piece's owners are
// the records whose bytes overlap it, found in the scan of their sizes.
template <bool IMAGE>
__global__ __launch_bounds__(256) void k_text_pack(TextPack a) {
    uint64_t qlo, qhi;
    piece_loop(
        a.dst, a.out_bytes, [&](uint64_t w0, uint64_t w1) { piece_wave_owners(a.off, a.count, w0, w1, qlo, qhi); },
        [&](Piece &pc) {
            piece_runs(pc, a.off, qlo, qhi, [&](uint64_t q, uint64_t rs, uint64_t o, uint64_t e) {
                text_put_record<IMAGE>(pc, a, q, text_klen(a.klen[q]), text_vlen(a.vlen[q]), (uint32_t)(o - rs), (uint32_t)(e - rs),
                                       pc.j0 + (uint32_t)(o - pc.o0));
            });
        });
}

// The runs of the partition rule (text_run_bound) and where each lands:
// record r of run p lies at file offset file_base[p] + roff[r], file_base[p] =
// the file's size before the chunk minus roff of the run's first record.
struct TextRuns {
    uint32_t partitions;
    uint64_t bound[TEXT_MAX_PARTS + 1];
    uint64_t file_base[TEXT_MAX_PARTS];
};

// the run of record i: the last p with bound[p] <= i (empty runs share their bound)
__device__ __forceinline__ uint32_t text_run_of(const TextRuns &runs, uint64_t i) {
    uint32_t lo = 0, hi = runs.partitions - 1;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (runs.bound[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// The value head index.approximate stores for a value of `vlen` bytes at
// `vpos` of the text: its first l = min(vlen, 8) bytes, the rest 0
// (BSDBWriter.java:140-142).  k_text_outputs writes it, the check of a database
// against its text (check_kernels.hip) compares the slot with it.
__device__ __forceinline__ uint64_t text_value_head(const uint8_t *text, uint64_t bytes, uint64_t vpos, uint32_t vlen, uint32_t &l) {
    const uint32_t vl = text_vlen(vlen);
    l = vl < 8 ? vl : 8;
    return (vpos < bytes ? sel_gload64(text, bytes, vpos) : 0) & low_bytes_mask(l);
}

// A record per lane: addr = p << 56 | offset (SimpleCompactKVWriter.java:62-73,
// PartitionedKVWriter.java:82-96) and, for index.approximate, the value head:
// the first min(vlen, 8) value bytes, the rest 0, and that length
// (BSDBWriter.java:140-142).
__global__ __launch_bounds__(256) void k_text_outputs(TextRuns runs, const uint8_t *text, uint64_t bytes, const uint32_t *vpos,
                                                      const uint32_t *vlen, const uint64_t *roff, uint64_t count,
                                                      uint64_t *addr, uint64_t *value8, uint8_t *value_len) {
    const uint64_t step = (uint64_t)gridDim.x * 256;
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < count; r += step) {
        if (addr) {
            const uint32_t p = text_run_of(runs, r);
            addr[r] = (uint64_t)p << 56 | (runs.file_base[p] + roff[r]);
        }
        if (value8) {
            uint32_t l;
            value8[r] = text_value_head(text, bytes, vpos[r], vlen[r], l);
            value_len[r] = (uint8_t)l;
        }
    }
}

}  // namespace bsdb
