// text_blocked_kernels.hip -- the blocked kv.db layout of the text front end
// on gfx950 (BlockedKVWriter.java:45-74; the rule: text_place_blocked,
// text_plan.hpp).  A record's place depends on a greedy recurrence (a record
// that does not fit the rest of its block opens a new one); it is placed
// without a lane walking a run:
//   k_text_sizes  (text_kernels.hip, with ssize) a record per lane: its size,
//                 its key bytes, and its size as a SMALL record (0 for a
//                 large one); S = the scan of the last
//   k_blk_tile    a workgroup per TEXT_TILE records, S's slice in LDS:
//                 next[a] = the first record that does not fit a block opened
//                 at a, capped at the run's end (a binary search, in LDS
//                 unless the block passes the tile's end); then by pointer
//                 doubling in LDS last[a] = the last block start of the tile
//                 reached from a, exit[a] = next[last[a]]
//   k_blk_chase   a lane per run follows exit from the run's first record,
//                 one hop per tile, and leaves per tile its ENTRY (the first
//                 block start at or past the tile's first record) and its
//                 CARRY (the block start before that)
//   k_blk_flags   a workgroup per tile: one lane walks next in LDS from the
//                 entry and flags the block starts; a max-scan gives every
//                 record its block's start, hence its offset in the block and
//                 the record that closes the block; the EVENT of record i is
//                 the bytes the file grows by when i arrives: a large
//                 record's own block, or B for the block a new start closes
//   (scan)        E = the scan of the events: file positions
//   k_blk_place   a record per lane: its address and its position in the image
//                 as a small record (PS) and as a large one (PL); both lists
//                 are sorted, a record of the other kind is an empty interval
//   k_text_pack_blocked   driven by the output, by the piece loop of
//                 piece_copy.hpp and k_text_pack's record writer: a piece's
//                 records are found in PS and PL; bytes of no record are zeros
// The chain of block starts runs through the whole chunk: next is capped at
// the run's end, so every run's first record is a block start (a large first
// record stands for the first small one after it: it adds nothing to S).
// Every index read back from device memory is clamped before it is used.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "text_kernels.hip"

namespace bsdb {

// Workgroup t: records [t TEXT_TILE, ...).  S[count + 1]; next[count]; exl[count] = (last, exit).
__global__ __launch_bounds__(256) void k_blk_tile(TextRuns runs, const uint64_t *S, uint64_t count, uint32_t B, uint32_t *next,
                                                  uint2 *exl) {
    __shared__ uint32_t sl[TEXT_TILE + 1], nx[TEXT_TILE], pa[TEXT_TILE], pb[TEXT_TILE];
    const uint64_t ts = (uint64_t)blockIdx.x * TEXT_TILE;
    const uint64_t te = ts + TEXT_TILE < count ? ts + TEXT_TILE : count;
    const uint32_t n = (uint32_t)(te - ts);
    const uint64_t S0 = S[ts];
    for (uint32_t j = threadIdx.x; j <= n; j += 256) sl[j] = (uint32_t)(S[ts + j] - S0);  // <= 2048 x 65 536
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < n; j += 256) {
        const uint64_t a = ts + j;
        uint64_t re = runs.bound[text_run_of(runs, a) + 1];
        re = re > count ? count : re;
        re = re > a ? re : a + 1;
        const uint32_t target = sl[j] + B;
        const uint64_t lim = re < te ? re : te;
        // the first m in (a, lim] with S[m] > S[a] + B; a block opened at a ends before record m - 1
        uint32_t lo = j + 1, hi = (uint32_t)(lim - ts) + 1;
        const uint32_t none = hi;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (sl[mid] > target) hi = mid;
            else lo = mid + 1;
        }
        uint64_t nxt;
        if (lo < none) {
            nxt = ts + lo - 1;
        } else if (lim == re) {
            nxt = re;
        } else {  // the block passes the tile's end: the same search in (te, re] of the whole scan
            const uint64_t t64 = S0 + target;
            uint64_t l = te + 1, h = re + 1;
            while (l < h) {
                const uint64_t mid = l + (h - l) / 2;
                if (S[mid] > t64) h = mid;
                else l = mid + 1;
            }
            nxt = l - 1;
        }
        nxt = nxt > a ? nxt : a + 1;
        nxt = nxt < re ? nxt : re;
        nx[j] = (uint32_t)nxt;
        pa[j] = nxt < te ? (uint32_t)(nxt - ts) : j;  // (a start whose next leaves the tile points at itself)
    }
    __syncthreads();
    uint32_t *from = pa, *to = pb;
    for (uint32_t round = 0; (1u << round) < TEXT_TILE; ++round) {
        for (uint32_t j = threadIdx.x; j < n; j += 256) to[j] = from[from[j]];
        __syncthreads();
        uint32_t *const sw = from;
        from = to;
        to = sw;
    }
    for (uint32_t j = threadIdx.x; j < n; j += 256) {
        const uint32_t l = from[j];
        next[ts + j] = nx[j];
        exl[ts + j] = make_uint2((uint32_t)ts + l, nx[l]);
    }
}

// Workgroup p, lane 0: run p's chain, a hop per tile.  entry / carry [tiles].
__global__ __launch_bounds__(64) void k_blk_chase(TextRuns runs, const uint2 *exl, uint64_t count, uint32_t tiles, uint32_t *entry,
                                                 uint32_t *carry) {
    if (threadIdx.x) return;
    const uint32_t p = blockIdx.x;
    uint64_t a = runs.bound[p], end = runs.bound[p + 1];
    end = end > count ? count : end;
    if (a >= end) return;
    if (a % TEXT_TILE == 0) entry[a / TEXT_TILE] = (uint32_t)a;
    uint64_t done = a / TEXT_TILE;  // tiles up to this one have their entry
    for (uint32_t hops = 0; a < end && hops <= tiles; ++hops) {
        const uint2 le = exl[a];
        uint64_t x = le.y;
        x = x > a ? x : a + 1;
        x = x < end ? x : end;
        const uint64_t tx = x / TEXT_TILE < tiles ? x / TEXT_TILE : tiles - 1;  // (x = count may lie past the last tile)
        for (uint64_t t = done + 1; t <= tx; ++t) {
            entry[t] = (uint32_t)x;
            carry[t] = le.x;
        }
        done = tx > done ? tx : done;
        a = x;
    }
}

// inclusive max-scan of one int per thread over a 256-thread workgroup, as an exclusive prefix
__device__ __forceinline__ int text_block_max_before(int v, int *wmax) {
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d, 64);
        if (lane >= (uint32_t)d) x = y > x ? y : x;
    }
    if (lane == 63) wmax[wid] = x;
    __syncthreads();
    int before = __shfl_up(x, 1, 64);
    if (lane == 0) before = -1;
    for (uint32_t w = 0; w < 4; ++w) {
        const int s = wmax[w];
        if (w < wid) before = s > before ? s : before;
    }
    return before;
}

// Workgroup t.  ev / boff / bend [count]: record i's event, its offset in its
// block (the small bytes of its block before it), the record that closes it.
__global__ __launch_bounds__(256) void k_blk_flags(TextRuns runs, const uint64_t *S, const uint32_t *rsize, const uint32_t *next,
                                                   const uint32_t *entry, const uint32_t *carry, uint64_t count, uint32_t B,
                                                   uint32_t *ev, uint32_t *boff, uint32_t *bend) {
    __shared__ uint32_t sl[TEXT_TILE + 1], nx[TEXT_TILE];
    __shared__ uint8_t fl[TEXT_TILE];
    __shared__ int wmax[4];
    const uint64_t ts = (uint64_t)blockIdx.x * TEXT_TILE;
    const uint64_t te = ts + TEXT_TILE < count ? ts + TEXT_TILE : count;
    const uint32_t n = (uint32_t)(te - ts);
    const uint64_t S0 = S[ts];
    for (uint32_t j = threadIdx.x; j <= n; j += 256) sl[j] = (uint32_t)(S[ts + j] - S0);
    for (uint32_t j = threadIdx.x; j < TEXT_TILE; j += 256) {
        nx[j] = j < n ? next[ts + j] : 0;
        fl[j] = 0;
    }
    uint64_t e0 = blockIdx.x ? entry[blockIdx.x] : 0;
    e0 = e0 < ts ? ts : e0 > count ? count : e0;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t a = e0;
        for (uint32_t steps = 0; a < te && steps < TEXT_TILE; ++steps) {
            fl[a - ts] = 1;
            const uint64_t nn = nx[a - ts];
            a = nn > a ? nn : a + 1;
        }
    }
    __syncthreads();
    // thread k holds records 8 k .. 8 k + 7: the last flagged record at or before each
    const uint32_t j0 = threadIdx.x * 8;
    int own = -1;
    for (uint32_t j = j0; j < j0 + 8; ++j)
        if (j < n && fl[j]) own = (int)j;
    int b = text_block_max_before(own, wmax);
    uint64_t Sc = 0;
    bool have_c = false;
    for (uint32_t j = j0; j < j0 + 8 && j < n; ++j) {
        if (fl[j]) b = (int)j;
        const uint64_t a = ts + j;
        uint64_t off, be;
        if (b >= 0) {
            off = sl[j] - sl[b];
            be = nx[b];
        } else {  // its block started in an earlier tile
            if (!have_c) {
                uint64_t c = blockIdx.x ? carry[blockIdx.x] : 0;
                c = c < ts ? c : (ts ? ts - 1 : 0);
                Sc = S[c];
                have_c = true;
            }
            off = S0 + sl[j] - Sc;
            be = e0;
        }
        const uint32_t rs = rsize[a];
        const bool start_of_run = runs.bound[text_run_of(runs, a)] == a;
        ev[a] = rs > B ? text_large_block(rs) : (fl[j] && !start_of_run ? B : 0);
        boff[a] = (uint32_t)(off < B ? off : B);
        bend[a] = (uint32_t)(be > a ? (be < count ? be : count) : a + 1);
    }
}

struct TextBlockedRuns {
    uint64_t image_base[TEXT_MAX_PARTS];  // where run p starts in the chunk's image
    uint64_t file_size[TEXT_MAX_PARTS];   // kv.db.<p>'s bytes before the chunk
};

// A record per lane (and i = count: the lists' sentinels).  addr = p << 56 |
// block pages << 48 | block page in the file << 16 | offset.
__global__ __launch_bounds__(256) void k_blk_place(TextRuns runs, TextBlockedRuns br, const uint64_t *E, const uint32_t *rsize,
                                                   const uint32_t *boff, const uint32_t *bend, uint64_t count, uint32_t B,
                                                   uint64_t image_bytes, uint64_t *PS, uint64_t *PL, uint64_t *addr) {
    const uint64_t step = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i <= count; i += step) {
        if (i == count) {
            PS[i] = PL[i] = image_bytes;
            continue;
        }
        const uint32_t p = text_run_of(runs, i);
        const uint64_t Ers = E[runs.bound[p]];
        uint64_t be = bend[i];
        be = be < count ? be : count;
        const uint64_t small_at = E[be] - Ers, large_at = E[i] - Ers;
        const uint32_t off = boff[i], rs = rsize[i];
        PS[i] = br.image_base[p] + small_at + off;
        PL[i] = br.image_base[p] + large_at;
        if (addr) {
            const bool large = rs > B;
            const uint64_t fpos = br.file_size[p] + (large ? large_at : small_at);
            addr[i] = (uint64_t)p << 56 | (uint64_t)((large ? text_large_block(rs) : B) >> 12) << 48 |
                      ((fpos >> 12) & 0xFFFFFFFFull) << 16 | (large ? 0 : off & 0xFFFF);
        }
    }
}

struct TextPackBlocked {
    TextPack t;          // off unused; dst / out_bytes: the chunk's blocked image
    const uint64_t *PS;  // [count + 1] a small record's first byte in the image (sorted; a large record: an empty interval)
    const uint64_t *PL;  // [count + 1] a large record's (sorted; a small record: an empty interval)
    uint32_t B;
};

// The piece loop of piece_copy.hpp and the record writer of k_text_pack.  The
// owner of output byte o is the last small record with PS <= o if o lies
// within its bytes, else the last large record with PL <= o if o lies within
// its bytes, else nobody: the byte is 0 up to the next entry of either list.
__global__ __launch_bounds__(256) void k_text_pack_blocked(TextPackBlocked b) {
    const TextPack &a = b.t;
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
                // a small record?
                uint64_t q = hint, rs = 0;
                uint32_t kl = 0, vl = 0, sz = 0;
                auto load = [&](const uint64_t *list) {
                    rs = list[q];
                    kl = text_klen(a.klen[q]), vl = text_vlen(a.vlen[q]), sz = 3 + kl + vl;
                };
                // record q, which starts at rs, owns o: its bytes up to the piece's end
                auto emit = [&]() {
                    const uint64_t e = rs + sz < pc.o1 ? rs + sz : pc.o1;
                    text_put_record<true>(pc, a, q, kl, vl, (uint32_t)(o - rs), (uint32_t)(e - rs), pc.j0 + (uint32_t)(o - pc.o0));
                    o = e;
                };
                if (q < a.count) load(b.PS);
                if (q >= a.count || rs != o || sz > b.B) {  // (a small record that starts at o is the last entry at or before o)
                    q = get_owner(b.PS, slo, shi, o);
                    load(b.PS);
                }
                hint = a.count;
                if (sz <= b.B && rs <= o && o < rs + sz) {
                    hint = q + 1;
                    emit();
                    continue;
                }
                uint64_t nearest = rs > o ? rs : b.PS[q + 1];  // the next list entry past o (PS[count] ends the image)
                // a large one?
                q = get_owner(b.PL, llo, lhi, o);
                load(b.PL);
                if (sz > b.B && rs <= o && o < rs + sz) {
                    emit();
                    continue;
                }
                const uint64_t nl = rs > o ? rs : b.PL[q + 1];
                nearest = nl < nearest ? nl : nearest;
                o = nearest > o && nearest < pc.o1 ? nearest : pc.o1;  // zeros up to there
            }
        });
}

}  // namespace bsdb
