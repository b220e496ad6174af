// dup_kernels.hip -- which keys are duplicates: the kernels
// that read a bucket range the build's grouping (gov_group: count, scan,
// scatter of (signature, position), k_bucket_sort / k_bucket_sort_big) left
// sorted.  Equal signatures are neighbours there, so a group of r equal keys
// is a run of r entries; it is reported as r - 1 pairs (smallest position of
// the run, other position).  Duplicates are rare: the kernels are one pass of
// neighbour compares, and only a wave that holds a run's first entry takes an
// atomic on the list cursor.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gov_kernels.hip"

namespace bsdb {

// report words (BSDB_DUP_WORDS of include/bsdb_mi355x.h)
enum DupWord : int { DUP_FOUND = 0, DUP_COLLISIONS = 1, DUP_FLAGS = 2, DUP_KEYS = 3 };
enum DupFlag : uint64_t { DUP_F_LIST_FULL = 1, DUP_F_PARTIAL = 2 };
enum DupKind : uint8_t { DUP_SAME_KEY = 0, DUP_COLLISION = 1, DUP_UNCOMPARED = 2 };

__device__ __forceinline__ uint64_t dup_shfl64(uint64_t v, int src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, 64);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 64);
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint64_t dup_shfl_up64(uint64_t v, uint32_t d) {
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d, 64);
    const uint32_t hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d, 64);
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ bool sig_eq(ulonglong2 a, ulonglong2 b) { return a.x == b.x && a.y == b.y; }

// Buckets over GB_CMAX keys (the sort's limit; k_big_list only flags them):
// each one's slice is cut into consecutive chunks of at most GB_CMAX entries.
// A bucket of c chunks takes c + 1 consecutive boundaries in Ec (global
// offsets, the form of Eb) and c entries of `list`, each the index of its
// chunk's first boundary: k_bucket_sort_big and k_dup_collect then take
// (Ec, list) as they take (Eb, the oversized buckets' list).  counters[0]:
// list entries, counters[1]: boundaries; both count past the capacities (the
// plan's bounds hold for every input; a full list only drops chunks).
__global__ __launch_bounds__(256) void k_dup_over_list(const uint64_t *Eb, uint64_t nb, uint64_t *Ec, uint32_t ec_cap,
                                                       uint32_t *list, uint32_t list_cap, uint32_t *counters) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x; b < nb; b += stride) {
        const uint64_t lo = Eb[b] & OFFSET_MASK, hi = Eb[b + 1] & OFFSET_MASK;
        const uint64_t cnt = hi - lo;
        if (cnt <= (uint64_t)GB_CMAX) continue;
        const uint32_t nch = (uint32_t)((cnt + GB_CMAX - 1) / GB_CMAX);
        const uint32_t l0 = atomicAdd(counters, nch);
        const uint32_t e0 = atomicAdd(counters + 1, nch + 1);
        if ((uint64_t)l0 + nch > list_cap || (uint64_t)e0 + nch + 1 > ec_cap) continue;
        for (uint32_t k = 0; k < nch; ++k) {
            Ec[e0 + k] = lo + (uint64_t)k * GB_CMAX;
            list[l0 + k] = e0 + k;
        }
        Ec[e0 + nch] = hi;
    }
}

// The runs of equal signatures of sorted segments: bucket b of Eb (list ==
// nullptr; buckets over GB_CMAX keys are not sorted and are skipped), or the
// segment list[i] of Eb for i < nseg.  The entry whose predecessor in the
// segment differs and whose successor is equal leads a run: it walks the run
// for its smallest position, and the run's other members are appended as
// (smallest, other) at the list cursor report[DUP_FOUND], which always counts
// every pair; writes stop at cap.  One ballot per wave and step, one cursor
// atomic per wave that leads any run.  pos (optional): the position of entry
// i is pos[pay[i]] (a pass whose source is a compacted copy: spill mode).
__global__ __launch_bounds__(256) void k_dup_collect(const uint64_t *sig, const uint64_t *pay, const uint64_t *pos,
                                                     const uint64_t *Eb, uint64_t nseg, const uint32_t *list, uint64_t e0,
                                                     uint64_t cap, uint64_t *pairs, uint64_t *report) {
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    for (uint64_t si = blockIdx.x; si < nseg; si += gridDim.x) {
        const uint64_t b = list ? (uint64_t)list[si] : si;
        const uint64_t lo = (Eb[b] & OFFSET_MASK) - e0, hi = (Eb[b + 1] & OFFSET_MASK) - e0;
        const uint64_t cnt = hi - lo;
        if (cnt < 2 || cnt > (uint64_t)GB_CMAX) continue;
        const ulonglong2 *g = reinterpret_cast<const ulonglong2 *>(sig) + lo;
        const uint64_t *gp = pay + lo;
        auto position = [&](uint64_t i) -> uint64_t { return pos ? pos[gp[i]] : gp[i]; };
        for (uint64_t i0 = 0; i0 < cnt; i0 += 256) {  // (uniform trip count)
            const uint64_t i = i0 + tid;
            bool leader = false;
            ulonglong2 cur = make_ulonglong2(0, 0);
            if (i + 1 < cnt) {
                cur = g[i];
                leader = sig_eq(g[i + 1], cur) && !(i && sig_eq(g[i - 1], cur));
            }
            if (!__builtin_amdgcn_ballot_w64(leader)) continue;
            uint64_t others = 0, mn = 0;
            if (leader) {
                mn = position(i);
                for (uint64_t j = i + 1; j < cnt && sig_eq(g[j], cur); ++j) {
                    mn = min(mn, position(j));
                    ++others;
                }
            }
            // the wave's pairs: an exclusive prefix of the leaders' counts, one atomic for their sum
            uint64_t inc = others;
#pragma unroll
            for (uint32_t d = 1; d < 64; d <<= 1) {
                const uint64_t y = dup_shfl_up64(inc, d);
                if (lane >= d) inc += y;
            }
            const uint64_t total = dup_shfl64(inc, 63);
            uint64_t base = 0;
            if (lane == 0) base = atomicAdd(reinterpret_cast<unsigned long long *>(report + DUP_FOUND), (unsigned long long)total);
            base = dup_shfl64(base, 0);
            if (leader) {
                uint64_t at = base + inc - others;
                for (uint64_t j = i; j < i + others + 1 && at < cap; ++j) {
                    const uint64_t p = position(j);
                    if (p == mn) continue;
                    pairs[2 * at] = mn;
                    pairs[2 * at + 1] = p;
                    ++at;
                }
            }
        }
    }
}

// The same bounds-checked dword-aligned read as the hash's (sel_gload64), so
// the compare sees the bytes the signatures were computed from.
// KIND 1: keys of key_len bytes back to back; KIND 2: blob + offsets.
// One pair per lane: lengths first, then 8 bytes a step; kinds[i] = 0 when the
// two keys are the same bytes, 1 when they differ (counted in
// report[DUP_COLLISIONS], one atomic per wave that saw any).
template <int KIND>
__global__ __launch_bounds__(256) void k_dup_classify(const uint8_t *keys, const uint64_t *off, uint64_t blob_bytes,
                                                      uint64_t n, uint32_t key_len, const uint64_t *pairs, uint64_t count,
                                                      uint8_t *kinds, uint64_t *report) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t rounds = (count + stride - 1) / stride;
    for (uint64_t r = 0; r < rounds; ++r) {  // (uniform: the ballot below)
        const uint64_t i = r * stride + (uint64_t)blockIdx.x * 256 + threadIdx.x;
        bool differ = false;
        if (i < count) {
            const uint64_t a = pairs[2 * i], b = pairs[2 * i + 1];
            if (a >= n || b >= n) {
                differ = true;  // (not a position of the key set)
            } else {
                const uint64_t pa = KIND == 2 ? off[a] : a * key_len, pb = KIND == 2 ? off[b] : b * key_len;
                const uint64_t la = KIND == 2 ? off[a + 1] - pa : key_len, lb = KIND == 2 ? off[b + 1] - pb : key_len;
                differ = la != lb || pa + la > blob_bytes || pb + lb > blob_bytes;
                for (uint64_t o = 0; !differ && o < la; o += 8) {
                    uint64_t x = sel_gload64(keys, blob_bytes, pa + o) ^ sel_gload64(keys, blob_bytes, pb + o);
                    if (la - o < 8) x &= (1ULL << (8 * (la - o))) - 1;
                    differ = x != 0;
                }
            }
            kinds[i] = differ ? DUP_COLLISION : DUP_SAME_KEY;
        }
        const uint64_t bal = __builtin_amdgcn_ballot_w64(differ);
        if (bal && lane == 0 && report)
            atomicAdd(reinterpret_cast<unsigned long long *>(report + DUP_COLLISIONS), (unsigned long long)__builtin_popcountll(bal));
    }
}

// the report's flags and key count, once the passes are done
__global__ void k_dup_report(uint64_t *report, uint64_t cap, uint64_t flags, uint64_t keys) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        report[DUP_FLAGS] = flags | (report[DUP_FOUND] > cap ? (uint64_t)DUP_F_LIST_FULL : 0);
        report[DUP_KEYS] = keys;
    }
}

}  // namespace bsdb
