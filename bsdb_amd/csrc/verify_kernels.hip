// verify_kernels.hip -- whole-database check on gfx950: key -> signature ->
// rank (checked getLong, GOV:557-569) -> index.db slot -> the record's own
// address (and, index.approximate, its own first value bytes), in ONE pass
// over the records.  What Builder -v does one synchronous lookup at a time
// (Builder.java:184-228, SyncReader.getAsBytes), batched on the device
// (SURVEY.md §8(f) F4).  No signature and no rank is written to memory.
//
// The address test is also the bijection test: record addresses are distinct
// by construction (partition and file offset), so n records that each find
// their own address in an index.db of n slots occupy n different ranks -- no
// seen-bitmap, no per-record atomics.
//
// Report words (bsdb_mi355x.h, BSDB_VERIFY_WORDS): [0] records seen,
// [1] rejected, [2] in_window, [3] wrong_addr, [4] wrong_value,
// [5] min_bad_addr; the kernels add to [0..4] and atomicMin into [5].  Bit 0
// of [6] (set by k_verify_structure) says E is not a valid offset array: the
// record kernels then do nothing, because only a valid E keeps every lookup
// inside values[] (an imported hash.db is untrusted input).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mph_kernels.hip"

namespace bsdb {

enum VerifyWord { VW_RECORDS = 0, VW_REJECTED, VW_IN_WINDOW, VW_WRONG_ADDR, VW_WRONG_VALUE, VW_MIN_BAD, VW_FLAGS, VW_WINDOWS };

struct VerifyArgs {
    const uint8_t *keys;       // fixed: n * key_len bytes; var: blob
    const uint64_t *off;       // var: n + 1 offsets
    uint64_t blob_bytes, n;    // bytes readable at keys; records of this launch
    uint32_t key_len;          // fixed
    const uint64_t *addr;      // n addresses, or null: addr_base + addr_stride * (first + i)
    uint64_t addr_base, addr_stride, first;
    const uint64_t *value8;    // index.approximate: first <= 8 value bytes (LE) and their count
    const uint8_t *vlen;
    uint64_t start, len;       // the window of ranks [start, start + len) held in index / index_a
    const uint64_t *index;     // big-endian addresses
    const uint64_t *index_a;   // 8-byte value slots, or null (exact mode)
    unsigned long long *out;   // the report
};

// E[0]'s offset is 0, the offsets (low 56 bits) never decrease, E[m]'s is n.
// Then every bucket's vertex range lies inside values[] and its ranks below n.
__global__ __launch_bounds__(256) void k_verify_structure(const uint64_t *E, uint64_t m, uint64_t n,
                                                          unsigned long long *out) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    bool bad = false;
    for (uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x; b <= m; b += stride) {
        const uint64_t e = E[b] & OFFSET_MASK;
        if (b == 0 && e != 0) bad = true;
        if (b == m ? e != n : e > (E[b + 1] & OFFSET_MASK)) bad = true;
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(out + VW_FLAGS, 1ULL);
}

// count_nonzero_pairs (mph_kernels.hip) with the whole words in between read
// 16 bytes at a time: the same sum from half the load instructions.  The
// count is this pass's long chain (a bucket's hinge lies ~26 words into its
// vertex range on average).  k_lookup and k_sign keep the 8-byte form.
__device__ __forceinline__ uint64_t count_nonzero_pairs_wide(uint64_t start, uint64_t end, const uint64_t *a) {
    uint64_t blk = start >> 5;
    const uint64_t end_blk = end >> 5;
    const uint32_t so = (uint32_t)(start & 31), eo = (uint32_t)(end & 31);
    if (blk == end_blk) return nz_pairs((a[blk] & ((1ULL << (eo * 2)) - 1)) >> (so * 2));
    uint64_t pairs = 0;
    if (so) pairs += nz_pairs(a[blk++] >> (so * 2));
    if (blk < end_blk && ((uintptr_t)(a + blk) & 8)) pairs += nz_pairs(a[blk++]);  // up to a 16-byte boundary
    for (; blk + 2 <= end_blk; blk += 2) {
        const ulonglong2 w = *reinterpret_cast<const ulonglong2 *>(a + blk);
        pairs += nz_pairs(w.x) + nz_pairs(w.y);
    }
    if (blk < end_blk) pairs += nz_pairs(a[blk++]);
    if (eo) pairs += nz_pairs(a[blk] & ((1ULL << (eo * 2)) - 1));
    return pairs;
}

// mph_lookup (getLongBySignature, GOV:557-569) over the wide count
__device__ __forceinline__ int64_t mph_lookup_wide(const MphView &v, uint64_t sig0, uint64_t sig1) {
    const uint32_t b = bucket_of_w(w64(sig0), v.mult);
    const uint64_t eos = v.E[b];
    const uint64_t vo = vertex_offset(eos);
    const uint32_t nv = (uint32_t)(vertex_offset(v.E[b + 1]) - vo);
    uint32_t e[3];
    sig_to_equation(sig0, sig1, eos & ~OFFSET_MASK, nv, e);
    const uint32_t h = (two_bit(v.values, vo + e[0]) + two_bit(v.values, vo + e[1]) + two_bit(v.values, vo + e[2])) % 3;
    const uint64_t r = (eos & OFFSET_MASK) + count_nonzero_pairs_wide(vo, vo + e[h], v.values);
    if (r >= v.n) return -1;
    if (v.width) {
        const uint64_t mask = v.width == 64 ? ~0ULL : ((1ULL << v.width) - 1);
        if (bitlist_get(v.sigs, r, v.width) != (sig0 & mask)) return -1;
    }
    return (int64_t)r;
}

// KIND 0: 13-byte keys (one dword-aligned 16-byte window per key), 1: fixed
// key_len, 2: variable length -- the readers of the pass build's re-hash
// (k_sel, gov_kernels.hip).  One record per lane; the loop is uniform per
// wave (inactive tail lanes are predicated off) so the ballots see all lanes.
template <int KIND>
__device__ __forceinline__ void verify_records(const MphView &v, const VerifyArgs &a) {
    typedef unsigned int u32x4w __attribute__((ext_vector_type(4), aligned(4)));
    if (a.out[VW_FLAGS] & 1) return;  // E invalid: no lookup is safe
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    uint64_t seen = 0, rejected = 0, in_window = 0, wrong_addr = 0, wrong_value = 0;  // wave totals
    uint64_t min_bad = ~0ULL;                                                        // this lane's
    for (uint64_t base = (uint64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); base < a.n; base += stride) {
        const uint64_t i = base + lane;
        const bool active = i < a.n;
        bool rej = false, inw = false, wa = false, wv = false;
        if (active) {
            uint64_t s0, s1;
            if (KIND == 0) {
                const uint64_t byte = i * 13, al = byte & ~3ULL;
                if (al + 16 <= a.blob_bytes) {
                    const u32x4w w = __builtin_nontemporal_load(reinterpret_cast<const u32x4w *>(a.keys + al));
                    W64 x0, x1;
                    spooky13_u(w.x, w.y, w.z, w.w, (uint32_t)(byte & 3) * 8, 0, x0, x1);
                    s0 = u64(x0);
                    s1 = u64(x1);
                } else {
                    auto rd = [&](uint32_t o) -> uint64_t { return sel_gload64(a.keys, a.blob_bytes, byte + o); };
                    spooky_short(rd, 13, 0, s0, s1);
                }
            } else {
                const uint64_t pos = KIND == 2 ? a.off[i] : i * a.key_len;
                const uint32_t len = KIND == 2 ? (uint32_t)(a.off[i + 1] - pos) : a.key_len;
                auto rd = [&](uint32_t o) -> uint64_t { return sel_gload64(a.keys, a.blob_bytes, pos + o); };
                spooky_short(rd, len, 0, s0, s1);
            }
            const uint64_t ad = a.addr ? a.addr[i] : a.addr_base + a.addr_stride * (a.first + i);
            const int64_t r = mph_lookup_wide(v, s0, s1);
            rej = r < 0;
            const uint64_t idx = (uint64_t)r - a.start;
            inw = !rej && (uint64_t)r >= a.start && idx < a.len;
            if (inw) {
                wa = a.index[idx] != __builtin_bswap64(ad);
                if (a.index_a) {
                    const uint32_t l = a.vlen[i] < 8 ? a.vlen[i] : 8;  // bytes past vlen: unspecified (W:141)
                    wv = ((a.index_a[idx] ^ a.value8[i]) & low_bytes_mask(l)) != 0;
                }
            }
            if (rej || wa || wv) min_bad = ad < min_bad ? ad : min_bad;
        }
        seen += __popcll(__ballot(active));
        rejected += __popcll(__ballot(rej));
        in_window += __popcll(__ballot(inw));
        wrong_addr += __popcll(__ballot(wa));
        wrong_value += __popcll(__ballot(wv));
    }
    for (int d = 32; d; d >>= 1) {
        const uint64_t o = __shfl_xor(min_bad, d, 64);
        min_bad = o < min_bad ? o : min_bad;
    }
    if (lane == 0) {
        if (seen) atomicAdd(a.out + VW_RECORDS, (unsigned long long)seen);
        if (rejected) atomicAdd(a.out + VW_REJECTED, (unsigned long long)rejected);
        if (in_window) atomicAdd(a.out + VW_IN_WINDOW, (unsigned long long)in_window);
        if (wrong_addr) atomicAdd(a.out + VW_WRONG_ADDR, (unsigned long long)wrong_addr);
        if (wrong_value) atomicAdd(a.out + VW_WRONG_VALUE, (unsigned long long)wrong_value);
        if (min_bad != ~0ULL) atomicMin(a.out + VW_MIN_BAD, (unsigned long long)min_bad);
    }
}

template <bool K13>
__global__ __launch_bounds__(256) void k_verify_fixed(MphView v, VerifyArgs a) {
    verify_records<K13 ? 0 : 1>(v, a);
}

__global__ __launch_bounds__(256) void k_verify_var(MphView v, VerifyArgs a) { verify_records<2>(v, a); }

}  // namespace bsdb
