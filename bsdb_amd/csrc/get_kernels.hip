// get_kernels.hip -- batched get on gfx950: key -> value out of a database
// resident in HBM.  What SyncReader.getAsBytes does one key per call
// (read/SyncReader.java:44-57 -> BaseKVReader.getValueAsBytes,
// read/kv/BaseKVReader.java:16-31), in two kernels with the offset scan
// (k_scan_*, hash_kernels.hip) between them:
//   k_get_locate  key -> signature -> rank (checked getLong) -> index.db slot
//                 -> address (get_decode, get_plan.hpp) -> record header ->
//                 key compare; writes where each value lies and how long it is
//   k_get_gather  copies the values into the packed output, driven by the
//                 output: a thread owns an aligned 16-byte piece of it
// The key readers, the hash and the lookup are verify's (verify_kernels.hip).
//
// index.db is untrusted: every address is bounds-tested against the image
// before the record is touched, and every read of the image goes through the
// bounded reader sel_gload64 with the record's own container (partition or
// block) as its limit.  Approximate mode reads no record: the value is the 8
// raw bytes of the index_a.db slot (LBufferIndexReader.getRawBytesAt).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "get_plan.hpp"
#include "verify_kernels.hip"

namespace bsdb {

struct GetDb {
    const uint8_t *image;     // exact: the kv.db partitions; approximate: index_a.db
    uint64_t image_bytes;
    const uint64_t *index;    // exact: n big-endian addresses
    const uint64_t *base;     // [partitions] byte position of each partition in the image
    const uint64_t *size;     // [partitions] its file size
    uint32_t partitions;
    int format;               // 0 compact, 1 blocked
    int approx;
};

struct GetArgs {
    const uint8_t *keys;      // fixed: nq * key_len bytes; var: blob
    const uint64_t *off;      // var: nq + 1 offsets
    uint64_t blob_bytes, nq;
    uint32_t key_len;         // fixed
    uint64_t *src;            // per query: byte position of the value in the image (approximate: the slot)
    uint32_t *vlen;           // its length (0 unless found)
    uint8_t *status;          // BSDB_GET_*
    unsigned long long *out;  // the report, GW_WORDS
};

// KIND as verify_records: 0 13-byte keys, 1 fixed key_len, 2 variable length.
// One query per lane; the loop is uniform per wave so the ballots see all lanes.
template <int KIND>
__device__ __forceinline__ void get_locate(const MphView &v, const GetDb &db, const GetArgs &a) {
    typedef unsigned int u32x4w __attribute__((ext_vector_type(4), aligned(4)));
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    uint64_t seen = 0, found = 0, rejected = 0, mismatch = 0, bad_addr = 0;  // wave totals
    uint64_t bytes = 0;                                                      // this lane's
    for (uint64_t base = (uint64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); base < a.nq; base += stride) {
        const uint64_t i = base + lane;
        const bool active = i < a.nq;
        int st = -1;
        if (active) {
            uint64_t s0, s1;
            const uint64_t kpos = KIND == 2 ? a.off[i] : i * (KIND == 0 ? 13 : a.key_len);
            const uint32_t klen = KIND == 2 ? (uint32_t)(a.off[i + 1] - kpos) : (KIND == 0 ? 13 : a.key_len);
            auto rdk = [&](uint32_t o) -> uint64_t { return sel_gload64(a.keys, a.blob_bytes, kpos + o); };
            const uint64_t al = kpos & ~3ULL;
            if (KIND == 0 && al + 16 <= a.blob_bytes) {
                const u32x4w w = __builtin_nontemporal_load(reinterpret_cast<const u32x4w *>(a.keys + al));
                W64 x0, x1;
                spooky13_u(w.x, w.y, w.z, w.w, (uint32_t)(kpos & 3) * 8, 0, x0, x1);
                s0 = u64(x0);
                s1 = u64(x1);
            } else {
                spooky_short(rdk, klen, 0, s0, s1);
            }
            const int64_t r = mph_lookup_wide(v, s0, s1);
            uint64_t src = 0;
            uint32_t vl = 0;
            st = GET_REJECTED;
            if (r >= 0 && db.approx) {
                st = GET_FOUND;
                src = (uint64_t)r;
                vl = 8;
            } else if (r >= 0) {
                st = GET_BAD_ADDR;
                const GetRecord rec = get_decode(__builtin_bswap64(db.index[r]), db.format, db.size, db.partitions);
                if (rec.ok) {
                    const uint64_t pb = db.base[rec.part];
                    const uint64_t lim = pb + rec.limit, p = pb + rec.pos;  // p + 3 <= lim <= image_bytes
                    const uint64_t h = sel_gload64(db.image, lim, p);
                    const uint32_t kl = (uint32_t)(h & 0xFF);               // BaseKVReader.java:19-20
                    const uint32_t vb = (uint32_t)((h >> 8) & 0xFF) << 8 | (uint32_t)((h >> 16) & 0xFF);
                    if (p + 3 + kl + vb <= lim) {
                        bool same = kl == klen;                              // BaseKVReader.java:66-69
                        for (uint32_t o = 0; same && o < kl; o += 8) {
                            const uint32_t k = kl - o < 8 ? kl - o : 8;
                            same = ((sel_gload64(db.image, lim, p + 3 + o) ^ rdk(o)) & low_bytes_mask(k)) == 0;
                        }
                        st = same ? GET_FOUND : GET_KEY_MISMATCH;
                        if (same) {
                            src = p + 3 + kl;
                            vl = vb;
                        }
                    }
                }
            }
            a.src[i] = src;
            a.vlen[i] = vl;
            a.status[i] = (uint8_t)st;
            bytes += vl;
        }
        seen += __popcll(__ballot(active));
        found += __popcll(__ballot(st == GET_FOUND));
        rejected += __popcll(__ballot(st == GET_REJECTED));
        mismatch += __popcll(__ballot(st == GET_KEY_MISMATCH));
        bad_addr += __popcll(__ballot(st == GET_BAD_ADDR));
    }
    for (int d = 32; d; d >>= 1) bytes += __shfl_xor(bytes, d, 64);
    if (lane == 0) {
        if (seen) atomicAdd(a.out + GW_QUERIES, (unsigned long long)seen);
        if (found) atomicAdd(a.out + GW_FOUND, (unsigned long long)found);
        if (rejected) atomicAdd(a.out + GW_REJECTED, (unsigned long long)rejected);
        if (mismatch) atomicAdd(a.out + GW_KEY_MISMATCH, (unsigned long long)mismatch);
        if (bad_addr) atomicAdd(a.out + GW_BAD_ADDR, (unsigned long long)bad_addr);
        if (bytes) atomicAdd(a.out + GW_VALUE_BYTES, (unsigned long long)bytes);
    }
}

template <int KIND>
__global__ __launch_bounds__(256) void k_get_locate(MphView v, GetDb db, GetArgs a) {
    get_locate<KIND>(v, db, a);
}

// The query whose value holds output byte o: the last q in [lo, hi] with
// voff[q] <= o (voff[lo] <= o is the caller's).  Empty values share their
// offset with the next query, so the last one is the one with bytes.
__device__ __forceinline__ uint64_t get_owner(const uint64_t *voff, uint64_t lo, uint64_t hi, uint64_t o) {
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (voff[mid] <= o) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

struct GatherArgs {
    const uint8_t *image;
    uint64_t image_bytes;
    uint32_t scale;        // bytes per unit of src: 1, or 8 when src is a slot (approximate)
    const uint64_t *src;   // [nq]
    const uint64_t *voff;  // [nq + 1] exclusive scan of the value lengths
    uint64_t nq;
    uint8_t *values;       // the packed output, value_bytes long, at any alignment
    uint64_t value_bytes;
};

// Piece k is the 16 bytes at (values & ~15) + 16 k: output bytes
// [16 k - mis, 16 k - mis + 16) cut to [0, value_bytes).  A thread finds the
// queries its piece overlaps by a search in voff -- the wave's first and last
// lanes search all of it, the others between those two results -- assembles
// the piece from its sources in registers and stores it once (the first and
// last pieces of the whole output byte by byte, inside the output).  The work
// of a piece does not depend on how long the values around it are: a run of
// empty values is stepped over by the search, a long value is shared by as
// many threads as it has pieces.
__global__ __launch_bounds__(256) void k_get_gather(GatherArgs a) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t mis = (uint32_t)((uintptr_t)a.values & 15);
    uint8_t *const aligned = a.values - mis;
    const uint64_t pieces = get_gather_pieces(a.value_bytes, mis);
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t wbase = (uint64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); wbase < pieces; wbase += stride) {
        const uint64_t k = wbase + lane;
        const bool active = k < pieces;
        // this piece's output bytes [o0, o1); the wave's [w0, w1)
        const uint64_t klast = wbase + 63 < pieces ? wbase + 63 : pieces - 1;
        auto first_of = [&](uint64_t kk) -> uint64_t { return kk ? kk * 16 - mis : 0; };
        auto end_of = [&](uint64_t kk) -> uint64_t {
            const uint64_t e = kk * 16 + 16 - mis;
            return e < a.value_bytes ? e : a.value_bytes;
        };
        const uint64_t w0 = first_of(wbase), w1 = end_of(klast);
        uint64_t qlo = 0, qhi = 0;
        if (lane == 0) qlo = get_owner(a.voff, 0, a.nq - 1, w0);
        if (lane == 63) qhi = get_owner(a.voff, 0, a.nq - 1, w1 - 1);
        qlo = __shfl(qlo, 0, 64);
        qhi = __shfl(qhi, 63, 64);
        if (!active) continue;  // (no wave-wide operation below)
        const uint64_t o0 = first_of(k), o1 = end_of(k);
        const uint32_t j0 = (uint32_t)(o0 + mis - k * 16);  // the piece's first valid byte
        uint64_t lo = 0, hi = 0;
        uint64_t q = qlo;
        bool searched = false;
        for (uint64_t o = o0; o < o1;) {
            if (!searched || a.voff[q + 1] <= o) {  // past q's value: the owner of o, within the wave's range
                q = get_owner(a.voff, q < qhi && searched ? q + 1 : q, qhi, o);
                searched = true;
            }
            const uint64_t vs = a.voff[q], ve = a.voff[q + 1];
            if (vs > o || ve <= o) break;  // offsets that are no scan of lengths: the rest stays zero
            const uint64_t run_end = ve < o1 ? ve : o1;
            const uint64_t sp = a.src[q] * a.scale + (o - vs);
            for (uint64_t t = o; t < run_end; t += 8) {
                const uint32_t nb = run_end - t < 8 ? (uint32_t)(run_end - t) : 8;
                const uint64_t p = sp + (t - o);
                const uint64_t x = (p < a.image_bytes ? sel_gload64(a.image, a.image_bytes, p) : 0) & low_bytes_mask(nb);
                const uint32_t j = j0 + (uint32_t)(t - o0);  // byte of the piece, 0..15
                if (j < 8) {
                    lo |= x << (8 * j);
                    if (j) hi |= x >> (64 - 8 * j);
                } else {
                    hi |= x << (8 * (j - 8));
                }
            }
            o = run_end;
        }
        uint8_t *dst = aligned + k * 16;
        if (o1 - o0 == 16) {
            *reinterpret_cast<ulonglong2 *>(dst) = make_ulonglong2(lo, hi);
        } else {
            for (uint32_t j = j0; j < j0 + (uint32_t)(o1 - o0); ++j) dst[j] = (uint8_t)((j < 8 ? lo >> (8 * j) : hi >> (8 * (j - 8))));
        }
    }
}

}  // namespace bsdb
