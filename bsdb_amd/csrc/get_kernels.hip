// get_kernels.hip -- batched get on gfx950: key -> value out of a database
// resident in HBM.  What SyncReader.getAsBytes does one key per call
// (read/SyncReader.java:44-57 -> BaseKVReader.getValueAsBytes,
// read/kv/BaseKVReader.java:16-31), in two kernels with the offset scan
// (k_scan_*, hash_kernels.hip) between them:
//   k_get_locate  key -> signature -> rank (checked getLong) -> index.db slot
//                 -> address (get_decode, get_plan.hpp) -> record header ->
//                 key compare; writes where each value lies and how long it is
//   k_get_gather  copies the values into the packed output, driven by the
//                 output: a thread owns an aligned 16-byte piece of it (the
//                 piece loop, its search and its store: piece_copy.hpp)
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
#include "piece_copy.hpp"
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

// The record an index.db slot names (`addr`: the slot's word, byte-swapped):
// its address decoded and bounds-tested (get_decode), its 3-byte header read,
// and the whole record tested against its container's end.  !ok is
// BSDB_GET_BAD_ADDR.  The key is image bytes [p + 3, p + 3 + kl), the value the
// vb bytes after it; every read of them takes `lim` as its limit.
// k_get_locate and k_db_records (dump_kernels.hip) both start here.
struct GetSlot {
    bool ok;
    uint64_t p, lim;  // the record's and its container's end's byte position in the image
    uint32_t kl, vb;  // BaseKVReader.java:19-20
};

__device__ __forceinline__ GetSlot get_slot(const GetDb &db, uint64_t addr) {
    GetSlot s = {false, 0, 0, 0, 0};
    const GetRecord rec = get_decode(addr, db.format, db.size, db.partitions);
    if (!rec.ok) return s;
    const uint64_t pb = db.base[rec.part];
    s.lim = pb + rec.limit, s.p = pb + rec.pos;  // p + 3 <= lim <= image_bytes
    const uint64_t h = sel_gload64(db.image, s.lim, s.p);
    s.kl = (uint32_t)(h & 0xFF);
    s.vb = (uint32_t)((h >> 8) & 0xFF) << 8 | (uint32_t)((h >> 16) & 0xFF);
    s.ok = s.p + 3 + s.kl + s.vb <= s.lim;
    return s;
}

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
                const GetSlot rec = get_slot(db, __builtin_bswap64(db.index[r]));
                if (rec.ok) {
                    const uint64_t lim = rec.lim, p = rec.p;
                    const uint32_t kl = rec.kl;
                    bool same = kl == klen;                              // BaseKVReader.java:66-69
                    for (uint32_t o = 0; same && o < kl; o += 8) {
                        const uint32_t k = kl - o < 8 ? kl - o : 8;
                        same = ((sel_gload64(db.image, lim, p + 3 + o) ^ rdk(o)) & low_bytes_mask(k)) == 0;
                    }
                    st = same ? GET_FOUND : GET_KEY_MISMATCH;
                    if (same) {
                        src = p + 3 + kl;
                        vl = rec.vb;
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


// The piece loop of piece_copy.hpp over the packed values: a piece's owners
// are the queries whose values overlap it, found in voff; a run of empty
// values is stepped over by the search, a long value is shared by as many
// threads as it has pieces.
__global__ __launch_bounds__(256) void k_get_gather(GatherArgs a) {
    uint64_t qlo, qhi;
    piece_loop(
        a.values, a.value_bytes, [&](uint64_t w0, uint64_t w1) { piece_wave_owners(a.voff, a.nq, w0, w1, qlo, qhi); },
        [&](Piece &pc) {
            piece_runs(pc, a.voff, qlo, qhi, [&](uint64_t q, uint64_t vs, uint64_t o, uint64_t e) {
                pc.copy(a.image, a.image_bytes, a.src[q] * a.scale + (o - vs), pc.j0 + (uint32_t)(o - pc.o0), (uint32_t)(e - o));
            });
        });
}

}  // namespace bsdb
