// piece_copy.hpp -- the output-driven copy of k_get_gather, k_text_pack and
// k_text_pack_blocked on gfx950.  Piece k of a destination (dst, out_bytes)
// is the 16 bytes at (dst & ~15) + 16 k: output bytes [16 k - mis, 16 k - mis
// + 16) cut to [0, out_bytes).  A thread owns a piece: it finds the records
// that overlap it by a search in a sorted offset list -- the wave's first and
// last lanes search all of it, the others between those two results --
// assembles the piece in two registers and stores it once; the first and
// last pieces of the destination byte by byte, inside the destination.  The
// work of a piece does not depend on how long the records around it are.
// Every source byte comes through the bounded reader sel_gload64, and every
// offset read back from memory is tested before it is used: offsets that are
// no scan leave zeros, they never move a store.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "piece_plan.hpp"
#include "spooky_dev.hpp"

namespace bsdb {

// The entry whose bytes hold output byte o: the last q in [lo, hi] with
// off[q] <= o (off[lo] <= o is the caller's).  Empty entries share their
// offset with the next one, so the last one is the one with bytes.
__device__ __forceinline__ uint64_t get_owner(const uint64_t *off, uint64_t lo, uint64_t hi, uint64_t o) {
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (off[mid] <= o) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// A wave step: the owners of the wave's output bytes [w0, w1) among `count`
// entries, searched by the first and the last lane and handed to all.
__device__ __forceinline__ void piece_wave_owners(const uint64_t *off, uint64_t count, uint64_t w0, uint64_t w1, uint64_t &qlo,
                                                  uint64_t &qhi) {
    const uint32_t lane = threadIdx.x & 63;
    qlo = qhi = 0;
    if (lane == 0) qlo = get_owner(off, 0, count - 1, w0);
    if (lane == 63) qhi = get_owner(off, 0, count - 1, w1 - 1);
    qlo = __shfl(qlo, 0, 64);
    qhi = __shfl(qhi, 63, 64);
}

struct Piece {
    uint64_t o0, o1;  // its output bytes [o0, o1)
    uint32_t j0;      // its first valid byte: output byte o is piece byte j0 + (o - o0)
    uint64_t lo = 0, hi = 0;

    // nb <= 8 bytes (the low ones of x) to piece bytes j .. j + nb - 1
    __device__ __forceinline__ void put(uint64_t x, uint32_t j, uint32_t nb) {
        x &= low_bytes_mask(nb);
        if (j < 8) {
            lo |= x << (8 * j);
            if (j) hi |= x >> (64 - 8 * j);
        } else {
            hi |= x << (8 * (j - 8));
        }
    }

    // n bytes at `pos` of the source (base, limit) to piece bytes from j, 8 source bytes a step
    __device__ __forceinline__ void copy(const uint8_t *base, uint64_t limit, uint64_t pos, uint32_t j, uint32_t n) {
        for (uint32_t x = 0; x < n; x += 8) {
            const uint64_t p = pos + x;
            put(p < limit ? sel_gload64(base, limit, p) : 0, j + x, n - x < 8 ? n - x : 8);
        }
    }

    __device__ __forceinline__ void store(uint8_t *dst) const {
        if (o1 - o0 == 16) {
            *reinterpret_cast<ulonglong2 *>(dst) = make_ulonglong2(lo, hi);
        } else {
            for (uint32_t j = j0; j < j0 + (uint32_t)(o1 - o0); ++j) dst[j] = (uint8_t)((j < 8 ? lo >> (8 * j) : hi >> (8 * (j - 8))));
        }
    }
};

// The piece's bytes by the entries of one scan `off` that hold them, the
// owners within the wave's [qlo, qhi]: run(q, start, o, e) for output bytes
// [o, e) of entry q, which starts at output byte `start`.
template <class Run>
__device__ __forceinline__ void piece_runs(const Piece &pc, const uint64_t *off, uint64_t qlo, uint64_t qhi, const Run &run) {
    uint64_t q = qlo;
    bool searched = false;
    for (uint64_t o = pc.o0; o < pc.o1;) {
        if (!searched || off[q + 1] <= o) {  // past q's bytes: the owner of o, within the wave's range
            q = get_owner(off, q < qhi && searched ? q + 1 : q, qhi, o);
            searched = true;
        }
        const uint64_t rs = off[q], re = off[q + 1];
        if (rs > o || re <= o) break;  // offsets that are no scan: the rest stays zero
        const uint64_t e = re < pc.o1 ? re : pc.o1;
        run(q, rs, o, e);
        o = e;
    }
}

// The loop of a kernel of 256-thread workgroups, uniform per wave.
// wave(w0, w1) runs on every lane before the lanes without a piece leave (its
// searches may shuffle); piece(pc) fills one piece and runs no wave-wide
// operation.
template <class Wave, class Fill>
__device__ __forceinline__ void piece_loop(uint8_t *dst, uint64_t out_bytes, const Wave &wave, const Fill &piece) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t mis = (uint32_t)((uintptr_t)dst & 15);
    uint8_t *const aligned = dst - mis;
    const uint64_t pieces = piece_count(out_bytes, mis);
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    auto first_of = [&](uint64_t kk) -> uint64_t { return kk ? kk * 16 - mis : 0; };
    auto end_of = [&](uint64_t kk) -> uint64_t {
        const uint64_t e = kk * 16 + 16 - mis;
        return e < out_bytes ? e : out_bytes;
    };
    for (uint64_t wbase = (uint64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); wbase < pieces; wbase += stride) {
        const uint64_t k = wbase + lane;
        const uint64_t klast = wbase + 63 < pieces ? wbase + 63 : pieces - 1;
        wave(first_of(wbase), end_of(klast));
        if (k >= pieces) continue;  // (no wave-wide operation below)
        Piece pc;
        pc.o0 = first_of(k), pc.o1 = end_of(k);
        pc.j0 = (uint32_t)(pc.o0 + mis - k * 16);
        piece(pc);
        pc.store(aligned + k * 16);
    }
}

}  // namespace bsdb
