// hist_plan.hpp -- what a histogram call launches, decided on the host from
// plain numbers: the pass-1 kernel, the id regions' layout and sizes, the
// launch length, the launches per span, and every launch's key range, blob
// limit, tiles, grid and tail.  histogram_impl (capi_hist.hip) fills a HistIn
// from the call, the context, the environment and the runtime, and enqueues
// what the HistPlan enumerates.  Host-only C++17: no HIP, no getenv, so the
// arithmetic runs (and is checked, tests/hist_plan_check.cpp) without a GPU.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "hist_geometry.hpp"

namespace bsdb {

// Keys per pass-1 LAUNCH (bsdb_set_chunk_keys).  A span's launches append to one region set and pass 2 runs once
// per span (hist_size), so the length costs pass 2 and the workspace nothing.  C4 step ms, median of 3
// (profiles/launch_length/): 2^32 42.73, 2^31 42.67, 2^30 42.72, 2^29 42.96, 2^28 43.37, 2^27 44.32 -- level down to
// 2^30, then ~18 us per further launch.  Longer (earlier kernel): 2^33 284 G keys/s against 286, one launch 266.
constexpr uint64_t DEFAULT_CHUNK_KEYS = 1ULL << 32;

// Everything a plan depends on.
struct HistIn {
    // the key set
    bool var = false;        // variable-length keys (offsets)
    uint32_t key_len = 0;    // fixed layouts only
    uint64_t n = 0, m = 0, blob_bytes = 0;
    bool seed0 = false;      // the seed is 0
    // the knobs (bsdb_ctx, the call's options, the environment)
    int hist_mode = 0, frontend = 0, d13_variant = 13, d13_copies = 8;
    uint64_t chunk_keys = 0;  // keys per pass-1 launch (0 = DEFAULT_CHUNK_KEYS)
    uint64_t span_max = 0;    // pass-1 launches per pass 2, at most (0 = no limit)
    bool pipe = false;        // pass 2 of a chunk beside pass 1 of the next
    uint64_t pipe_chunks = 0;
    uint32_t pipe_cus = 0;
    bool no_fixed_window = false;  // BSDB_NO_FIXED_WINDOW
    bool no_seed0 = false;         // BSDB_NO_SEED0
    int64_t d13_grid = INT64_MAX;  // BSDB_D13_GRID (unset: no limit)
    // the device
    int num_cus = 256;
    int wg_per_cu = 0;      // resident workgroups per CU of the chosen kernel (< 1: unknown, taken as 1)
    size_t free_bytes = 0;  // device memory free now
    size_t ids_bytes = 0;   // id bytes the context already holds
};

// The persistent pass-1 kernel of a key set, or none: the
// one-tile-per-workgroup kernels of launch_pass1.
enum class P1Kind { NONE, D13, D13E, VARE };  // k_pass1_d13<D13_NT>, k_pass1_d13e, k_pass1_vare

struct Pass1Choice {
    P1Kind kind = P1Kind::NONE;
    uint32_t key_len = 0;  // 0: variable-length keys
    bool seed0 = false;    // the kernel with the seed folded at compile time
    int variant = 0;       // k_pass1_d13e's VARIANT
    int nt() const { return kind == P1Kind::D13 ? D13_NT : kind == P1Kind::D13E ? D13E_NT : kind == P1Kind::VARE ? VARE_NT : 0; }
    // keys per tile
    uint64_t tile() const {
        return kind == P1Kind::D13 ? (uint64_t)D13_NT * P1_KEYS_PER_THREAD : kind == P1Kind::D13E ? D13E_TILE : kind == P1Kind::VARE ? VARE_TILE : 0;
    }
    // runs padded to 8 ids, region copies = d13_copies
    bool binned() const { return kind == P1Kind::D13E || kind == P1Kind::VARE; }
    // fixed-length keys read as 16-byte windows (k_pass1_d13e, k_pass1_d13), not k_pass1_vare
    bool windowed() const { return kind == P1Kind::D13E || kind == P1Kind::D13; }
};

// Keys [k0, k0 + nk) of the call; blob: the bytes readable from key k0 on
// (variable-length keys: the whole blob's, whose base does not move).
struct KeyRange {
    uint64_t k0 = 0, nk = 0, blob = 0;
};

// A span: consecutive pass-1 launches into one region set, then one pass 2.
struct HistSpan {
    KeyRange r;
    uint64_t launches = 0;
    uint32_t buf = 0;      // id buffer
    uint32_t p2_grid = 0;  // workgroups of its pass 2
};

struct HistLaunch {
    KeyRange r;
    uint64_t tiles = 0;      // the persistent kernel's whole tiles (no such kernel: P1_TILE tiles, one per workgroup)
    uint32_t grid = 0;       // the persistent kernel's workgroups
    KeyRange tail;           // the rest, to the bounds-checked kernel in the tail regions (nk == 0: none)
    uint64_t tail_tiles = 0;
};

inline uint64_t p1_tiles(uint64_t nk) { return (nk + P1_TILE - 1) / P1_TILE; }
inline uint64_t round64(double x) { return ((uint64_t)x + 63) & ~63ULL; }

struct HistPlan {
    bool atomic_mode = false;  // direct atomics: one launch_pass1<EPI_ATOMIC> over the call
    Pass1Choice k;
    // the id regions of a span
    uint32_t nparts = 0;     // region bins: bucket >> bin_shift
    uint32_t bin_shift = 0;  // <= PART_SHIFT; bins nest in the 32768-bucket pass-2 partitions
    uint32_t capb = 0;       // binned kernels: ids per LDS bin
    uint32_t nmain = 0;      // region copies shared by the workgroups of one XCD
    uint32_t ntail = 0;      // persistent kernels: NCOPY regions of the bounds-checked tail kernel
    uint32_t grid_d13 = 0;   // persistent workgroups (0 = generic path)
    uint64_t cap = 0;        // ids per (bin, main region), multiple of 64
    uint64_t cap_tail = 0;   // ids per (bin, tail region), multiple of 64
    uint64_t keys_per_copy = 0;  // the most keys one copy takes (a bin's cursor cannot pass it)
    // the launches
    uint64_t launch = 0;    // keys per pass-1 launch
    uint64_t per_span = 1;  // launches per span
    bool pipe = false;      // pipelined: two id buffers, spans of one launch
    uint32_t nbuf = 1;
    uint32_t p2_cus = 0;    // pipelined: the CUs pass 2 keeps while pass 1 runs
    bool bottomed_out = false;  // the halving ended at launches of <= 2 P1_TILE keys with a rule still unmet
    // the call (for the enumeration)
    bool var = false;
    uint32_t key_len = 0;
    uint64_t n = 0, blob_bytes = 0;
    uint32_t num_cus = 0;

    // Layout of a buffer's ids: [nmain][P][cap], then the tail kernel's
    // [ntail][P][cap_tail]; of its cursors: [nmain][P], then the tail's.
    size_t set_elems() const { return (size_t)nparts * nmain * cap; }
    size_t tail_elems() const { return (size_t)nparts * ntail * cap_tail; }
    size_t ids_per_buf() const { return set_elems() + tail_elems(); }
    size_t cur_per_buf() const { return (size_t)nparts * (nmain + ntail); }
    // the workspace: ids, cursors + the kernels' scratch, pass 2's prefix
    size_t ids_bytes() const { return nbuf * ids_per_buf() * sizeof(uint16_t); }
    size_t cursor_bytes() const {
        return (nbuf * cur_per_buf() + P1_SCRATCH_WG + (size_t)P1_SCRATCH_MAXWG * 1024) * sizeof(uint32_t);
    }
    size_t prefix_bytes() const { return nbuf * (cur_per_buf() + 1) * sizeof(uint64_t); }

    uint64_t spans() const { return (n + per_span * launch - 1) / (per_span * launch); }
    HistSpan span(uint64_t i) const {
        HistSpan sp;
        const uint64_t s0 = i * per_span * launch, ns = std::min(per_span * launch, n - s0);
        sp.r = {s0, ns, var ? blob_bytes : pipe ? blob_bytes - s0 * key_len : ns * key_len};
        sp.launches = (ns + launch - 1) / launch;
        sp.buf = pipe ? (uint32_t)(i & 1) : 0;
        sp.p2_grid = pipe && s0 + ns < n ? p2_cus : num_cus;  // (the last pass 2 gets the whole chip)
        return sp;
    }
    HistLaunch launch_of(const HistSpan &sp, uint64_t j) const {
        HistLaunch l;
        const uint64_t k0 = sp.r.k0 + j * launch, nk = std::min(launch, n - k0);
        // a window past the launch reads the next launch's bytes (the blob
        // goes on): only the blob's end limits the persistent kernel, so a
        // launch of whole tiles leaves no tail.  (A span's last launch keeps
        // its own length, as a call of one launch always had.)
        const bool to_end = pipe || j + 1 != sp.launches;
        l.r = {k0, nk, var ? blob_bytes : to_end ? blob_bytes - k0 * key_len : nk * key_len};
        if (k.kind == P1Kind::NONE) {
            l.tiles = p1_tiles(nk);
            return l;
        }
        // Whole tiles go to the persistent kernel; windowed: those whose
        // 16-byte windows stay inside the readable blob (a key's window ends
        // 16 - L bytes past it at most).  The rest (< 1 tile, windowed: < 2)
        // goes to the bounds-checked kernel.  (Fixed-length keys on
        // k_pass1_vare, over = 0: the blob term changes nothing while the
        // blob holds the launch's keys, as every caller's does.)
        const uint64_t tile = k.tile(), over = k.windowed() ? 16 - key_len : 0;
        l.tiles = var ? nk / tile : l.r.blob >= over ? std::min(nk / tile, (l.r.blob - over) / key_len / tile) : 0;
        if (l.tiles) {
            l.grid = (uint32_t)std::min<uint64_t>(l.tiles, grid_d13);
            // pipelined: pass 2 of the launch before runs beside this one on its own CUs
            if (pipe && k0 != 0) l.grid = std::max<uint32_t>(1, std::min<uint32_t>(l.grid, num_cus - p2_cus));
        }
        const uint64_t done = l.tiles * tile;
        if (done < nk) {
            l.tail = {k0 + done, nk - done, var ? blob_bytes : (nk - done) * key_len};
            l.tail_tiles = p1_tiles(nk - done);
        }
        return l;
    }
};

// Bins of a binned kernel: the smallest bin_shift with ceil(m >> shift) <=
// maxp, so a tile fills each LDS bin to tile/P on average while a bin holds
// bin_ids/P >= 2.25x that (>= 8 sigma).
inline bool binned_layout(HistPlan &p, uint32_t maxp, uint32_t bin_ids, uint64_t m) {
    uint32_t shift = 0;
    while (shift <= (uint32_t)PART_SHIFT && ((m + (1ULL << shift) - 1) >> shift) > (uint64_t)maxp) ++shift;
    if (shift > (uint32_t)PART_SHIFT) return false;
    p.bin_shift = shift;
    p.nparts = (uint32_t)((m + (1ULL << shift) - 1) >> shift);
    p.capb = std::min<uint32_t>((bin_ids / p.nparts) & ~7u, (uint32_t)p.k.tile() + 8);
    return true;
}

// The one place that chooses the mode and pass 1's kernel (two-pass path, m
// buckets), with the kernel's bins:
//  * 13-byte keys: k_pass1_d13e with its cursor atomic as a buffer atomic
//    (VARIANT 13, the default; BSDB_D13_VARIANT=0: as a flat atomic); above
//    its 288 bins (m > 288 * 32768), or with BSDB_D13_VARIANT=2, the round-1
//    sort kernel k_pass1_d13 (up to 1024 partitions).  Every other value of
//    the variable means 0.
//  * 8 / 12 / 16-byte keys: k_pass1_d13e, a key's 16-byte window from its
//    aligned start; BSDB_NO_FIXED_WINDOW=1 sends them to the var-len kernel
//    instead (A/B switch for measurements).
//  * variable-length keys and every other fixed length up to 32 B (as k * L
//    offsets): k_pass1_vare.  (Fixed keys over 32 B: a 128-key group would
//    overflow its LDS stage.)
//  * none: a frontend other than 0, fixed keys of 0 or over 32 B, more bins
//    than the kernel holds.
// seed0: the kernels with the seed folded at compile time (BSDB_NO_SEED0: A/B
// switch for measurements).
inline HistPlan pass1_select(const HistIn &in) {
    HistPlan p;
    p.nparts = (uint32_t)((in.m + PART_BUCKETS - 1) / PART_BUCKETS);
    p.bin_shift = (uint32_t)PART_SHIFT;
    // (mode 3 on a set the fused kernel does not take: the two-pass path)
    p.atomic_mode = in.hist_mode == 2 || p.nparts > (uint32_t)MAX_PARTS;
    if (p.atomic_mode || in.frontend != 0) return p;
    const bool var = in.var, seed0 = in.seed0 && !in.no_seed0;
    const uint32_t key_len = in.key_len;
    const Pass1Choice none{}, sort{P1Kind::D13, 13, false, 0};
    const bool sort_fits = p.nparts <= 1024;
    const bool k13 = !var && key_len == 13;
    const bool window = k13 || (!var && (key_len == 8 || key_len == 12 || key_len == 16) && !in.no_fixed_window);
    if (window) {
        if (k13 && in.d13_variant == 2) {
            p.k = sort_fits ? sort : none;
            return p;
        }
        p.k = {P1Kind::D13E, key_len, seed0, k13 && in.d13_variant == 13 ? 13 : 0};
        if (!binned_layout(p, D13E_MAXP, D13E_BIN_IDS, in.m)) p.k = k13 && sort_fits ? sort : none;
        return p;
    }
    if (!var && (key_len == 0 || key_len > 32)) return p;
    p.k = {P1Kind::VARE, var ? 0 : key_len, seed0, 0};
    if (!binned_layout(p, VARE_MAXP, VARE_BIN_IDS, in.m)) p.k = none;
    return p;
}

// Region capacities of a span: `span` keys in launches of `launch` keys, all
// appending to one region set.  Every launch deals its tiles round-robin over
// the copies from copy 0 on, so a copy takes at most ceil(tiles / copies)
// tiles of each launch (launches of 8k + 1 tiles all give the odd tile to
// copy 0).  cap = a bin's expected share of the keys of those tiles plus 2 %,
// 8 sigma and two tiles of slack, plus the pads of padded runs:
//  * k_pass1_d13e pads once per workgroup per bin per launch (at most 7 ids,
//    in the copy of the workgroup's last tile; the last tiles of a launch's G
//    workgroups are G consecutive tiles, so at most ceil(G / copies) of them
//    end in one copy): 7 * (G / copies + 1) * launches;
//  * k_pass1_vare pads every tile's run: 7 per tile of the copy.
// A fill beyond cap raises the overflow flag and the span is recounted with
// direct atomics.
inline void size_regions(const HistIn &in, HistPlan &p, uint64_t span, uint64_t launch) {
    const bool d13 = p.k.kind != P1Kind::NONE, binned = p.k.binned();
    const double frac = std::min(1.0, (double)(1ULL << p.bin_shift) / (double)in.m);
    p.nmain = binned ? (uint32_t)in.d13_copies : NCOPY;
    launch = std::min(launch, span);
    const uint64_t tile = d13 ? p.k.tile() : (uint64_t)P1_TILE;
    const uint64_t full = span / launch, rest = span % launch;  // whole launches, keys of a shorter last one
    const uint64_t launches = full + (rest ? 1 : 0);
    auto copy_tiles = [&](uint64_t keys) { return ((keys + tile - 1) / tile + p.nmain - 1) / p.nmain; };
    const uint64_t tiles_per_copy = full * copy_tiles(launch) + copy_tiles(rest);
    p.keys_per_copy = std::min(span, tiles_per_copy * tile);
    const double e = (double)p.keys_per_copy * frac;
    double pads = 0;
    p.ntail = 0;
    p.cap_tail = 0;
    p.grid_d13 = 0;
    if (d13) {
        const int per_cu = std::min(std::max(in.wg_per_cu, 1), 2048 / p.k.nt());  // at most 32 waves per CU
        const uint64_t tiles = (launch + tile - 1) / tile;
        p.grid_d13 = (uint32_t)std::min<uint64_t>(tiles, (uint64_t)in.num_cus * per_cu);
        // measurement aid: fewer persistent workgroups (BSDB_D13_GRID, e.g. CUs left for other work)
        p.grid_d13 = (uint32_t)std::max<int64_t>(1, std::min<int64_t>(p.grid_d13, in.d13_grid));
        if (binned && p.k.windowed())
            pads = 7.0 * (p.grid_d13 / p.nmain + 1) * (double)launches;
        else if (binned)
            pads = 7.0 * (double)tiles_per_copy;
        // the tail (< 2 tiles of the persistent kernel) goes to k_pass1 in
        // blocks of P1_TILE keys, one region each
        p.ntail = NCOPY;
        p.cap_tail = round64(std::max<uint64_t>(P1_TILE, tile) + 64);
    }
    p.cap = round64(e * 1.02 + 8.0 * std::sqrt(e) + pads + 2 * P1_TILE + 64);
}

// Completes pass1_select's plan of a two-pass call: launch length, launches
// per span, region sizes, buffers.  (in.wg_per_cu: of the kernel chosen.)
inline void hist_size(const HistIn &in, HistPlan &p) {
    p.var = in.var;
    p.key_len = in.key_len;
    p.n = in.n;
    p.blob_bytes = in.blob_bytes;
    p.num_cus = (uint32_t)in.num_cus;
    if (p.atomic_mode) return;
    const uint64_t n = in.n, tile = p.k.tile();
    const bool d13 = p.k.kind != P1Kind::NONE;
    uint64_t chunk = in.chunk_keys ? in.chunk_keys : DEFAULT_CHUNK_KEYS;
    chunk = std::max<uint64_t>(P1_TILE, chunk / P1_TILE * P1_TILE);
    chunk = std::min<uint64_t>(chunk, p1_tiles(n) * P1_TILE);
    const bool pipe_pl = in.pipe && p.k.windowed() && p.k.binned();
    if (pipe_pl && !in.chunk_keys) {
        // equal chunks of whole tiles: pass 2 of each beside pass 1 of the next
        const uint64_t nch = in.pipe_chunks ? in.pipe_chunks : 8;
        chunk = std::max<uint64_t>(tile, ((n + nch - 1) / nch + tile - 1) / tile * tile);
    }
    // several launches of a persistent kernel: whole tiles of it each, so
    // that only a span's last launch leaves keys to the tail kernel
    auto whole_tiles = [&](uint64_t ch) { return d13 && !pipe_pl && ch < n && ch >= tile ? ch / tile * tile : ch; };
    chunk = whole_tiles(chunk);
    // A span: J consecutive pass-1 launches of chunk keys, all appending to
    // ONE region set (the kernels reserve their runs with a cursor atomic per
    // (copy, bin) and never assume a cursor starts at 0), then ONE pass 2
    // (its workgroups flush their LDS tables once per span, not once per
    // launch).  cap is sized for the span's keys, so pass 2 and the workspace
    // see the same layout whatever the launch length.  The whole call is one
    // span unless span_max (launches per span at most) or the rules below
    // shorten it.  A persistent kernel's launches must be whole tiles of it:
    // every launch but the span's last then runs entirely in that kernel, and
    // the span has one set of tail regions.  (The one-tile-per-workgroup
    // kernels have no tail: any launch length, a multiple of P1_TILE.)
    uint64_t J = 1;
    if (!pipe_pl && n > chunk && (!d13 || chunk % tile == 0)) {
        J = (n + chunk - 1) / chunk;
        if (in.span_max) J = std::min<uint64_t>(J, in.span_max);
    }
    // The id buffers take at most half of the device memory left (workspace
    // included); the kernels address one region copy (P segments of cap ids)
    // with 32-bit offsets and count a segment's fill in 32 bits.  These bound
    // the SPAN: it is halved until they hold, and only a span of one launch
    // halves the launch.
    const size_t budget = (in.free_bytes + in.ids_bytes) / 2 / (pipe_pl ? 2 : 1);
    size_regions(in, p, std::min(n, J * chunk), chunk);
    while (p.ids_per_buf() * sizeof(uint16_t) > budget || (uint64_t)p.nparts * p.cap >= (1ULL << 32) ||
           p.keys_per_copy >= (1ULL << 32)) {
        if (J > 1)
            J = (J + 1) / 2;
        else if (chunk > 2 * P1_TILE)
            chunk = whole_tiles(std::max<uint64_t>(P1_TILE, chunk / 2 / P1_TILE * P1_TILE));
        else {
            p.bottomed_out = true;
            break;
        }
        size_regions(in, p, std::min(n, J * chunk), chunk);
    }
    p.launch = chunk;
    p.per_span = J;
    // Pass 2 of chunk i overlapped with pass 1 of chunk i + 1 (13-byte
    // windowed keys, several chunks): two id buffers; pass 1 on the caller's
    // stream over all CUs but the ones pass 2 keeps (its workgroups hold 128
    // KiB of LDS, pass 1's 146 KiB: one per CU each, so the two launches
    // split the chip); pass 2 on the context's second stream.  The first
    // pass 1 and the last pass 2 get the whole chip.
    p.pipe = pipe_pl && n > chunk;
    p.nbuf = p.pipe ? 2 : 1;
    if (p.pipe) {
        const uint32_t k = in.pipe_cus ? in.pipe_cus : (uint32_t)in.num_cus / 8;  // 4 per XCD
        p.p2_cus = std::max<uint32_t>(1, std::min<uint32_t>(k, (uint32_t)in.num_cus / 2));
    }
}

}  // namespace bsdb
