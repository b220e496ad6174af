// capi_hist.hip -- the histogram and hash stages: pass-1 dispatch, the
// single-pass kernel's launch, and histogram_impl, which enqueues what
// hist_plan.hpp decides.  Included by bsdb_capi.hip (inside its namespace).

// The key set of a launch (the epilogue's fields are the caller's).
P1Args key_args(const uint8_t *keys, const uint64_t *offsets, uint64_t blob_bytes, uint32_t key_len, uint64_t n,
                uint64_t seed) {
    P1Args a{};
    a.keys = keys;
    a.offsets = offsets;
    a.blob_bytes = blob_bytes;
    a.key_len = key_len;
    a.n = n;
    a.seed = seed;
    return a;
}

// Keys [k0, k0 + nk) of a's: keys or offsets, and signatures when set,
// shifted; blob: the bytes readable from key k0 on (fixed layouts).
P1Args slice(const P1Args &a0, bool var, uint64_t k0, uint64_t nk, uint64_t blob) {
    P1Args a = a0;
    a.n = nk;
    if (var) {
        a.offsets = a0.offsets + k0;
    } else {
        a.keys = a0.keys + k0 * a0.key_len;
        a.blob_bytes = blob;
    }
    if (a.sig) a.sig = a0.sig + 2 * k0;
    return a;
}
P1Args slice(const P1Args &a, bool var, const KeyRange &r) { return slice(a, var, r.k0, r.nk, r.blob); }

// ---- pass-1 dispatch over (source layout, epilogue) ------------------------
// One-tile-per-workgroup launches: tiles * 512 work-items must stay below 2^32
// (a dispatch packet's grid size is 32-bit), so callers split larger key sets.
constexpr uint64_t MAX_TILES_PER_LAUNCH = (1ULL << 32) / P1_THREADS - 1;

template <int EPI>
void launch_pass1(const P1Args &a, bool var, uint32_t key_len, uint64_t tiles, hipStream_t s, int frontend) {
    if (tiles > MAX_TILES_PER_LAUNCH) {
        // split into launches of whole tiles
        for (uint64_t t0 = 0; t0 < tiles; t0 += MAX_TILES_PER_LAUNCH) {
            const uint64_t nt = std::min(MAX_TILES_PER_LAUNCH, tiles - t0), k0 = t0 * P1_TILE;
            launch_pass1<EPI>(slice(a, var, k0, std::min<uint64_t>(a.n - k0, nt * P1_TILE), a.blob_bytes - k0 * key_len),
                              var, key_len, nt, s, frontend);
        }
        return;
    }
    const dim3 g((uint32_t)tiles), b(P1_THREADS);
    if (var && frontend == 2) {
        k_pass1<SRC_VAR, EPI, 1, 0><<<g, b, 0, s>>>(a);
    } else if (var) {
        k_pass1<SRC_VARSTAGED, EPI, 1, 0><<<g, b, 0, s>>>(a);
    } else if (key_len == 13 && frontend != 1) {
        k_pass1<SRC_DIRECT13, EPI, 4, 13><<<g, b, 0, s>>>(a);
    } else if (key_len == 13) {
        k_pass1<SRC_STAGED13, EPI, 4, 13><<<g, b, 0, s>>>(a);
    } else if (key_len >= 1 && key_len <= 13) {
        k_pass1<SRC_STAGED, EPI, 4, 0><<<g, b, 0, s>>>(a);
    } else if (key_len >= 14 && key_len <= 26) {
        k_pass1<SRC_STAGED, EPI, 2, 0><<<g, b, 0, s>>>(a);
    } else if (key_len >= 27 && key_len <= 52) {
        k_pass1<SRC_STAGED, EPI, 1, 0><<<g, b, 0, s>>>(a);
    } else {
        k_pass1<SRC_FIXED_DIRECT, EPI, 1, 0><<<g, b, 0, s>>>(a);
    }
}

using D13Kernel = void (*)(P1Args, uint64_t);

// The kernel of a choice (pass1_select, hist_plan.hpp); nullptr: none.
D13Kernel pass1_kernel(const Pass1Choice &k) {
    const bool seed0 = k.seed0;
    switch (k.kind) {
        case P1Kind::D13: return k_pass1_d13<D13_NT>;
        case P1Kind::D13E:
            return k.key_len == 8    ? (seed0 ? k_pass1_d13e<0, true, 8> : k_pass1_d13e<0, false, 8>)
                   : k.key_len == 12 ? (seed0 ? k_pass1_d13e<0, true, 12> : k_pass1_d13e<0, false, 12>)
                   : k.key_len == 16 ? (seed0 ? k_pass1_d13e<0, true, 16> : k_pass1_d13e<0, false, 16>)
                   : k.variant == 13 ? (seed0 ? k_pass1_d13e<13, true> : k_pass1_d13e<13>)
                                     : (seed0 ? k_pass1_d13e<0, true> : k_pass1_d13e<0>);
        case P1Kind::VARE:
            return k.key_len == 0 ? (seed0 ? k_pass1_vare<false, true> : k_pass1_vare<false>)
                                  : (seed0 ? k_pass1_vare<true, true> : k_pass1_vare<true>);
        case P1Kind::NONE: break;
    }
    return nullptr;
}

// The single-pass kernel (fused_kernels.hip) over the whole super-tiles of a
// 13-byte key set: *done = the keys it covers (a multiple of 256 * 16384);
// 0 when the set does not qualify.  Enqueue only.
constexpr uint64_t FU_MIN_SUPER = 4;  // super-tiles per workgroup, at least

int fused13_impl(bsdb_ctx *c, const uint8_t *keys, uint64_t blob_bytes, uint64_t n, uint64_t seed, uint64_t m,
                 uint32_t *counts, hipStream_t s, uint64_t *done) {
    *done = 0;
    const uint64_t per = (uint64_t)FU_OWNERS * FU_TILE;
    if (c->num_cus != FU_OWNERS || m == 0 || m > (uint64_t)FU_OWNERS * (FU_TCAP - 2)) return BSDB_OK;
    // a key's 16-byte window ends 3 bytes past it: whole super-tiles whose
    // windows stay inside the blob
    if (blob_bytes < 3) return BSDB_OK;
    const uint64_t nsuper = std::min(n / per, (blob_bytes - 3) / 13 / per);
    if (nsuper < FU_MIN_SUPER) return BSDB_OK;
    // the owner tables count in u16: keep the mean bucket count far below 2^16
    // (a wrap is detected and recounted, but costs the whole launch)
    if (n / m > 16384) return BSDB_OK;
    static int per_cu = -1;
    if (per_cu < 0 && hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_hist13_fused<true>, FU_NT, 0) != hipSuccess)
        per_cu = 0;
    if (per_cu < 1) return BSDB_OK;  // every workgroup must be resident
    const size_t sync_bytes = FU_SYNC_U64 * sizeof(uint64_t);
    const size_t ring_bytes = (size_t)FU_SLOTS * FU_SLOT_BYTES;
    int rc = c->fu_ring.grow(ring_bytes + sync_bytes);
    if (rc) return rc;
    FusedArgs fa{};
    fa.keys = keys;
    fa.nsuper = nsuper;
    fa.seed = seed;
    fa.mult = (uint32_t)(2 * m);
    fa.m = (uint32_t)m;
    fa.ring = c->fu_ring.as<uint8_t>();
    fa.sync = (uint64_t *)(c->fu_ring.as<uint8_t>() + ring_bytes);
    fa.overflow = c->overflow.as<uint32_t>();
    fa.counts = counts;
    HIP_OK(hipMemsetAsync(fa.sync, 0, sync_bytes, s));
    HIP_OK(hipMemsetAsync(c->overflow.p, 0, sizeof(uint32_t), s));
    ++c->fu_launches;
    {
        ProfScope ps(c, s, 0, nsuper * per);
        if (seed == 0 && !getenv("BSDB_NO_SEED0"))
            k_hist13_fused<true><<<FU_OWNERS, FU_NT, 0, s>>>(fa);
        else
            k_hist13_fused<false><<<FU_OWNERS, FU_NT, 0, s>>>(fa);
    }
    // an overflow anywhere (adversarial sets): nothing was added; recount
    P1Args af = key_args(keys, nullptr, blob_bytes, 13, nsuper * per, seed);
    af.multiplier = 2 * m;
    af.counts = counts;
    af.overflow = c->overflow.as<uint32_t>();
    k_overflow_fallback<SRC_FIXED_DIRECT, 0><<<1024, P1_THREADS, 0, s>>>(af);
    if ((rc = launch_status())) return rc;
    *done = nsuper * per;
    return BSDB_OK;
}

bool fused_wanted(const bsdb_ctx *c) {
    if (c->hist_mode == 3) return true;
    if (c->hist_mode != 0) return false;
    if (c->fused >= 0) return c->fused == 1;
    return false;
}

// A call's own options: keys per pass-1 launch and launches per span at most
// (0: the default, no limit).  The public entry points pass the context's.
struct HistOpts {
    uint64_t chunk_keys, span_max;
};
HistOpts hist_opts(const bsdb_ctx *c) { return {c->chunk_keys, c->span_max}; }

// The plan's inputs but the key set and the runtime's answers: the context's
// knobs, the call's options and the environment, read at every call.
HistIn hist_knobs(const bsdb_ctx *c, HistOpts opts) {
    HistIn in;
    in.hist_mode = c->hist_mode, in.frontend = c->frontend, in.d13_variant = c->d13_variant, in.d13_copies = c->d13_copies;
    in.chunk_keys = opts.chunk_keys, in.span_max = opts.span_max;
    in.pipe = c->pipe == 1, in.pipe_chunks = c->pipe_chunks, in.pipe_cus = c->pipe_cus;
    in.no_fixed_window = getenv("BSDB_NO_FIXED_WINDOW") != nullptr;
    in.no_seed0 = getenv("BSDB_NO_SEED0") != nullptr;
    if (const char *v = getenv("BSDB_D13_GRID")) in.d13_grid = atoll(v);
    in.num_cus = c->num_cus;
    return in;
}

// The pipelined mode's second stream and events; pass 2 (on *s2) starts after
// the caller's earlier work on s.
int pipe_begin(bsdb_ctx *c, hipStream_t s, hipStream_t *s2) {
    if (!c->p2_stream && hipStreamCreateWithFlags(&c->p2_stream, hipStreamNonBlocking) != hipSuccess) return BSDB_EIO;
    for (auto &e : c->pipe_ev)
        if (!e && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return BSDB_EIO;
    *s2 = c->p2_stream;
    HIP_OK(hipEventRecord(c->pipe_ev[4], s));  // the caller's earlier work
    HIP_OK(hipStreamWaitEvent(*s2, c->pipe_ev[4], 0));
    return BSDB_OK;
}

// The plan's region layout as pass 1 (main regions) and pass 2 take it.
void region_args(P1Args &a, const HistPlan &p) {
    a.cap = p.cap;
    a.nparts = p.nparts;
    a.nregions = p.nmain;
    a.region0 = 0;
    a.ncopy = p.nmain;
    a.bin_shift = p.bin_shift;
    a.capb = p.capb;
}
P2Layout pass2_layout(const HistPlan &p, uint64_t m, uint32_t *counts) {
    P2Layout L{};
    L.cap = p.cap;
    L.cap_tail = p.cap_tail;
    L.nparts = p.nparts;
    L.nmain = p.nmain;
    L.ntail = p.ntail;
    L.bshift = PART_SHIFT - p.bin_shift;
    L.num_buckets = m;
    L.counts = counts;
    return L;
}

// Fills the plan's inputs, plans (hist_plan.hpp: every number below is the
// plan's), grows the workspace, and enqueues the plan's spans: per span the
// cursor memsets, its pass-1 launches (persistent kernel + tail, or the
// one-tile-per-workgroup kernels), one pass 2 and the overflow fallback.
int histogram_impl(bsdb_ctx *c, const uint8_t *keys, const uint64_t *offsets, uint64_t blob_bytes,
                   uint32_t key_len, uint64_t n, uint64_t seed, uint64_t m, uint32_t *counts, HistOpts opts,
                   hipStream_t s) {
    if (n == 0) return BSDB_OK;
    const bool var = offsets != nullptr;
    if (!var && key_len == 13 && fused_wanted(c)) {
        uint64_t done = 0;
        const int rc = fused13_impl(c, keys, blob_bytes, n, seed, m, counts, s, &done);
        if (rc) return rc;
        if (done) return histogram_impl(c, keys + done * 13, nullptr, blob_bytes - done * 13, 13, n - done, seed, m,
                                        counts, opts, s);  // the rest (< one super-tile round): two-pass
    }
    HistIn in = hist_knobs(c, opts);
    in.var = var, in.key_len = key_len, in.n = n, in.m = m, in.blob_bytes = blob_bytes, in.seed0 = seed == 0;
    HistPlan p = pass1_select(in);
    P1Args a = key_args(keys, offsets, blob_bytes, key_len, n, seed);
    a.multiplier = 2 * m;
    a.counts = counts;
    if (p.atomic_mode) {
        ProfScope ps(c, s, 0, n);
        launch_pass1<EPI_ATOMIC>(a, var, key_len, p1_tiles(n), s, c->frontend);
        return launch_status();
    }
    const D13Kernel kern = pass1_kernel(p.k);
    if (kern && hipOccupancyMaxActiveBlocksPerMultiprocessor(&in.wg_per_cu, kern, p.k.nt(), 0) != hipSuccess) in.wg_per_cu = 0;
    size_t total_b = 0;
    if (hipMemGetInfo(&in.free_bytes, &total_b) != hipSuccess) in.free_bytes = 0;
    in.ids_bytes = c->ids.bytes;
    hist_size(in, p);
    int rc;
    if ((rc = c->ids.grow(p.ids_bytes())) || (rc = c->cursor.grow(p.cursor_bytes())) ||
        (rc = c->p2_pref.grow(p.prefix_bytes())))
        return rc;
    // pipelined: pass 1 on the caller's stream, pass 2 on the context's second
    hipStream_t s2 = s;
    if (p.pipe && (rc = pipe_begin(c, s, &s2))) return rc;
    a.scratch = c->cursor.as<uint32_t>() + p.nbuf * p.cur_per_buf();
    region_args(a, p);
    P2Layout L = pass2_layout(p, m, counts);
    for (uint64_t i = 0, nspans = p.spans(); i < nspans; ++i) {
        const HistSpan sp = p.span(i);
        const uint32_t b = sp.buf;
        // buffer b's ids, cursors, pass-2 plan and overflow flag
        L.ids = a.ids = c->ids.as<uint16_t>() + b * p.ids_per_buf();
        L.cursor = a.cursor = c->cursor.as<uint32_t>() + b * p.cur_per_buf();
        L.overflow = a.overflow = c->overflow.as<uint32_t>() + 4 * b;
        uint64_t *pref = c->p2_pref.as<uint64_t>() + b * (p.cur_per_buf() + 1);
        if (p.pipe && i >= 2) HIP_OK(hipStreamWaitEvent(s, c->pipe_ev[2 + b], 0));  // pass 2 of chunk i - 2 read buffer b
        HIP_OK(hipMemsetAsync(a.cursor, 0, sizeof(uint32_t) * p.cur_per_buf(), s));
        HIP_OK(hipMemsetAsync(a.overflow, 0, sizeof(uint32_t), s));
        for (uint64_t j = 0; j < sp.launches; ++j) {
            // launch j appends to the span's regions (a.ids, a.cursor)
            const HistLaunch l = p.launch_of(sp, j);
            const P1Args ac = slice(a, var, l.r);
            ProfScope ps(c, s, 0, l.r.nk);
            // the tail: to the bounds-checked kernel, in the tail regions
            // (they follow the span's main regions)
            auto tail = [&] {
                P1Args at = slice(a, var, l.tail);
                at.ids = a.ids + p.set_elems();
                at.cursor = a.cursor + p.nmain * p.nparts;
                at.cap = p.cap_tail;
                at.nregions = p.ntail;
                if (var)
                    k_pass1<SRC_VAR, EPI_PARTITION, 1, 0><<<(uint32_t)l.tail_tiles, P1_THREADS, 0, s>>>(at);
                else
                    launch_pass1<EPI_PARTITION>(at, false, key_len, l.tail_tiles, s, 0);
            };
            if (!kern)
                launch_pass1<EPI_PARTITION>(ac, var, key_len, l.tiles, s, c->frontend);
            else if (l.tiles)
                kern<<<l.grid, p.k.nt(), 0, s>>>(ac, l.tiles);
            if (l.tail.nk) tail();
        }
        if (p.pipe) {
            HIP_OK(hipEventRecord(c->pipe_ev[b], s));  // pass 1 of chunk i done
            HIP_OK(hipStreamWaitEvent(s2, c->pipe_ev[b], 0));
        }
        {
            ProfScope ps(c, s2, 1, sp.r.nk);
            k_pass2_plan<<<1, SCAN_THREADS, 0, s2>>>(L, pref);
            k_pass2b<<<sp.p2_grid, P2_THREADS, 0, s2>>>(L, pref);
        }
        // an overflow anywhere in the span: pass 2 skipped all of it, and the
        // whole span is recounted
        const P1Args as = slice(a, var, sp.r);
        if (var) {
            k_overflow_fallback<SRC_VAR, 0><<<1024, P1_THREADS, 0, s2>>>(as);
        } else {
            k_overflow_fallback<SRC_FIXED_DIRECT, 0><<<1024, P1_THREADS, 0, s2>>>(as);
        }
        if (p.pipe) HIP_OK(hipEventRecord(c->pipe_ev[2 + b], s2));  // buffer b free again
        if ((rc = launch_status())) return rc;
    }
    if (p.pipe) {
        // the caller's stream continues after the last pass 2
        HIP_OK(hipEventRecord(c->pipe_ev[5], s2));
        HIP_OK(hipStreamWaitEvent(s, c->pipe_ev[5], 0));
    }
    return BSDB_OK;
}

int hash_impl(bsdb_ctx *c, const uint8_t *keys, const uint64_t *offsets, uint64_t blob_bytes, uint32_t key_len,
              uint64_t n, uint64_t seed, uint64_t *sig, hipStream_t s) {
    if (n == 0) return BSDB_OK;
    P1Args a = key_args(keys, offsets, blob_bytes, key_len, n, seed);
    a.sig = sig;
    launch_pass1<EPI_SIG>(a, offsets != nullptr, key_len, p1_tiles(n), s, c->frontend);
    return launch_status();
}
