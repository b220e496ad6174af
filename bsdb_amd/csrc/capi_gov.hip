// capi_gov.hip -- the GOV build on the device (A5, A6, A8, A11), included by
// bsdb_capi.hip inside its extern "C" block.  gov_plan.hpp decides the class,
// every size and every grid; the three steps here (gov_group, gov_solve,
// gov_finish) grow the workspace and enqueue what it says.

uint64_t bsdb_values_words(uint64_t n) { return gov_values_words(n); }

extern "C++" {

// lds_pad of one solver workgroup per CU (BSDB_GOV_PER_CU=1): its subtraction does not wrap
static_assert(GS_PER_CU < 2 || sizeof(SolveLds) <= CU_LDS_BYTES / 2 + 1024, "gov_solve_plan: lds_pad for per_cu = 1");

// The environment of one build, read once.
static GovKnobs gov_knobs() {
    GovKnobs k;
    k.per_cu = gov_parse_per_cu(getenv("BSDB_GOV_ONE_PER_CU") != nullptr, getenv("BSDB_GOV_PER_CU"));
    k.fvs_max = gov_parse_fvs_max(getenv("BSDB_GOV_FVS_MAX"), getenv("BSDB_GOV_PICK_EXACT") != nullptr);
    k.spec = gov_parse_spec(getenv("BSDB_GOV_SPEC"));
    k.profile = getenv("BSDB_GOV_PROFILE") != nullptr;
    return k;
}

constexpr GovSizes gov_sizes() {
    return {sizeof(SolveLds), solve_scratch_words<SolveLds>(), solve_scratch_words<SolveMid>(), big_slab_bytes()};
}

static void print_gov_profile(const std::vector<uint64_t> &h, uint32_t solve_grid, uint64_t m) {
    const char *names[] = {"edges", "peel", "greedy", "bfs", "tarjan", "singletons", "dense", "back",
                           "store", "n_seeds", "n_bfs", "n_bfs_pops", "n_dense_rows", "n_dense_max",
                           "n_core", "n_blocks", "n_rows_in_blocks_over_440", "n_scc_sweeps",
                           "n_small_scc_fallbacks", "fvs_select", "fvs_forms", "fvs_gauss_jordan",
                           "n_fail_degenerate", "n_fail_orient", "n_fail_inconsistent", "failed_attempt_cycles",
                           "bfs_flip", "n_bfs_iters", "n_flip_steps", "n_sel_batches", "n_sel_picks",
                           "sel_pick_cycles", "sel_prep_cycles", "n_singular_solved", "n_null_vectors", "n_speculative_lost",
                           "n_fvs_blocks", "n_form_levels", "n_heavy", "gj_columns", "gj_barrier_wait_cycles",
                           "unused", "tarjan_prep", "tarjan_sweeps", "tarjan_compact",
                           "gj_leader_cycles", "gj_follower_cycles", "gj_slot_columns", "gj_leader_columns",
                           "gj_trailing_cycles", "gj_panels"};
    static_assert(sizeof(names) / sizeof(names[0]) == GP_N, "a name per phase counter");
    std::vector<double> tot(GP_N, 0.0);
    for (uint32_t w = 0; w < solve_grid; ++w)
        for (int k = 0; k < GP_N; ++k) {
            const double v = (double)h[(size_t)w * GP_N + k];
            tot[k] = k == GP_N_DENSE_MAX ? std::max(tot[k], v) : tot[k] + v;
        }
    fprintf(stderr, "[gov-profile] m=%llu grid=%u", (unsigned long long)m, solve_grid);
    for (int k = 0; k < GP_N; ++k)
        fprintf(stderr, " %s=%.4g", names[k], k == GP_N_DENSE_MAX ? tot[k] : tot[k] / ((k < GP_N_SEEDS || (k >= GP_FVS_SEL && k <= GP_FVS_GJ) || k == GP_FAILED_CYCLES || k == GP_BFS_FLIP || k == GP_SEL_PICK_CYCLES || k == GP_SEL_PREP_CYCLES || (k >= GP_TJ_PREP && k <= GP_TJ_COMPACT)) ? solve_grid : 1));
    fprintf(stderr, "  (cycles: mean per workgroup; counts: totals)\n");
}

struct DevFree {
    void operator()(void *p) const { if (p) (void)hipFree(p); }
};

// Where a GOV build takes its keys from: n_local signatures of the range
// (sig != nullptr), or the keys themselves (fixed length or a var-len blob),
// re-hashed and filtered to the range's buckets (the sequential range builds
// of bsdb_dev_mph_build_index_passes: no signature array for the whole set).
struct GovSrc {
    const uint64_t *sig = nullptr;
    uint64_t n = 0;  // signatures, or keys
    const uint8_t *keys = nullptr;
    const uint64_t *off = nullptr;
    uint64_t blob_bytes = 0;
    uint32_t key_len = 0;
    // (key sources) every bucket's count over the whole key set, when known:
    // a range build then takes its counts from here instead of re-hashing
    const uint32_t *counts_all = nullptr;
};

// A13 fused into the solve: slot r - idx_lo of index_out gets key p's
// byte-reversed address (addr[p] or addr_base + addr_stride * p).
struct GovIndexOut {
    uint64_t *index = nullptr;
    uint64_t idx_lo = 0;
    const uint64_t *addr = nullptr;
    uint64_t addr_base = 0, addr_stride = 0;
    // (optional) called once the range's key count is known, returns the
    // slots' buffer (at least that many), nullptr when it cannot
    std::function<uint64_t *(uint64_t n_local)> slots;
};

template <int MODE>
static void launch_sel(const GovSrc &src, SelArgs &a, uint32_t grid, hipStream_t s) {
    if (!src.off && src.key_len == 13) k_sel<MODE, 0><<<grid, 256, 0, s>>>(a);
    else if (!src.off) k_sel<MODE, 1><<<grid, 256, 0, s>>>(a);
    else k_sel<MODE, 2><<<grid, 256, 0, s>>>(a);
}

// One build: its arguments, and what each step leaves for the next.
struct GovBuild {
    bsdb_ctx *c;
    const GovSrc &src;
    uint64_t n_global, b_lo, b_hi, e_lo;
    uint32_t width;
    uint64_t *d_E, *d_values, *d_sigbits;
    int64_t *d_rank;
    GovIndexOut ixo;
    hipStream_t s;
    bool full;
    uint64_t *n_found;
    GovKnobs knobs;
    GovGroupPlan g;
    GovSolvePlan sp;      // (from gov_group on)
    uint64_t n_local = 0;
    uint64_t *pay = nullptr;
    // the grouping alone, with positions (the duplicate finder, capi_dup.hip):
    // no solver scratch is reserved
    bool group_only = false;
    uint64_t *Eb() const { return d_E + b_lo; }
    uint64_t *sorted() const { return c->g_sorted.as<uint64_t>(); }
    uint32_t *status() const { return c->g_status.as<uint32_t>(); }
};

// The counting launches of the build's class: counts[0..nb) of the range's buckets.
static int gov_count(GovBuild &b, SelArgs &sel, uint16_t *mid_cw) {
    const GovSrc &src = b.src;
    const GovGroupPlan &g = b.g;
    hipStream_t s = b.s;
    const uint64_t nb = g.nb;
    const uint32_t b_lo = (uint32_t)b.b_lo, nb32 = (uint32_t)nb;
    uint32_t *counts = b.c->g_counts.as<uint32_t>();
    switch (g.cls) {
        case GovClass::COPY_COUNTS:
            HIP_OK(hipMemcpyAsync(counts, src.counts_all + b.b_lo, nb * 4, hipMemcpyDeviceToDevice, s));
            break;
        case GovClass::SEL: launch_sel<0>(src, sel, g.count_grid, s); break;
        case GovClass::SMALL:
            k_bucket_count_small<<<g.count_grid, 256, 0, s>>>(src.sig, src.n, g.mult, b_lo, nb32, counts);
            break;
        case GovClass::MID:
            k_bucket_count_mid<<<g.count_grid, MID_THREADS, 0, s>>>(src.sig, src.n, g.mult, b_lo, nb32, mid_cw, counts + nb);
            k_mid_colsum<<<g.col_grid, 256, 0, s>>>(mid_cw, g.mid_g, nb32, counts);
            k_bucket_count_redo<<<1, 256, 0, s>>>(src.sig, src.n, g.mult, b_lo, nb32, counts, counts + nb);
            break;
        case GovClass::LARGE: k_bucket_count<<<g.count_grid, 256, 0, s>>>(src.sig, src.n, g.mult, b_lo, counts); break;
        case GovClass::NONE: break;
    }
    return BSDB_OK;
}

// A5, A6: the range's keys counted per bucket, the offsets Eb[0..nb], the
// signatures scattered to their buckets, each bucket sorted, the oversized
// buckets listed.  With a key source the range's key count is read back here
// (the first host synchronisation).
static int gov_group(GovBuild &b) {
    bsdb_ctx *c = b.c;
    const GovSrc &src = b.src;
    const GovGroupPlan &g = b.g;
    hipStream_t s = b.s;
    const uint64_t nb = g.nb, e_lo = b.e_lo;
    const uint32_t b_lo = (uint32_t)b.b_lo, nb32 = (uint32_t)nb;
    int rc;
    if ((rc = c->g_counts.grow(g.counts_bytes)) || (rc = c->g_cursor.grow(g.cursor_bytes)) ||
        (rc = c->g_status.grow(g.status_bytes)))
        return rc;
    uint32_t *counts = c->g_counts.as<uint32_t>(), *status = b.status();
    HIP_OK(hipMemsetAsync(counts, 0, g.counts_bytes, s));
    HIP_OK(hipMemsetAsync(status, 0, g.status_bytes, s));
    if (b.full) HIP_OK(hipMemsetAsync(b.d_values, 0, g.values_bytes, s));
    uint64_t *Eb = b.Eb();
    SelArgs sel{src.keys, src.off, src.blob_bytes, src.n, src.key_len, g.mult, b_lo, nb32, counts, nullptr, nullptr, nullptr};
    uint16_t *mid_cw = nullptr;
    uint32_t *mid_base = nullptr;
    if (g.cls == GovClass::MID) {
        if ((rc = c->g_mid.grow(g.mid_bytes))) return rc;
        mid_cw = c->g_mid.as<uint16_t>();
        mid_base = (uint32_t *)(c->g_mid.as<uint8_t>() + g.cw_bytes);
    }
    if ((rc = gov_count(b, sel, mid_cw))) return rc;
    if ((rc = edge_offsets_impl(c, counts, nb, Eb, s))) return rc;  // A6: Eb[0..nb]
    if (e_lo) k_add_base<<<g.base_grid, 256, 0, s>>>(Eb, nb + 1, e_lo);
    uint64_t n_local = src.n;
    if (g.in.from_keys) {  // the range's key count: its last offset
        uint64_t eh = 0;
        HIP_OK(hipMemcpyAsync(&eh, Eb + nb, 8, hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));
        n_local = (eh & OFFSET_MASK) - e_lo;
    }
    b.n_local = n_local;
    if (b.n_found) *b.n_found = n_local;
    if (e_lo + n_local > b.n_global) return BSDB_EINVAL;
    if (b.ixo.slots && !(b.ixo.index = b.ixo.slots(n_local))) return BSDB_ENOMEM;
    const GovSolvePlan &sp = b.sp = gov_solve_plan(g, n_local, b.d_rank || b.ixo.index || b.group_only, b.width, b.knobs, gov_sizes());
    if ((rc = c->g_sorted.grow(sp.sorted_bytes))) return rc;
    if (sp.need_pay) {
        if ((rc = c->g_pay.grow(sp.pay_bytes))) return rc;
        b.pay = c->g_pay.as<uint64_t>();
    }
    if ((rc = c->g_big.grow(sp.big_bytes)) || (!b.group_only && (rc = c->g_scratch.grow(sp.scratch_bytes)))) return rc;
    uint64_t *sorted = b.sorted(), *pay = b.pay;
    unsigned long long *cursor = c->g_cursor.as<unsigned long long>();
    k_cursor_init<<<sp.cursor_grid, 256, 0, s>>>(Eb, nb, e_lo, c->g_cursor.as<uint64_t>());
    switch (g.cls) {  // (the class that counted)
        case GovClass::COPY_COUNTS:
        case GovClass::SEL:
            sel.cursor = cursor;
            sel.sorted = sorted;
            sel.pay = pay;
            if (src.n) launch_sel<1>(src, sel, sp.scatter_grid, s);
            break;
        case GovClass::SMALL:
            k_bucket_scatter_small<<<sp.scatter_grid, 256, 0, s>>>(src.sig, n_local, g.mult, b_lo, nb32, cursor, sorted, pay);
            break;
        case GovClass::MID:
            k_mid_colscan<<<g.col_grid, 256, 0, s>>>(mid_cw, g.mid_g, nb32, Eb, e_lo, mid_base);
            k_bucket_scatter_mid<<<sp.scatter_grid, MID_THREADS, 0, s>>>(src.sig, n_local, g.mult, b_lo, nb32, mid_base,
                                                                         counts + nb, cursor, sorted, pay);
            break;
        case GovClass::LARGE:
            k_bucket_scatter<<<sp.scatter_grid, 256, 0, s>>>(src.sig, n_local, g.mult, b_lo, cursor, sorted, pay);
            break;
        case GovClass::NONE: break;
    }
    k_bucket_sort<<<sp.sort_grid, 256, 0, s>>>(sorted, Eb, nb, e_lo, status, pay);  // A5
    k_big_list<<<sp.list_grid, 256, 0, s>>>(Eb, nb, status, c->g_big.as<uint32_t>(), sp.big_cap);
    return launch_status();
}

// The seed ledger carved out of g_led as the plan lays it out, zeroed (active: all ones).
static int gov_ledger(GovBuild &b, SeedLedger &led) {
    const GovLedger &l = b.sp.led;
    const int rc = b.c->g_led.grow(l.bytes);
    if (rc) return rc;
    uint8_t *q = b.c->g_led.as<uint8_t>();
    led.fail = (unsigned long long *)(q + l.fail);
    led.claim = (uint32_t *)(q + l.claim);
    led.won = (uint32_t *)(q + l.won);
    led.done = (uint32_t *)(q + l.done);
    led.active = (uint32_t *)(q + l.active);
    HIP_OK(hipMemsetAsync(q, 0, l.zero_bytes, b.s));
    HIP_OK(hipMemsetAsync(led.active, 0xFF, l.ones_bytes, b.s));
    return BSDB_OK;
}

// BSDB_GOV_PROFILE=1: the solver's phase counters, read back and printed to stderr.
static int gov_profile_report(GovBuild &b, const uint64_t *d_prof) {
    const GovSolvePlan &sp = b.sp;
    std::vector<uint64_t> h((size_t)sp.solve_grid * GP_N);
    HIP_OK(hipMemcpyAsync(h.data(), d_prof, h.size() * 8, hipMemcpyDeviceToHost, b.s));
    HIP_OK(hipStreamSynchronize(b.s));
    int occ = 0;
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_gov_solve<true>, GS_THREADS, sp.lds_pad);
    fprintf(stderr, "[gov-profile] solver workgroups per CU: %d (LDS %zu B each + %zu padding), grid %u\n", occ,
            sizeof(SolveLds), sp.lds_pad, sp.solve_grid);
    print_gov_profile(h, sp.solve_grid, b.g.m);
    return BSDB_OK;
}

// A8, with A11 (checksum bits at each rank), F2 (ranks) and A13 (index slots)
// in the solve.  Reads the grouping's status back first (the second host
// synchronisation): duplicates, a bucket too big, the oversized buckets.
static int gov_solve(GovBuild &b) {
    bsdb_ctx *c = b.c;
    const GovSolvePlan &sp = b.sp;
    hipStream_t s = b.s;
    uint32_t *status = b.status();
    int rc;
    uint32_t st[4] = {0, 0, 0, 0};
    HIP_OK(hipMemcpyAsync(st, status, 16, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    if (st[0] & GOV_DUP) return BSDB_EDUP;
    if (st[0] & GOV_TOO_BIG) return BSDB_E2BIG;
    const GovBigPlan bp = gov_big_plan(st[1], st[3], sp.big_cap, c->num_cus, gov_sizes());
    const uint32_t *big_list = c->g_big.as<uint32_t>();
    if (bp.nbig) {
        if ((rc = c->g_slabs.grow(bp.slabs_bytes))) return rc;
        if (bp.mid_grid && (rc = c->g_midscr.grow(bp.midscr_bytes))) return rc;
        k_bucket_sort_big<<<bp.sort_grid, GB_THREADS, 0, s>>>(b.sorted(), b.Eb(), b.e_lo, big_list, bp.nbig,
                                                              c->g_slabs.as<ulonglong2>(), status, b.pay);
    }
    // BSDB_GOV_PROFILE=1: per-phase cycle totals of the solver printed to stderr
    const bool gprof = b.knobs.profile;
    const size_t prof_bytes = (size_t)sp.solve_grid * GP_N * 8;
    std::unique_ptr<void, DevFree> prof_buf;
    uint64_t *d_prof = nullptr;
    if (gprof) {
        void *p = nullptr;
        HIP_OK(dmalloc(&p, prof_bytes));
        prof_buf.reset(p);
        d_prof = (uint64_t *)p;
        HIP_OK(hipMemsetAsync(d_prof, 0, prof_bytes, s));
    }
    if (b.width && b.full) HIP_OK(hipMemsetAsync(b.d_sigbits, 0, sp.sigbits_bytes, s));
    SeedLedger led;
    if ((rc = gov_ledger(b, led))) return rc;
    SolveArgs sa{b.sorted(), b.b_hi, b.d_E, b.d_values, c->g_scratch.as<uint64_t>(), status, d_prof, b.knobs.fvs_max,
                 b.b_lo, b.e_lo, b.d_sigbits, b.width, b.pay, b.d_rank, b.ixo.index, b.ixo.idx_lo, b.ixo.addr,
                 b.ixo.addr_base, b.ixo.addr_stride, led, b.knobs.spec};
    // zeroing status[2] (the bucket queue) above happens before both launches.
    // The oversized buckets (C2: ~3 of 66 667, 2.8 ms of one workgroup each)
    // are solved on a stream of their own, queued first, so their few
    // workgroups run beside k_gov_solve's instead of after them (they touch
    // other buckets; shared value words and checksum words are OR-ed).
    if (bp.nbig) {
        if (!c->big_stream) {
            HIP_OK(hipStreamCreateWithFlags(&c->big_stream, hipStreamNonBlocking));
            for (hipEvent_t &e : c->big_ev) HIP_OK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        }
        HIP_OK(hipEventRecord(c->big_ev[0], s));
        HIP_OK(hipStreamWaitEvent(c->big_stream, c->big_ev[0], 0));
        if (bp.mid_grid)
            k_gov_solve_mid<<<bp.mid_grid, GS_THREADS, 0, c->big_stream>>>(sa, big_list, bp.nbig, c->g_midscr.as<uint64_t>());
        if (bp.big_grid)
            k_gov_solve_big<<<bp.big_grid, GS_THREADS, 0, c->big_stream>>>(sa, big_list, bp.nbig, c->g_slabs.as<uint8_t>(),
                                                                          big_slab_bytes());
        HIP_OK(hipEventRecord(c->big_ev[1], c->big_stream));
    }
    // (the phase counters are compiled only into k_gov_solve<true>)
    const void *solve_fn = gprof ? (const void *)k_gov_solve<true> : (const void *)k_gov_solve<false>;
    if (sp.lds_pad) HIP_OK(hipFuncSetAttribute(solve_fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sp.lds_pad));
    if (gprof)
        k_gov_solve<true><<<sp.solve_grid, GS_THREADS, sp.lds_pad, s>>>(sa);  // A8
    else
        k_gov_solve<false><<<sp.solve_grid, GS_THREADS, sp.lds_pad, s>>>(sa);
    if (bp.nbig) HIP_OK(hipStreamWaitEvent(s, c->big_ev[1], 0));
    return gprof ? gov_profile_report(b, d_prof) : BSDB_OK;
}

// The optional bijection check, E[b_hi] handed to the next range, and the
// build's status.
static int gov_finish(GovBuild &b) {
    bsdb_ctx *c = b.c;
    hipStream_t s = b.s;
    uint32_t *status = b.status();
    int rc;
    const MphView v{b.d_E, b.d_values, nullptr, b.n_global, b.g.mult, b.width};
    if (c->verify && b.n_local) {
        const size_t bm_bytes = ((b.n_local + 63) / 64) * 8;
        void *p = nullptr;
        HIP_OK(dmalloc(&p, bm_bytes));
        std::unique_ptr<void, DevFree> bm(p);
        HIP_OK(hipMemsetAsync(p, 0, bm_bytes, s));
        k_verify_ranks<<<b.sp.verify_grid, 256, 0, s>>>(v, b.sorted(), b.n_local, b.e_lo, (unsigned long long *)p, status);
        HIP_OK(hipStreamSynchronize(s));
    }
    if (b.b_hi < b.g.m) HIP_OK(hipMemsetAsync(b.d_E + b.b_hi, 0, 8, s));  // owned by the next range
    if ((rc = launch_status())) return rc;
    uint32_t st = 0;
    HIP_OK(hipMemcpyAsync(&st, status, 4, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    if (st & GOV_DUP) return BSDB_EDUP;
    if (st & GOV_TOO_BIG) return BSDB_E2BIG;
    if (st & GOV_SEEDS) return BSDB_ESEEDS;
    if (st & GOV_VERIFY) return BSDB_EVERIFY;
    return BSDB_OK;
}

// A5 + A6 + A8 + A11 over the buckets [b_lo, b_hi) of a GOV structure on
// n_global keys; d_sig = the n_local signatures of that range.  full: a whole
// build (zeroes the outputs first); otherwise the caller zeroed full-size
// outputs and E[b_hi] is cleared again unless b_hi == m (the next range owns it).
// d_rank (optional, F2): the rank of input signature i at d_rank[i], from the
// solve itself.  With a key source the range's keys are found by re-hashing
// every key, and *n_found (optional) returns how many there were.
static int gov_build_impl(bsdb_ctx *c, const GovSrc &src, uint64_t n_global, uint64_t b_lo, uint64_t b_hi,
                          uint64_t e_lo, uint32_t width, uint64_t *d_E, uint64_t *d_values, uint64_t *d_sigbits,
                          int64_t *d_rank, const GovIndexOut &ixo, hipStream_t s, bool full, uint64_t *n_found = nullptr) {
    GovBuild b{c, src, n_global, b_lo, b_hi, e_lo, width, d_E, d_values, d_sigbits, d_rank, ixo, s, full, n_found,
               gov_knobs(),
               gov_group_plan({src.n, src.sig == nullptr, src.counts_all != nullptr, b_lo, b_hi, n_global, c->num_cus})};
    int rc;
    if ((rc = gov_group(b)) || (rc = gov_solve(b))) return rc;
    return gov_finish(b);
}

// the signature form used by the existing entry points
static int gov_build_impl(bsdb_ctx *c, const uint64_t *d_sig, uint64_t n_local, uint64_t n_global, uint64_t b_lo,
                          uint64_t b_hi, uint64_t e_lo, uint32_t width, uint64_t *d_E, uint64_t *d_values,
                          uint64_t *d_sigbits, int64_t *d_rank, hipStream_t s, bool full) {
    GovSrc src;
    src.sig = d_sig ? d_sig : reinterpret_cast<const uint64_t *>(16);  // (n_local == 0: never read)
    src.n = n_local;
    return gov_build_impl(c, src, n_global, b_lo, b_hi, e_lo, width, d_E, d_values, d_sigbits, d_rank, GovIndexOut{}, s,
                          full);
}

// What the bsdb_dev_gov_build* entry points share: the argument checks (every
// invalid combination is BSDB_EINVAL; `invalid`: the entry point's own), then
// the lock, the device, the stream and the workspace's order, then build(s).
template <class Build>
static int gov_entry(bsdb_ctx *c, const uint64_t *d_sig, uint64_t n_local, uint64_t n_global, uint32_t width,
                     const void *d_E, const void *d_values, const void *d_sigbits, bool invalid, void *stream,
                     Build &&build) {
    if (!c || width > 64 || !d_E || !d_values || (n_local && !d_sig) || (width && !d_sigbits) || !aligned16(d_sig) ||
        n_global / BUCKET_SIZE + 1 > 0x7FFFFFFFULL || invalid)
        return BSDB_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    HIP_OK(hipSetDevice(c->device));
    hipStream_t s = pick(c, stream);
    Ordered ord(c, s);
    return build(s);
}

static bool bad_range(uint64_t n_local, uint64_t n_global, uint64_t b_lo, uint64_t b_hi, uint64_t e_lo) {
    return b_lo >= b_hi || b_hi > n_global / BUCKET_SIZE + 1 || n_local > n_global || e_lo + n_local > n_global;
}

}  // extern "C++"

int bsdb_dev_gov_build(bsdb_ctx *c, const uint64_t *d_sig, uint64_t n, uint32_t width, uint64_t *d_E,
                       uint64_t *d_values, uint64_t *d_sigbits, void *stream) {
    return gov_entry(c, d_sig, n, n, width, d_E, d_values, d_sigbits, false, stream, [&](hipStream_t s) {
        return gov_build_impl(c, d_sig, n, n, 0, n / BUCKET_SIZE + 1, 0, width, d_E, d_values, d_sigbits, nullptr, s, true);
    });
}

int bsdb_dev_gov_build_ranks(bsdb_ctx *c, const uint64_t *d_sig, uint64_t n, uint32_t width, uint64_t *d_E,
                             uint64_t *d_values, uint64_t *d_sigbits, int64_t *d_rank, void *stream) {
    return gov_entry(c, d_sig, n, n, width, d_E, d_values, d_sigbits, n && !d_rank, stream, [&](hipStream_t s) {
        return gov_build_impl(c, d_sig, n, n, 0, n / BUCKET_SIZE + 1, 0, width, d_E, d_values, d_sigbits, d_rank, s, true);
    });
}

int bsdb_dev_gov_build_range(bsdb_ctx *c, const uint64_t *d_sig, uint64_t n_local, uint64_t n_global, uint64_t b_lo,
                             uint64_t b_hi, uint64_t e_lo, uint32_t width, uint64_t *d_E, uint64_t *d_values,
                             uint64_t *d_sigbits, int64_t *d_rank, void *stream) {
    return gov_entry(c, d_sig, n_local, n_global, width, d_E, d_values, d_sigbits,
                     bad_range(n_local, n_global, b_lo, b_hi, e_lo), stream, [&](hipStream_t s) {
                         return gov_build_impl(c, d_sig, n_local, n_global, b_lo, b_hi, e_lo, width, d_E, d_values,
                                               d_sigbits, d_rank, s, false);
                     });
}

// The value words and checksum words the range [e_lo, e_lo + n_local) of keys
// writes (store_bucket: words [vo >> 5, (vo + nv + 31) >> 5) of its vertices,
// the checksum fields of its ranks).
int bsdb_gov_range_windows(uint64_t n_global, uint32_t width, uint64_t e_lo, uint64_t n_local, uint64_t *out4) {
    if (!out4 || width > 64 || e_lo + n_local > n_global || n_global > (1ULL << 56)) return BSDB_EINVAL;
    auto vo = [](uint64_t x) { return (x * 281) >> 8; };  // vertexOffset (GOV:315-317)
    const uint64_t v_lo = vo(e_lo), v_hi = vo(e_lo + n_local);
    out4[0] = v_lo >> 5;
    out4[1] = ((v_hi + 31) >> 5) - out4[0];
    out4[2] = width ? (e_lo * width) >> 6 : 0;
    out4[3] = width ? ((((e_lo + n_local) * width) + 63) >> 6) - out4[2] : 0;
    return BSDB_OK;
}

int bsdb_dev_gov_build_window(bsdb_ctx *c, const uint64_t *d_sig, uint64_t n_local, uint64_t n_global, uint64_t b_lo,
                              uint64_t b_hi, uint64_t e_lo, uint32_t width, uint64_t *d_E_win, uint64_t *d_values_win,
                              uint64_t values_w0, uint64_t values_words, uint64_t *d_sigbits_win, uint64_t sig_w0,
                              uint64_t sig_words, int64_t *d_rank, void *stream) {
    // the windows must hold every word the range writes
    uint64_t need[4];
    const bool invalid = bad_range(n_local, n_global, b_lo, b_hi, e_lo) ||
                         bsdb_gov_range_windows(n_global, width, e_lo, n_local, need) != BSDB_OK || values_w0 > need[0] ||
                         values_w0 + values_words < need[0] + need[1] ||
                         (width && (sig_w0 > need[2] || sig_w0 + sig_words < need[2] + need[3]));
    // the range build indexes the structure globally: its bases are moved so
    // that every index it forms lands in the windows (no other word is touched)
    auto shift = [](uint64_t *p, uint64_t first) {
        return reinterpret_cast<uint64_t *>(reinterpret_cast<uintptr_t>(p) - (uintptr_t)first * 8);
    };
    return gov_entry(c, d_sig, n_local, n_global, width, d_E_win, d_values_win, d_sigbits_win, invalid, stream,
                     [&](hipStream_t s) {
                         return gov_build_impl(c, d_sig, n_local, n_global, b_lo, b_hi, e_lo, width, shift(d_E_win, b_lo),
                                               shift(d_values_win, values_w0),
                                               width ? shift(d_sigbits_win, sig_w0) : nullptr, d_rank, s, false);
                     });
}

int bsdb_dev_partition_owners(bsdb_ctx *c, const uint64_t *d_sig, const uint64_t *d_payload, uint64_t n, uint64_t m,
                              int nranks, uint64_t *d_out, uint64_t *d_payload_out, uint64_t *h_counts, void *stream) {
    if (!c || nranks < 1 || nranks > OWN_MAXR || m == 0 || m > 0x7FFFFFFFULL || !h_counts ||
        (n && (!d_sig || !d_out)) || !aligned16(d_sig) || !aligned16(d_out) || (!d_payload != !d_payload_out))
        return BSDB_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    HIP_OK(hipSetDevice(c->device));
    hipStream_t s = pick(c, stream);
    Ordered ord(c, s);
    int rc;
    if ((rc = c->g_cursor.grow(OWN_MAXR * 8))) return rc;
    unsigned long long *cur = c->g_cursor.as<unsigned long long>();
    HIP_OK(hipMemsetAsync(cur, 0, OWN_MAXR * 8, s));
    if (n) k_owner_count<<<grid_for(c->num_cus, n), 256, 0, s>>>(d_sig, n, (uint32_t)(2 * m), m, (uint32_t)nranks, cur);
    if ((rc = launch_status())) return rc;
    uint64_t cnt[OWN_MAXR];
    HIP_OK(hipMemcpyAsync(cnt, cur, nranks * 8, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    uint64_t start[OWN_MAXR], acc = 0;
    for (int g2 = 0; g2 < nranks; ++g2) {
        start[g2] = acc;
        acc += cnt[g2];
        h_counts[g2] = cnt[g2];
    }
    HIP_OK(hipMemcpyAsync(cur, start, nranks * 8, hipMemcpyHostToDevice, s));
    if (n)
        k_owner_scatter<<<grid_for(c->num_cus, n), 256, 0, s>>>(d_sig, d_payload, n, (uint32_t)(2 * m), m, (uint32_t)nranks, cur,
                                                       d_out, d_payload_out);
    if ((rc = launch_status())) return rc;
    HIP_OK(hipStreamSynchronize(s));  // start[] is a stack buffer
    return BSDB_OK;
}
