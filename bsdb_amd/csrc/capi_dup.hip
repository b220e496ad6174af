// capi_dup.hip -- which keys of a key set are duplicates:
// the query behind BSDB_EDUP.  Included by bsdb_capi.hip after capi_verify.hip.
//   CBHS = src/main/java/it/unimi/dsi/sux4j/io/ConcurrentBucketedHashStore.java
//   GOV  = src/main/java/it/unimi/dsi/sux4j/mph/GOVMinimalPerfectHashFunctionModified.java
//
// The build rejects a duplicate 128-bit signature (CBHS:969-972, GOV:471-479)
// where its bucket sort sees two equal neighbours, and says no more.  The
// finder runs the same grouping -- gov_group per bucket-range pass: count,
// scan, scatter of (signature, position), k_bucket_sort, then
// k_bucket_sort_big for the buckets of 1 665 .. GB_CMAX keys -- with none of
// the solve (no solver scratch, no seed ledger), reads the status word, and
// only where it carries GOV_DUP walks the sorted slice for runs of equal
// signatures (k_dup_collect).  A pass that finds nothing costs its grouping.
// Buckets over GB_CMAX keys (the build's GOV_TOO_BIG) are cut into chunks of
// GB_CMAX entries, each sorted and collected on its own: bounded work, and the
// report carries BSDB_DUP_PARTIAL.  dup_plan.hpp decides every size and grid.

namespace {

struct DupOut {
    uint64_t cap = 0;
    uint64_t *d_pairs = nullptr;   // 2 cap
    uint64_t *d_report = nullptr;  // BSDB_DUP_WORDS
};

static_assert(BSDB_DUP_WORDS == 4 && DUP_KEYS == 3, "the report's words");
static_assert(BSDB_DUP_LIST_FULL == DUP_F_LIST_FULL && BSDB_DUP_PARTIAL == DUP_F_PARTIAL, "the report's flags");
static_assert(BSDB_DUP_SAME_KEY == DUP_SAME_KEY && BSDB_DUP_COLLISION == DUP_COLLISION &&
                  BSDB_DUP_UNCOMPARED == DUP_UNCOMPARED,
              "the kinds");

// One pass: the buckets [b_lo, b_hi) of the structure over n keys grouped and
// sorted, their runs of equal signatures appended to the list.  pos: see
// k_dup_collect.  *n_found: the pass's key count.
int dup_pass(bsdb_ctx *c, const GovSrc &src, const uint64_t *pos, uint64_t n, uint64_t b_lo, uint64_t b_hi, uint64_t e_lo,
             uint64_t *d_E, const DupOut &o, hipStream_t s, uint64_t *n_found, bool *partial) {
    GovBuild b{c, src, n, b_lo, b_hi, e_lo, 0, d_E, nullptr, nullptr, nullptr, GovIndexOut{}, s, false, n_found, GovKnobs{},
               gov_group_plan({src.n, src.sig == nullptr, src.counts_all != nullptr, b_lo, b_hi, n, c->num_cus})};
    b.group_only = true;
    int rc;
    if ((rc = gov_group(b))) return rc;
    const uint64_t nb = b.g.nb;
    uint32_t *status = b.status();
    uint32_t st[4] = {0, 0, 0, 0};
    HIP_OK(hipMemcpyAsync(st, status, 16, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    const uint32_t nbig = std::min(st[3], b.sp.big_cap);
    const DupCollectPlan cp = dup_collect_plan(nb, b.n_local, nbig, c->num_cus);
    if (nbig) {  // buckets of 1 665 .. GB_CMAX keys: sorted here, as gov_solve does
        if ((rc = c->g_slabs.grow(cp.slabs_bytes))) return rc;
        k_bucket_sort_big<<<cp.big_sort_grid, GB_THREADS, 0, s>>>(b.sorted(), b.Eb(), e_lo, c->g_big.as<uint32_t>(), nbig,
                                                                  c->g_slabs.as<ulonglong2>(), status, b.pay);
        HIP_OK(hipMemcpyAsync(st, status, 4, hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));
    }
    if (st[0] & GOV_DUP)
        k_dup_collect<<<cp.collect_grid, 256, 0, s>>>(b.sorted(), b.pay, pos, b.Eb(), nb, nullptr, e_lo, o.cap, o.d_pairs,
                                                      o.d_report);
    if (st[0] & GOV_TOO_BIG) {  // buckets over GB_CMAX keys: chunk by chunk
        *partial = true;
        DevBuf over;
        if ((rc = over.grow(cp.over_bytes))) return rc;
        const uint32_t ec_cap = cp.chunk_cap + cp.over_cap;
        uint32_t *counters = over.as<uint32_t>();
        uint64_t *Ec = reinterpret_cast<uint64_t *>(over.as<uint8_t>() + 64);
        uint32_t *list = reinterpret_cast<uint32_t *>(Ec + ec_cap);
        auto released = [&](int r) {
            (void)hipStreamSynchronize(s);
            over.free();
            return r;
        };
        if (hipMemsetAsync(counters, 0, 64, s) != hipSuccess) return released(BSDB_EIO);
        k_dup_over_list<<<cp.over_grid, 256, 0, s>>>(b.Eb(), nb, Ec, ec_cap, list, cp.chunk_cap, counters);
        uint32_t got[2] = {0, 0};
        if (hipMemcpyAsync(got, counters, 8, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
            return released(BSDB_EIO);
        if (got[0] > cp.chunk_cap || got[1] > ec_cap) return released(BSDB_EIO);  // (the plan's bounds hold for every input)
        const DupOverPlan op = dup_over_plan(got[0], cp.chunk_cap, c->num_cus);
        if (op.chunks) {
            if ((rc = c->g_slabs.grow(op.slabs_bytes))) return released(rc);
            k_bucket_sort_big<<<op.sort_grid, GB_THREADS, 0, s>>>(b.sorted(), Ec, e_lo, list, op.chunks,
                                                                  c->g_slabs.as<ulonglong2>(), status, b.pay);
            k_dup_collect<<<op.collect_grid, 256, 0, s>>>(b.sorted(), b.pay, pos, Ec, op.chunks, list, e_lo, o.cap,
                                                          o.d_pairs, o.d_report);
        }
        if ((rc = released(launch_status()))) return rc;
    }
    return launch_status();
}

// The passes over a key set: src = the resident keys, or (source) each pass's
// signatures and positions, as PassSink::source gives them to the build.
// Zeroes the report, appends every pass's pairs, then sets flags and keys.
// Returns after the device finished.
int dup_find(bsdb_ctx *c, const GovSrc &src, uint64_t n, uint32_t passes,
             const std::function<int(uint64_t, uint64_t, GovSrc &, const uint64_t **)> &source,
             uint64_t source_bytes_per_key, const DupOut &o, hipStream_t s) {
    HIP_OK(hipMemsetAsync(o.d_report, 0, BSDB_DUP_WORDS * 8, s));
    bool partial = false;
    if (n) {
        // every bucket's count once, by the histogram stage, as passes_build does
        GovSrc gsrc = src;
        std::unique_ptr<void, DevFree> counts_all;
        const uint64_t m = n / BUCKET_SIZE + 1;
        const bool fixed_ok = src.off || (!bad_key_len(src.key_len) && aligned16(src.keys));
        if (n >= (1ULL << 16) && fixed_ok && !source && !src.sig) {
            void *q = nullptr;
            HIP_OK(dmalloc(&q, m * 4));
            counts_all.reset(q);
            HIP_OK(hipMemsetAsync(q, 0, m * 4, s));
            const int hrc = histogram_impl(c, src.keys, src.off, src.blob_bytes, src.off ? 0 : src.key_len, n, 0, m,
                                           (uint32_t *)q, HistOpts{1ULL << 30, 1}, s);
            HIP_OK(hipStreamSynchronize(s));
            c->ids.free();
            if (hrc) return hrc;
            gsrc.counts_all = (const uint32_t *)q;
        }
        HIP_OK(hipStreamSynchronize(s));
        c->g_sorted.free();
        c->g_pay.free();
        size_t free_b = 0, total_b = 0;
        HIP_OK(hipMemGetInfo(&free_b, &total_b));
        const DupPassPlan pp = dup_pass_plan(n, src.sig ? 1 : passes, free_b, source_bytes_per_key);
        DevBuf E;
        int rc = E.grow((pp.m + 1) * 8);
        if (rc) return rc;
        uint64_t e_lo = 0;
        for (uint32_t p = 0; p < pp.passes && !rc; ++p) {
            const uint64_t b_lo = (uint64_t)p * pp.m / pp.passes, b_hi = (uint64_t)(p + 1) * pp.m / pp.passes;
            if (b_lo >= b_hi) continue;
            GovSrc psrc = gsrc;
            const uint64_t *pos = nullptr;
            if (source) rc = source(b_lo, b_hi, psrc, &pos);
            uint64_t nl = 0;
            if (!rc) rc = dup_pass(c, psrc, pos, n, b_lo, b_hi, e_lo, E.as<uint64_t>(), o, s, &nl, &partial);
            e_lo += nl;
        }
        (void)hipStreamSynchronize(s);
        E.free();
        if (rc) return rc;
        if (e_lo != n) return BSDB_EIO;
    }
    k_dup_report<<<1, 64, 0, s>>>(o.d_report, o.cap, partial ? (uint64_t)DUP_F_PARTIAL : 0, n);
    const int rc = launch_status();
    if (rc) return rc;
    HIP_OK(hipStreamSynchronize(s));
    return BSDB_OK;
}

// kinds of the listed pairs (positions) by comparing the key bytes
int dup_classify(bsdb_ctx *c, const GovSrc &src, const uint64_t *d_pairs, uint64_t count, uint8_t *d_kinds,
                 uint64_t *d_report, hipStream_t s) {
    const DupListPlan lp = dup_list_plan(count, count, c->num_cus);
    if (!lp.listed) return BSDB_OK;
    if (src.off)
        k_dup_classify<2><<<lp.classify_grid, 256, 0, s>>>(src.keys, src.off, src.blob_bytes, src.n, 0, d_pairs, count, d_kinds,
                                                           d_report);
    else
        k_dup_classify<1><<<lp.classify_grid, 256, 0, s>>>(src.keys, nullptr, src.blob_bytes, src.n, src.key_len, d_pairs,
                                                           count, d_kinds, d_report);
    return launch_status();
}

// the pairs listed of a finished report: min(found, cap)
int dup_listed(const DupOut &o, hipStream_t s, uint64_t *listed) {
    uint64_t found = 0;
    HIP_OK(hipMemcpyAsync(&found, o.d_report, 8, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    *listed = std::min(found, o.cap);
    return BSDB_OK;
}

bool dup_keys_unaligned(const void *p) { return ((uintptr_t)p & 3) != 0; }

int dup_dev_entry(bsdb_ctx *c, const GovSrc &src, uint64_t n, uint32_t passes, uint64_t cap, uint64_t *d_pairs,
                  uint8_t *d_kinds, uint64_t *d_report, void *stream) {
    if (!c || !d_report || (cap && !d_pairs) || (n && !src.keys && !src.sig) || n / BUCKET_SIZE + 1 > 0x7FFFFFFFULL ||
        passes > 4096 || dup_keys_unaligned(src.keys) || !aligned16(src.sig))
        return BSDB_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    HIP_OK(hipSetDevice(c->device));
    hipStream_t s = pick(c, stream);
    Ordered ord(c, s);
    const DupOut o{cap, d_pairs, d_report};
    int rc = dup_find(c, src, n, passes, nullptr, 0, o, s);
    if (rc || !d_kinds || src.sig) return rc;
    uint64_t listed = 0;
    if ((rc = dup_listed(o, s, &listed)) || (rc = dup_classify(c, src, d_pairs, listed, d_kinds, d_report, s))) return rc;
    HIP_OK(hipStreamSynchronize(s));
    return BSDB_OK;
}

int dup_classify_entry(bsdb_ctx *c, const GovSrc &src, const uint64_t *d_pairs, uint64_t count, uint8_t *d_kinds,
                       void *stream) {
    // (a blob with offsets at any address, as bsdb_dev_hash_var takes it: the header asks no alignment of it)
    if (!c || (count && (!d_pairs || !d_kinds || !src.keys)) || (!src.off && dup_keys_unaligned(src.keys)))
        return BSDB_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    HIP_OK(hipSetDevice(c->device));
    return dup_classify(c, src, d_pairs, count, d_kinds, nullptr, pick(c, stream));
}

GovSrc dup_src_fixed(const uint8_t *d_keys, uint32_t key_len, uint64_t n) {
    GovSrc src;
    src.keys = d_keys;
    src.n = n;
    src.key_len = key_len;
    src.blob_bytes = n * key_len;
    return src;
}

GovSrc dup_src_var(const uint8_t *d_blob, uint64_t blob_bytes, const uint64_t *d_off, uint64_t n) {
    GovSrc src;
    src.keys = d_blob;
    src.off = d_off;
    src.n = n;
    src.blob_bytes = blob_bytes;
    return src;
}

// The finder over everything added to a builder (caller holds the builder's
// locks and the context's, device set): pairs of record addresses and kinds
// into host arrays.  Resident keys: compared (kinds 0 / 1); spill mode: the
// pairs come from the spilled (signature, position) segments and every kind
// is BSDB_DUP_UNCOMPARED.
int builder_find_duplicates_locked(bsdb_builder *b, uint64_t cap, uint64_t *h_pairs, uint8_t *h_kinds, uint64_t *report) {
    bsdb_ctx *c = b->c;
    hipStream_t s = c->stream;
    const uint64_t n = b->n;
    DevBuf d_pairs, d_kinds, d_report, sp_in, sp_out;
    auto done = [&](int rc) {
        (void)hipStreamSynchronize(s);
        for (DevBuf *q : {&d_pairs, &d_kinds, &d_report, &sp_in, &sp_out}) q->free();
        return rc;
    };
    const DupListPlan room = dup_list_plan(0, cap, c->num_cus);
    int rc;
    if ((rc = d_pairs.grow(std::max<size_t>(room.pairs_bytes, 16))) || (rc = d_kinds.grow(std::max<size_t>(room.kinds_bytes, 16))) ||
        (rc = d_report.grow(BSDB_DUP_WORDS * 8)))
        return done(rc);
    const DupOut o{cap, d_pairs.as<uint64_t>(), d_report.as<uint64_t>()};
    GovSrc src;
    src.n = n;
    src.keys = b->d_keys;
    const uint32_t flen = b->key_len ? b->key_len : (b->uniform && !bad_key_len(b->uni_len) ? b->uni_len : 0);
    if (flen) {  // (as the finish: one length, the fixed-length kernels over the same bytes)
        src.key_len = flen;
        src.blob_bytes = n * flen;
    } else {
        src.off = b->d_off;
        src.blob_bytes = b->key_bytes;
    }
    if (b->spill)
        rc = dup_find(c, src, n, 0, spill_source(b, sp_in, sp_out), SPILL_SOURCE_BYTES_PER_KEY, o, s);
    else
        rc = dup_find(c, src, n, 0, nullptr, 0, o, s);
    if (rc) return done(rc);
    uint64_t listed = 0;
    if ((rc = dup_listed(o, s, &listed))) return done(rc);
    if (b->spill) {
        if (listed && hipMemsetAsync(d_kinds.p, DUP_UNCOMPARED, listed, s) != hipSuccess) return done(BSDB_EIO);
    } else if ((rc = dup_classify(c, src, o.d_pairs, listed, d_kinds.as<uint8_t>(), o.d_report, s))) {
        return done(rc);
    }
    if (hipMemcpyAsync(report, o.d_report, BSDB_DUP_WORDS * 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
        (listed && (hipMemcpyAsync(h_pairs, o.d_pairs, listed * 16, hipMemcpyDeviceToHost, s) != hipSuccess ||
                    hipMemcpyAsync(h_kinds, d_kinds.p, listed, hipMemcpyDeviceToHost, s) != hipSuccess)) ||
        hipStreamSynchronize(s) != hipSuccess)
        return done(BSDB_EIO);
    // positions -> the records' addresses
    for (uint64_t i = 0; i < 2 * listed; ++i) {
        const uint64_t p = h_pairs[i];
        if (p >= n) return done(BSDB_EIO);
        h_pairs[i] = b->stride ? b->addr_base + b->addr_stride * p : b->addr.p[p];
    }
    return done(BSDB_OK);
}

// The builder's locks as the finish takes them, then the finder.
int builder_find_duplicates(bsdb_builder *b, uint64_t cap, uint64_t *h_pairs, uint8_t *h_kinds, uint64_t *report) {
    std::lock_guard<std::mutex> gb(b->mu);
    if (b->failed) return b->failed;
    if (b->finished || b->n / BUCKET_SIZE + 1 > 0x7FFFFFFFULL) return BSDB_EINVAL;
    if (!b->stride && !b->borrowed_records && b->addr.n < b->n) return BSDB_EINVAL;
    bsdb_ctx *c = b->c;
    std::unique_lock<std::shared_mutex> settled(b->grow_mu);  // every add's copies are done
    if (const int cf = b->copy_failed.load()) return b->failed = cf;
    std::lock_guard<std::mutex> g(c->mu);
    HIP_OK(hipSetDevice(c->device));
    Ordered ord(c, c->stream);
    return builder_find_duplicates_locked(b, cap, h_pairs, h_kinds, report);
}

// Keys in host memory through a builder whose addresses are the input
// positions (addr_base 0, addr_stride 1): batches as host_passes_build's.
int host_find_duplicates(bsdb_ctx *c, const uint8_t *h_keys, uint32_t key_len, const uint8_t *h_blob, const uint64_t *h_off,
                         uint64_t n, uint64_t cap, uint64_t *h_pairs, uint8_t *h_kinds, uint64_t *report) {
    const bool var = h_off != nullptr;
    const uint64_t blob = var ? (n ? h_off[n] - h_off[0] : 0) : 0;
    bsdb_builder *b = nullptr;
    int rc = builder_open(c, var ? 0 : key_len, n, blob, 0, 0, 1, &b, true);
    if (rc) return rc;
    constexpr uint64_t BATCH = 4ULL << 30;
    for (uint64_t k0 = 0; k0 < n && !rc;) {
        uint64_t k1;
        AddBatch a;
        if (var) {
            k1 = std::min<uint64_t>(n, k0 + (1ULL << 28));
            while (k1 - k0 > 1 && h_off[k1] - h_off[k0] > BATCH) k1 = k0 + (k1 - k0) / 2;
            uint32_t uni = 0;
            rc = var_batch_lengths(h_off + k0, k1 - k0, &uni);
            a.keys = h_blob;
            a.off = h_off + k0;
            a.uni = uni;
        } else {
            k1 = std::min(n, k0 + std::max<uint64_t>(1, BATCH / key_len));
            a.keys = h_keys + k0 * key_len;
            a.key_len = a.uni = key_len;
        }
        a.count = k1 - k0;
        if (!rc) rc = builder_add(b, a, nullptr, nullptr, nullptr);
        k0 = k1;
    }
    if (!rc) rc = builder_find_duplicates(b, cap, h_pairs, h_kinds, report);
    (void)bsdb_builder_free(b);
    return rc;
}

bool dup_host_args_bad(const void *ctx, uint64_t n, uint64_t cap, const void *h_pairs, const void *h_kinds,
                       const void *report) {
    return !ctx || !report || (cap && (!h_pairs || !h_kinds)) || n / BUCKET_SIZE + 1 > 0x7FFFFFFFULL;
}

}  // namespace

extern "C" {

int bsdb_dev_find_duplicates_fixed(bsdb_ctx *c, const uint8_t *d_keys, uint32_t key_len, uint64_t n, uint32_t passes,
                                   uint64_t cap, uint64_t *d_pairs, uint8_t *d_kinds, uint64_t *d_report, void *stream) {
    if (bad_key_len(key_len)) return BSDB_EINVAL;
    return dup_dev_entry(c, dup_src_fixed(d_keys, key_len, n), n, passes, cap, d_pairs, d_kinds, d_report, stream);
}

int bsdb_dev_find_duplicates_var(bsdb_ctx *c, const uint8_t *d_blob, uint64_t blob_bytes, const uint64_t *d_off, uint64_t n,
                                 uint32_t passes, uint64_t cap, uint64_t *d_pairs, uint8_t *d_kinds, uint64_t *d_report,
                                 void *stream) {
    if (n && (!d_off || !d_blob)) return BSDB_EINVAL;
    return dup_dev_entry(c, dup_src_var(d_blob, blob_bytes, d_off, n), n, passes, cap, d_pairs, d_kinds, d_report, stream);
}

int bsdb_dev_find_duplicates_sig(bsdb_ctx *c, const uint64_t *d_sig, uint64_t n, uint64_t cap, uint64_t *d_pairs,
                                 uint64_t *d_report, void *stream) {
    if (n && !d_sig) return BSDB_EINVAL;
    GovSrc src;
    src.sig = d_sig ? d_sig : reinterpret_cast<const uint64_t *>(16);  // (n == 0: never read)
    src.n = n;
    return dup_dev_entry(c, src, n, 1, cap, d_pairs, nullptr, d_report, stream);
}

int bsdb_dev_classify_pairs_fixed(bsdb_ctx *c, const uint8_t *d_keys, uint32_t key_len, uint64_t n, const uint64_t *d_pairs,
                                  uint64_t count, uint8_t *d_kinds, void *stream) {
    if (bad_key_len(key_len)) return BSDB_EINVAL;
    return dup_classify_entry(c, dup_src_fixed(d_keys, key_len, n), d_pairs, count, d_kinds, stream);
}

int bsdb_dev_classify_pairs_var(bsdb_ctx *c, const uint8_t *d_blob, uint64_t blob_bytes, const uint64_t *d_off, uint64_t n,
                                const uint64_t *d_pairs, uint64_t count, uint8_t *d_kinds, void *stream) {
    if (count && !d_off) return BSDB_EINVAL;
    return dup_classify_entry(c, dup_src_var(d_blob, blob_bytes, d_off, n), d_pairs, count, d_kinds, stream);
}

int bsdb_find_duplicates_fixed(bsdb_ctx *c, const uint8_t *h_keys, uint32_t key_len, uint64_t n, uint64_t cap,
                               uint64_t *h_pairs, uint8_t *h_kinds, uint64_t *report) {
    if (dup_host_args_bad(c, n, cap, h_pairs, h_kinds, report) || bad_key_len(key_len) || (n && !h_keys)) return BSDB_EINVAL;
    return host_find_duplicates(c, h_keys, key_len, nullptr, nullptr, n, cap, h_pairs, h_kinds, report);
}

int bsdb_find_duplicates_var(bsdb_ctx *c, const uint8_t *h_blob, const uint64_t *h_off, uint64_t n, uint64_t cap,
                             uint64_t *h_pairs, uint8_t *h_kinds, uint64_t *report) {
    if (dup_host_args_bad(c, n, cap, h_pairs, h_kinds, report) || !h_off || (n && !h_blob)) return BSDB_EINVAL;
    return host_find_duplicates(c, nullptr, 0, h_blob, h_off, n, cap, h_pairs, h_kinds, report);
}

int bsdb_builder_find_duplicates(bsdb_builder *b, uint64_t cap, uint64_t *h_addr_pairs, uint8_t *h_kinds, uint64_t *report) {
    if (!b || dup_host_args_bad(b, 0, cap, h_addr_pairs, h_kinds, report)) return BSDB_EINVAL;
    return builder_find_duplicates(b, cap, h_addr_pairs, h_kinds, report);
}

int bsdb_kv_find_duplicates(bsdb_ctx *c, const char *kv_base, int partitions, int format, uint32_t block_size, int threads,
                            uint64_t cap, uint64_t *h_addr_pairs, uint8_t *h_kinds, uint64_t *report) {
    if (dup_host_args_bad(c, 0, cap, h_addr_pairs, h_kinds, report) || !kv_base || partitions < 1 ||
        (format != 0 && format != 1) || (format == 1 && (block_size == 0 || block_size % KV_PAGE)))
        return BSDB_EINVAL;
    bsdb_builder *b = nullptr;
    int rc = builder_open(c, 0, 0, 0, 0, 0, 0, &b);
    if (rc) return rc;
    // the scan of bsdb_kv_build_index: every parsed chunk into the builder (keys
    // into HBM, addresses kept in host memory), from the scan threads
    rc = kv_scan_chunks(kv_base, partitions, format, block_size, threads, false, [&](KvPart &part) {
        uint32_t uni = 0;
        const uint64_t k = part.addr.size();
        int f = var_batch_lengths(part.off.data(), k, &uni);
        if (f) return f;
        AddBatch a;
        a.keys = part.blob.data();
        a.off = part.off.data();
        a.count = k;
        a.uni = uni;
        return builder_add(b, a, part.addr.data(), nullptr, nullptr);
    });
    if (!rc) rc = builder_find_duplicates(b, cap, h_addr_pairs, h_kinds, report);
    (void)bsdb_builder_free(b);
    return rc;
}

}  // extern "C"
