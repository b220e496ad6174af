// capi_diff.hip -- the diff of two resident databases behind the C ABI
// (kernels: diff_kernels.hip, plan: diff_plan.hpp).  Included by bsdb_capi.hip
// after capi_dump.hip.
//   bsdb_dev_db_diff     the compare on device buffers: A's descriptors and
//                        what locate returned for A's keys in B
//   bsdb_dev_db_select   the records of chosen statuses, in slot order
//   bsdb_db_diff         both directions over all slots, the delta as text
// The reference has no diff.  The pieces around the two new launches are the
// dump's and the get's: k_db_records lists a side, the get's scan and gather
// pack its keys, k_get_locate finds them in the other side, and the dump's
// text kernels write the selected records.

namespace {

// The diff's kernels over `a` (cmp_len / coff are filled in here, from the
// context's workspace); the caller holds the context's lock and has set the
// device.  Nothing waits.
int diff_launch(bsdb_ctx *c, DiffArgs a, hipStream_t s) {
    if (!a.count) return BSDB_OK;
    int rc;
    if ((rc = c->k_cmp.grow(4 * a.count)) || (rc = c->k_coff.grow(8 * (a.count + 1)))) return rc;
    a.cmp_len = c->k_cmp.as<uint32_t>();
    a.coff = c->k_coff.as<const uint64_t>();
    const uint32_t lgrid = diff_lane_grid(a.count, c->num_cus);
    k_diff_lengths<<<lgrid, 256, 0, s>>>(a);
    if ((rc = edge_offsets_impl(c, a.cmp_len, a.count, c->k_coff.as<uint64_t>(), s))) return rc;
    {
        ProfScope ps(c, s, 5, a.count);  // (bsdb_set_profiling: the compare alone, tools/diff_rate.py)
        k_diff_values<<<diff_values_grid(a.count, c->num_cus), 256, 0, s>>>(a);
    }
    k_diff_report<<<lgrid, 256, 0, s>>>(a);
    return launch_status();
}

DiffArgs diff_args(const bsdb_db *da, const bsdb_db *db, uint64_t count, const uint64_t *d_vsrc_a, const uint32_t *d_vlen_a,
                   const uint8_t *d_status_a, const uint64_t *d_src_b, const uint32_t *d_vlen_b, uint8_t *d_status,
                   uint64_t slot_base, unsigned long long *d_report) {
    DiffArgs a{};
    a.image_a = da->d_image, a.bytes_a = da->image_bytes;
    a.image_b = db->d_image, a.bytes_b = db->image_bytes;
    a.vsrc_a = d_vsrc_a, a.vlen_a = d_vlen_a, a.status_a = d_status_a;
    a.src_b = d_src_b, a.vlen_b = d_vlen_b;
    a.status = d_status;
    a.count = count;
    a.slot_base = slot_base;
    a.out = d_report;
    return a;
}

// The selection's kernels over `a` (flag / soff are filled in here, from the
// context's workspace); *a.nsel = 0 when there is no record.
int select_launch(bsdb_ctx *c, SelectArgs a, hipStream_t s) {
    if (!a.count) {
        HIP_OK(hipMemsetAsync(a.nsel, 0, 8, s));
        return BSDB_OK;
    }
    int rc;
    if ((rc = c->k_cmp.grow(4 * a.count)) || (rc = c->k_coff.grow(8 * (a.count + 1)))) return rc;
    a.flag = c->k_cmp.as<uint32_t>();
    a.soff = c->k_coff.as<const uint64_t>();
    const uint32_t lgrid = diff_lane_grid(a.count, c->num_cus);
    k_diff_select_flags<<<lgrid, 256, 0, s>>>(a);
    if ((rc = edge_offsets_impl(c, a.flag, a.count, c->k_coff.as<uint64_t>(), s))) return rc;
    k_diff_select_scatter<<<lgrid, 256, 0, s>>>(a);
    return launch_status();
}

// a database the diff can read: exact, its MPHF alive
bool diff_bad_db(const bsdb_db *db) { return !db || db->approx; }

// the device buffers of one bsdb_db_diff call (freed when it ends)
struct DiffBufs {
    DevBuf ksrc, vsrc, klen, vlen, st_a, koff, keys;  // a chunk of one side: descriptors, packed keys
    DevBuf src_b, vlen_b, status;                     // what locate gave in the other side; the diff's status
    DevBuf sel, ksrc_o, vsrc_o, klen_o, vlen_o;       // the selection
    DevBuf st_o, llen, loff, text;                    // its text
    DevBuf report;
    ~DiffBufs() {
        for (DevBuf *q : {&ksrc, &vsrc, &klen, &vlen, &st_a, &koff, &keys, &src_b, &vlen_b, &status, &sel, &ksrc_o, &vsrc_o, &klen_o,
                          &vlen_o, &st_o, &llen, &loff, &text, &report})
            q->free();
    }
    int grow(uint64_t nk) {
        int rc;
        for (DevBuf *q : {&ksrc, &vsrc, &src_b, &sel, &ksrc_o, &vsrc_o})
            if ((rc = q->grow(8 * nk))) return rc;
        for (DevBuf *q : {&klen, &vlen, &vlen_b, &klen_o, &vlen_o, &llen})
            if ((rc = q->grow(4 * nk))) return rc;
        for (DevBuf *q : {&st_a, &status, &st_o})
            if ((rc = q->grow(nk))) return rc;
        if ((rc = koff.grow(8 * (nk + 1))) || (rc = loff.grow(8 * (nk + 1)))) return rc;
        return BSDB_OK;
    }
    // the reports on the device: the diff's, the text's, the records' and locate's (nobody reads those two), nsel
    unsigned long long *d_diff() const { return report.as<unsigned long long>(); }
    unsigned long long *d_text() const { return d_diff() + FW_WORDS; }
    unsigned long long *d_records() const { return d_text() + DW_WORDS; }
    unsigned long long *d_get() const { return d_records() + DW_WORDS; }
    uint64_t *d_nsel() const { return (uint64_t *)(d_get() + GW_WORDS); }
    static constexpr size_t WORDS = FW_WORDS + 2 * DW_WORDS + GW_WORDS + 1;
    int zero_reports(hipStream_t s) {
        int rc;
        if ((rc = report.grow(8 * WORDS))) return rc;
        HIP_OK(hipMemsetAsync(report.p, 0, 8 * WORDS, s));
        for (unsigned long long *w : {d_diff() + FW_FIRST_DIFF, d_text() + DW_FIRST_BAD, d_records() + DW_FIRST_BAD})
            HIP_OK(hipMemsetAsync(w, 0xFF, 8, s));
        return BSDB_OK;
    }
};

void diff_empty_report(uint64_t *report) {
    memset(report, 0, sizeof(uint64_t) * BSDB_DIFF_WORDS);
    report[FW_FIRST_DIFF] = DIFF_NONE;
}

// What one direction of bsdb_db_diff keeps from chunk to chunk.
struct DiffRun {
    bsdb_ctx *c;
    bsdb_db *from, *to;  // every slot of `from` is looked up in `to`
    uint32_t mask;       // the statuses whose records go to the file
    int fd, sep;         // fd < 0: no file
    uint64_t written = 0;  // records written so far: the text report's first_bad counts lines of the file
    std::vector<uint64_t> hloff;
    std::vector<uint8_t> htext;
};

// The selected records' lines to the file, a piece of text at a time, each cut
// to the cap as bsdb_db_dump_text cuts its own; under the context's lock.
int diff_write_selected(DiffRun &r, DiffBufs &b, uint64_t nsel, uint64_t cap, hipStream_t s) {
    bsdb_ctx *c = r.c;
    for (uint64_t p0 = 0; p0 < nsel;) {
        const uint64_t nk = nsel - p0;
        int rc;
        try {
            r.hloff.resize(nk + 1);
        } catch (const std::bad_alloc &) {
            return BSDB_ENOMEM;
        }
        DumpArgs a = dump_args(r.from, nk, b.ksrc_o.as<uint64_t>() + p0, b.klen_o.as<uint32_t>() + p0, b.vsrc_o.as<uint64_t>() + p0,
                               b.vlen_o.as<uint32_t>() + p0, b.st_o.as<uint8_t>() + p0, b.llen.as<uint32_t>(),
                               b.loff.as<const uint64_t>(), r.sep, nullptr, 0, r.written, b.d_text());
        if ((rc = dump_lengths_launch(c, a, b.loff.as<uint64_t>(), s))) return rc;
        HIP_OK(hipMemcpyAsync(r.hloff.data(), b.loff.p, (nk + 1) * 8, hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));
        const uint64_t cut = dump_cut(r.hloff.data(), nk, cap), bytes = r.hloff[cut];
        if ((rc = b.text.grow(bytes))) return rc;
        try {
            r.htext.resize(bytes);
        } catch (const std::bad_alloc &) {
            return BSDB_ENOMEM;
        }
        a.count = cut;
        a.text = b.text.as<uint8_t>();
        a.text_bytes = bytes;
        if ((rc = dump_text_launch(c, a, s))) return rc;
        if (bytes) HIP_OK(hipMemcpyAsync(r.htext.data(), b.text.p, bytes, hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));
        if ((rc = launch_status())) return rc;
        if (write_all(r.fd, r.htext.data(), bytes)) return BSDB_EFILE;
        p0 += cut, r.written += cut;
    }
    return BSDB_OK;
}

// One chunk of one direction, under the context's lock: slots [r0, r0 + nk) of
// `from` listed, their keys packed and located in `to`, the values compared;
// then, with a file, the records of the mask's statuses selected and written.
int diff_chunk_step(DiffRun &r, DiffBufs &b, uint64_t r0, uint64_t nk, uint64_t cap) {
    bsdb_ctx *c = r.c;
    std::lock_guard<std::mutex> g(c->mu);
    HIP_OK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    Ordered ord(c, s);
    int rc;
    if ((rc = b.grow(nk))) return rc;
    const RecordsArgs ra{r0, nk, b.ksrc.as<uint64_t>(), b.vsrc.as<uint64_t>(), b.klen.as<uint32_t>(), b.vlen.as<uint32_t>(),
                         b.st_a.as<uint8_t>(), b.d_records()};
    dump_records_launch(c, r.from, ra, s);
    if ((rc = edge_offsets_impl(c, ra.klen, nk, b.koff.as<uint64_t>(), s))) return rc;
    uint64_t key_bytes = 0;
    HIP_OK(hipMemcpyAsync(&key_bytes, b.koff.as<uint64_t>() + nk, 8, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    if ((rc = b.keys.grow(key_bytes + 16))) return rc;
    get_gather_launch(c, r.from, ra.ksrc, b.koff.as<const uint64_t>(), nk, b.keys.as<uint8_t>(), key_bytes, s);
    GetArgs ga{};
    ga.keys = b.keys.as<const uint8_t>();
    ga.off = b.koff.as<const uint64_t>();
    ga.blob_bytes = key_bytes;
    ga.nq = nk;
    ga.src = b.src_b.as<uint64_t>();
    ga.vlen = b.vlen_b.as<uint32_t>();
    ga.status = b.status.as<uint8_t>();
    ga.out = b.d_get();
    get_locate_launch(c, r.to, ga, s);
    if ((rc = diff_launch(c, diff_args(r.from, r.to, nk, ra.vsrc, ra.vlen, ra.status, ga.src, ga.vlen, ga.status, r0, b.d_diff()), s)))
        return rc;
    if (r.fd < 0) return launch_status();
    SelectArgs sa{};
    sa.status = ga.status;
    sa.count = nk;
    sa.mask = r.mask;
    sa.ksrc = ra.ksrc, sa.vsrc = ra.vsrc, sa.klen = ra.klen, sa.vlen = ra.vlen;
    sa.sel = b.sel.as<uint64_t>();
    sa.ksrc_out = b.ksrc_o.as<uint64_t>(), sa.vsrc_out = b.vsrc_o.as<uint64_t>();
    sa.klen_out = b.klen_o.as<uint32_t>(), sa.vlen_out = b.vlen_o.as<uint32_t>();
    sa.nsel = b.d_nsel();
    if ((rc = select_launch(c, sa, s))) return rc;
    HIP_OK(hipMemsetAsync(b.st_o.p, 0, nk, s));
    uint64_t nsel = 0;
    HIP_OK(hipMemcpyAsync(&nsel, b.d_nsel(), 8, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    if ((rc = launch_status())) return rc;
    if (nsel > nk) return BSDB_EIO;
    return diff_write_selected(r, b, nsel, cap, s);
}

// One direction: every slot of `from` against `to`, in chunks; the reports come back at its end.
int diff_direction(DiffRun &r, uint64_t *report, uint64_t *scan_report) {
    bsdb_ctx *c = r.c;
    DiffBufs b;
    uint64_t chunk = 0, cap = 0;
    {
        std::lock_guard<std::mutex> g(c->mu);
        HIP_OK(hipSetDevice(c->device));
        chunk = get_host_chunk(r.from->batch, 0);
        cap = dump_chunk_bytes(r.from->text_chunk);
        int rc = b.zero_reports(c->stream);
        if (rc) return rc;
        HIP_OK(hipStreamSynchronize(c->stream));
    }
    for (uint64_t r0 = 0, n = r.from->n; r0 < n; r0 += chunk) {
        const int rc = diff_chunk_step(r, b, r0, std::min(chunk, n - r0), cap);
        if (rc) {
            std::lock_guard<std::mutex> g(c->mu);
            (void)hipStreamSynchronize(c->stream);
            return rc;
        }
    }
    std::lock_guard<std::mutex> g(c->mu);
    HIP_OK(hipSetDevice(c->device));
    HIP_OK(hipMemcpyAsync(report, b.d_diff(), sizeof(uint64_t) * FW_WORDS, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipMemcpyAsync(scan_report, b.d_text(), sizeof(uint64_t) * DW_WORDS, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    return BSDB_OK;
}

}  // namespace

extern "C" {

int bsdb_dev_db_diff(bsdb_db *a, bsdb_db *b, uint64_t count, const uint64_t *d_vsrc_a, const uint32_t *d_vlen_a,
                     const uint8_t *d_status_a, const uint64_t *d_src_b, const uint32_t *d_vlen_b, uint8_t *d_status,
                     uint64_t slot_base, uint64_t *d_report, void *stream) {
    if (diff_bad_db(a) || diff_bad_db(b) || count > DIFF_MAX_COUNT || !d_report || ((uintptr_t)d_report & 7) ||
        (count && (!d_vsrc_a || !d_vlen_a || !d_status_a || !d_src_b || !d_vlen_b || !d_status)) ||
        (((uintptr_t)d_vsrc_a | (uintptr_t)d_src_b) & 7) || (((uintptr_t)d_vlen_a | (uintptr_t)d_vlen_b) & 3))
        return BSDB_EINVAL;
    bsdb_ctx *c = db_ctx(a);
    if (!c || db_ctx(b) != c) return BSDB_EINVAL;  // an MPHF freed, a context closed, or two contexts
    std::lock_guard<std::mutex> g(c->mu);
    HIP_OK(hipSetDevice(c->device));
    hipStream_t s = pick(c, stream);
    Ordered ord(c, s);
    return diff_launch(c, diff_args(a, b, count, d_vsrc_a, d_vlen_a, d_status_a, d_src_b, d_vlen_b, d_status, slot_base,
                                    (unsigned long long *)d_report),
                       s);
}

int bsdb_dev_db_select(bsdb_db *db, uint64_t count, const uint8_t *d_status, uint32_t mask, const uint64_t *d_ksrc,
                       const uint32_t *d_klen, const uint64_t *d_vsrc, const uint32_t *d_vlen, uint64_t *d_sel, uint64_t *d_ksrc_out,
                       uint32_t *d_klen_out, uint64_t *d_vsrc_out, uint32_t *d_vlen_out, uint64_t *d_nsel, void *stream) {
    if (diff_bad_db(db) || diff_bad_mask(mask) || count > DIFF_MAX_COUNT || !d_nsel || ((uintptr_t)d_nsel & 7) ||
        (count && (!d_status || !d_ksrc || !d_klen || !d_vsrc || !d_vlen || !d_sel || !d_ksrc_out || !d_klen_out || !d_vsrc_out ||
                   !d_vlen_out)) ||
        (((uintptr_t)d_ksrc | (uintptr_t)d_vsrc | (uintptr_t)d_sel | (uintptr_t)d_ksrc_out | (uintptr_t)d_vsrc_out) & 7) ||
        (((uintptr_t)d_klen | (uintptr_t)d_vlen | (uintptr_t)d_klen_out | (uintptr_t)d_vlen_out) & 3))
        return BSDB_EINVAL;
    bsdb_ctx *c = db_ctx(db);
    if (!c) return BSDB_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    HIP_OK(hipSetDevice(c->device));
    hipStream_t s = pick(c, stream);
    Ordered ord(c, s);
    SelectArgs a{};
    a.status = d_status;
    a.count = count;
    a.mask = mask;
    a.ksrc = d_ksrc, a.vsrc = d_vsrc, a.klen = d_klen, a.vlen = d_vlen;
    a.sel = d_sel;
    a.ksrc_out = d_ksrc_out, a.vsrc_out = d_vsrc_out, a.klen_out = d_klen_out, a.vlen_out = d_vlen_out;
    a.nsel = d_nsel;
    return select_launch(c, a, s);
}

int bsdb_db_diff(bsdb_db *a, bsdb_db *b, int separator, const char *upsert_path, const char *removed_path, uint64_t *report_ab,
                 uint64_t *report_ba, uint64_t *scan_upsert, uint64_t *scan_removed) {
    if (diff_bad_db(a) || diff_bad_db(b) || text_bad_separator(separator) || !report_ab || !report_ba || !scan_upsert || !scan_removed)
        return BSDB_EINVAL;
    bsdb_ctx *c = db_ctx(a);
    if (!c || db_ctx(b) != c) return BSDB_EINVAL;  // an MPHF freed, a context closed, or two contexts
    diff_empty_report(report_ab);
    diff_empty_report(report_ba);
    dump_empty_report(scan_upsert);
    dump_empty_report(scan_removed);
    Fd up, rm;
    if (removed_path && (rm.fd = ::open(removed_path, O_WRONLY | O_CREAT | O_TRUNC, 0644)) < 0) return BSDB_EFILE;
    if (upsert_path && (up.fd = ::open(upsert_path, O_WRONLY | O_CREAT | O_TRUNC, 0644)) < 0) return BSDB_EFILE;
    DiffRun ab{c, a, b, DIFF_MASK_ABSENT, rm.fd, separator};
    int rc = diff_direction(ab, report_ab, scan_removed);
    if (rc) return rc;
    DiffRun ba{c, b, a, DIFF_MASK_UPSERT, up.fd, separator};
    return diff_direction(ba, report_ba, scan_upsert);
}

}  // extern "C"
