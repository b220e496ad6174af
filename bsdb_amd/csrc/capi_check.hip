// capi_check.hip -- a database checked against text input behind the C ABI
// (kernels: check_kernels.hip, plan: check_plan.hpp).  Included by
// bsdb_capi.hip after capi_text.hip.
//   bsdb_dev_db_check     the compare on device buffers: a chunk of text, the
//                         split's value descriptors and what locate returned
//   bsdb_db_check_text    files of text lines against a resident database
// What Builder's verify does one getAsBytes per line (tools/Builder.java:
// 184-228).  The files are read by the loop of bsdb_text_build
// (text_read_chunks, capi_text.hip), the keys packed by its k_text_pack<false>.

namespace {

// The check's kernels over `a` (cmp_len / coff are filled in here, from the
// context's workspace); the caller holds the context's lock and has set the
// device.  Nothing waits.
int check_launch(bsdb_ctx *c, const bsdb_db *db, CheckArgs a, hipStream_t s) {
    if (!a.count) return BSDB_OK;
    const uint32_t lgrid = check_lane_grid(a.count, c->num_cus);
    if (db->approx) {
        k_check_approx<<<lgrid, 256, 0, s>>>(a);
    } else {
        int rc;
        if ((rc = c->k_cmp.grow(4 * a.count)) || (rc = c->k_coff.grow(8 * (a.count + 1)))) return rc;
        a.cmp_len = c->k_cmp.as<uint32_t>();
        a.coff = c->k_coff.as<const uint64_t>();
        k_check_lengths<<<lgrid, 256, 0, s>>>(a);
        if ((rc = edge_offsets_impl(c, a.cmp_len, a.count, c->k_coff.as<uint64_t>(), s))) return rc;
        ProfScope ps(c, s, 3, a.count);  // (bsdb_set_profiling: the compare alone, tools/check_rate.py)
        k_check_values<<<check_values_grid(a.text_bytes, c->num_cus), 256, 0, s>>>(a);
    }
    k_check_report<<<lgrid, 256, 0, s>>>(a.status, a.count, a.record_base, a.out);
    return launch_status();
}

CheckArgs check_args(const bsdb_db *db, const uint8_t *d_text, uint64_t text_bytes, const uint32_t *d_vpos, const uint32_t *d_vlen,
                     const uint64_t *d_src, const uint32_t *d_dbvlen, uint8_t *d_status, uint64_t count, uint64_t record_base,
                     unsigned long long *d_report) {
    CheckArgs a{};
    a.text = d_text;
    a.text_bytes = text_bytes;
    a.image = db->d_image;
    a.image_bytes = db->image_bytes;
    a.vpos = d_vpos;
    a.vlen = d_vlen;
    a.src = d_src;
    a.dbvlen = d_dbvlen;
    a.status = d_status;
    a.count = count;
    a.record_base = record_base;
    a.out = d_report;
    return a;
}

// the device buffers of one bsdb_db_check_text call (freed when it ends)
struct CheckBufs {
    DevBuf text, desc, blob, off, src, dbvlen, status, report;
    ~CheckBufs() {
        for (DevBuf *q : {&text, &desc, &blob, &off, &src, &dbvlen, &status, &report}) q->free();
    }
};

// What one bsdb_db_check_text call keeps from chunk to chunk.
struct CheckRun {
    bsdb_ctx *c;
    bsdb_db *db;
    int sep;
    CheckBufs bufs;
    uint64_t records = 0;  // kept so far: the next chunk's record base
    std::vector<uint8_t> hstatus;
    std::vector<uint32_t> hkpos;
    // the not-OK records
    uint64_t bad_cap, *n_bad;
    uint32_t *bad_file;
    uint64_t *bad_offset;
    uint8_t *bad_status;
    // the reports on the device, in bufs.report: the text's, locate's (not returned), the check's
    unsigned long long *d_text_report() const { return bufs.report.as<unsigned long long>(); }
    unsigned long long *d_get_report() const { return d_text_report() + TW_WORDS; }
    unsigned long long *d_check_report() const { return d_get_report() + GW_WORDS; }
};

// The device step of one chunk, under the context's lock: the `cut` bytes at
// h_text (file `file`, from file offset `base`) go up and are split, their
// keys packed, located and checked; the status bytes come back and the not-OK
// records are appended.
int check_chunk_step(CheckRun &cr, int file, uint64_t base, const uint8_t *h_text, uint64_t cut, uint64_t *text_report) {
    bsdb_ctx *c = cr.c;
    CheckBufs &bufs = cr.bufs;
    std::lock_guard<std::mutex> g(c->mu);
    HIP_OK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    Ordered ord(c, s);
    const uint64_t cap = text_max_records(cut);
    int rc;
    if ((rc = bufs.text.grow(cut + 16)) || (rc = bufs.desc.grow(4 * 4 * cap))) return rc;
    if ((rc = h2d_bounce(s, bufs.text.p, h_text, cut))) return rc;
    const uint8_t *d_text = bufs.text.as<const uint8_t>();
    uint32_t *desc = bufs.desc.as<uint32_t>();
    if ((rc = text_split_impl(c, d_text, cut, (uint32_t)cr.sep, cap, desc, desc + cap, desc + 2 * cap, desc + 3 * cap,
                              cr.d_text_report(), s)))
        return rc;
    HIP_OK(hipMemcpyAsync(text_report, cr.d_text_report(), 8 * TW_WORDS, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    const uint64_t k = text_report[TW_RECORDS] - cr.records, record_base = cr.records;
    cr.records = text_report[TW_RECORDS];
    if (k > cap) return BSDB_EIO;
    if (!k) return BSDB_OK;
    if ((rc = bufs.blob.grow(text_blob_max(cut))) || (rc = bufs.off.grow(8 * (k + 1))) || (rc = bufs.src.grow(8 * k)) ||
        (rc = bufs.dbvlen.grow(4 * k)) || (rc = bufs.status.grow(k)))
        return rc;
    // the key blob and its offsets: the pack without an image, one run
    uint64_t no_file = 0, run_bytes = 0, blob_bytes = 0;
    const TextPackIO io{d_text, cut, {desc, desc + cap, desc + 2 * cap, desc + 3 * cap}, k, 1, 0, &no_file, nullptr, 0, &run_bytes,
                        nullptr, bufs.blob.as<uint8_t>(), text_blob_max(cut), bufs.off.as<uint64_t>(), &blob_bytes, nullptr, nullptr};
    if ((rc = text_pack_impl(c, io, s))) return rc;
    GetArgs ga{};
    ga.keys = bufs.blob.as<const uint8_t>();
    ga.off = bufs.off.as<const uint64_t>();
    ga.blob_bytes = blob_bytes;
    ga.nq = k;
    ga.src = bufs.src.as<uint64_t>();
    ga.vlen = bufs.dbvlen.as<uint32_t>();
    ga.status = bufs.status.as<uint8_t>();
    ga.out = cr.d_get_report();
    get_locate_launch(c, cr.db, ga, s);
    if ((rc = check_launch(c, cr.db,
                           check_args(cr.db, d_text, cut, desc + 2 * cap, desc + 3 * cap, ga.src, ga.vlen, ga.status, k, record_base,
                                      cr.d_check_report()),
                           s)))
        return rc;
    try {
        cr.hstatus.resize(k);
    } catch (const std::bad_alloc &) {
        return BSDB_ENOMEM;
    }
    HIP_OK(hipMemcpyAsync(cr.hstatus.data(), ga.status, k, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    if ((rc = launch_status())) return rc;
    bool have_kpos = false;
    for (uint64_t r = 0; r < k; ++r) {
        if (!cr.hstatus[r]) continue;
        const uint64_t at = (*cr.n_bad)++;
        if (at >= cr.bad_cap) continue;
        if (!have_kpos) {  // (the key positions come back only for a chunk that has a line to name)
            try {
                cr.hkpos.resize(k);
            } catch (const std::bad_alloc &) {
                return BSDB_ENOMEM;
            }
            HIP_OK(hipMemcpyAsync(cr.hkpos.data(), desc, 4 * k, hipMemcpyDeviceToHost, s));
            HIP_OK(hipStreamSynchronize(s));
            have_kpos = true;
        }
        cr.bad_file[at] = (uint32_t)file;
        cr.bad_offset[at] = base + cr.hkpos[r];
        cr.bad_status[at] = cr.hstatus[r];
    }
    return BSDB_OK;
}

}  // namespace

extern "C" {

int bsdb_dev_db_check(bsdb_db *db, const uint8_t *d_text, uint64_t text_bytes, const uint32_t *d_vpos, const uint32_t *d_vlen,
                      const uint64_t *d_src, const uint32_t *d_dbvlen, uint8_t *d_status, uint64_t count, uint64_t record_base,
                      uint64_t *d_report, void *stream) {
    if (!db || !d_report || ((uintptr_t)d_report & 7) || text_bytes > TEXT_MAX_BYTES || (text_bytes && !d_text) ||
        !aligned16(d_text) || (count && (!d_vpos || !d_vlen || !d_src || !d_dbvlen || !d_status)) ||
        (((uintptr_t)d_vpos | (uintptr_t)d_vlen | (uintptr_t)d_dbvlen) & 3) || ((uintptr_t)d_src & 7))
        return BSDB_EINVAL;
    bsdb_ctx *c = db_ctx(db);
    if (!c) return BSDB_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    HIP_OK(hipSetDevice(c->device));
    hipStream_t s = pick(c, stream);
    Ordered ord(c, s);
    return check_launch(c, db,
                        check_args(db, d_text, text_bytes, d_vpos, d_vlen, d_src, d_dbvlen, d_status, count, record_base,
                                   (unsigned long long *)d_report),
                        s);
}

int bsdb_db_check_text(bsdb_db *db, const char *const *paths, int nfiles, int sep, uint64_t *text_report, uint64_t *check_report,
                       uint64_t bad_cap, uint32_t *h_bad_file, uint64_t *h_bad_offset, uint8_t *h_bad_status, uint64_t *n_bad) {
    if (!db || nfiles < 0 || (nfiles && !paths) || text_bad_separator(sep) || !text_report || !check_report || !n_bad ||
        (bad_cap && (!h_bad_file || !h_bad_offset || !h_bad_status)))
        return BSDB_EINVAL;
    for (int f = 0; f < nfiles; ++f)
        if (!paths[f]) return BSDB_EINVAL;
    bsdb_ctx *c = db_ctx(db);
    if (!c) return BSDB_EINVAL;  // its MPHF was freed or its context closed
    memset(text_report, 0, sizeof(uint64_t) * BSDB_TEXT_WORDS);
    memset(check_report, 0, sizeof(uint64_t) * BSDB_CHECK_WORDS);
    check_report[CW_FIRST_BAD] = CHECK_NONE;
    *n_bad = 0;
    std::vector<TextReader> in((size_t)nfiles);
    uint64_t total_bytes = 0;
    int rc = text_open_inputs(paths, nfiles, in, total_bytes);
    if (rc) return rc;
    CheckRun cr{c, db, sep};
    cr.bad_cap = bad_cap, cr.n_bad = n_bad;
    cr.bad_file = h_bad_file, cr.bad_offset = h_bad_offset, cr.bad_status = h_bad_status;
    uint64_t chunk = 0;
    {
        // the chunk size beside the resident image, and the reports on the device
        std::lock_guard<std::mutex> g(c->mu);
        HIP_OK(hipSetDevice(c->device));
        size_t free_b = 0, total_b = 0;
        HIP_OK(hipMemGetInfo(&free_b, &total_b));
        chunk = check_chunk_bytes(c->text_chunk, free_b);
        const size_t words = TW_WORDS + GW_WORDS + CW_WORDS;
        if ((rc = cr.bufs.report.grow(8 * words))) return rc;
        HIP_OK(hipMemsetAsync(cr.bufs.report.p, 0, 8 * words, c->stream));
        HIP_OK(hipMemcpyAsync(cr.d_check_report() + CW_FIRST_BAD, &CHECK_NONE, 8, hipMemcpyHostToDevice, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
    }
    std::vector<uint8_t> hbuf;
    try {
        hbuf.resize(chunk);
    } catch (const std::bad_alloc &) {
        return BSDB_ENOMEM;
    }
    rc = text_read_chunks(in, hbuf, chunk, [&](int file, uint64_t base, const uint8_t *h_text, uint64_t cut) {
        return check_chunk_step(cr, file, base, h_text, cut, text_report);
    });
    std::lock_guard<std::mutex> g(c->mu);
    if (rc) {
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    HIP_OK(hipSetDevice(c->device));
    HIP_OK(hipMemcpyAsync(check_report, cr.d_check_report(), 8 * CW_WORDS, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    return check_report[CW_OK] == check_report[CW_RECORDS] ? BSDB_OK : BSDB_EVERIFY;
}

}  // extern "C"
