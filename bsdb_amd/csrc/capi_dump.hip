// capi_dump.hip -- a resident database enumerated by slot behind the C ABI
// (kernels: dump_kernels.hip, plan: dump_plan.hpp).  Included by bsdb_capi.hip
// after capi_check.hip.
//   bsdb_dev_db_records        slots -> record descriptors on device buffers
//   bsdb_dev_db_dump_lengths   descriptors -> line lengths and their scan
//   bsdb_dev_db_dump_text      descriptors + scan -> "key<sep>value\n" text
//   bsdb_db_scan               a slot window -> packed keys and values in host memory
//   bsdb_db_dump_text          a slot window -> a text file
// Exact mode only: an approximate database holds no records.  The packed keys
// and values are the get's scan and gather (edge_offsets_impl, k_get_gather)
// over the descriptors.

namespace {

// db is exact and [first, first + count) are slots of it
bool dump_bad_window(const bsdb_db *db, uint64_t first, uint64_t count) {
    return !db || db->approx || first > db->n || count > db->n - first;
}

void dump_records_launch(bsdb_ctx *c, const bsdb_db *db, const RecordsArgs &a, hipStream_t s) {
    if (!a.count) return;
    k_db_records<<<dump_lane_grid(a.count, c->num_cus), 256, 0, s>>>(db_view(db), a);
}

// line lengths and their scan (d_loff[0] = 0 when there is no record)
int dump_lengths_launch(bsdb_ctx *c, const DumpArgs &a, uint64_t *d_loff, hipStream_t s) {
    if (!a.count) {
        HIP_OK(hipMemsetAsync(d_loff, 0, 8, s));
        return BSDB_OK;
    }
    k_dump_lengths<<<dump_lane_grid(a.count, c->num_cus), 256, 0, s>>>(a);
    return edge_offsets_impl(c, a.llen, a.count, d_loff, s);
}

// the text (when there is any) and the report
int dump_text_launch(bsdb_ctx *c, const DumpArgs &a, hipStream_t s) {
    if (!a.count) return BSDB_OK;
    if (a.text_bytes) {
        ProfScope ps(c, s, 4, a.count);  // (bsdb_set_profiling: the text kernel alone, tools/dump_rate.py)
        const uint32_t mis = (uint32_t)((uintptr_t)a.text & 15);
        k_dump_text<<<dump_text_grid(a.text_bytes, mis, c->num_cus), 256, 0, s>>>(a);
    }
    k_dump_report<<<dump_lane_grid(a.count, c->num_cus), 256, 0, s>>>(a);
    return launch_status();
}

// the device buffers of one host call (freed when it ends)
struct DumpBufs {
    DevBuf ksrc, vsrc, klen, vlen, status, llen, koff, voff, out, report;
    ~DumpBufs() {
        for (DevBuf *q : {&ksrc, &vsrc, &klen, &vlen, &status, &llen, &koff, &voff, &out, &report}) q->free();
    }
    int grow(uint64_t nk) {
        int rc;
        if ((rc = ksrc.grow(8 * nk)) || (rc = vsrc.grow(8 * nk)) || (rc = klen.grow(4 * nk)) || (rc = vlen.grow(4 * nk)) ||
            (rc = status.grow(nk)) || (rc = koff.grow(8 * (nk + 1))) || (rc = voff.grow(8 * (nk + 1))))
            return rc;
        return BSDB_OK;
    }
    // two reports: [0] the call's, [1] one nobody reads (records seen again after a cut)
    unsigned long long *d_report(int i) const { return report.as<unsigned long long>() + i * DW_WORDS; }
    int zero_reports(hipStream_t s) {
        int rc;
        if ((rc = report.grow(2 * 8 * DW_WORDS))) return rc;
        HIP_OK(hipMemsetAsync(report.p, 0, 2 * 8 * DW_WORDS, s));
        for (int i = 0; i < 2; ++i) HIP_OK(hipMemsetAsync(d_report(i) + DW_FIRST_BAD, 0xFF, 8, s));
        return BSDB_OK;
    }
    RecordsArgs records(uint64_t first, uint64_t nk, int rep) const {
        return RecordsArgs{first, nk, ksrc.as<uint64_t>(), vsrc.as<uint64_t>(), klen.as<uint32_t>(), vlen.as<uint32_t>(),
                           status.as<uint8_t>(), d_report(rep)};
    }
};

void dump_empty_report(uint64_t *report) {
    memset(report, 0, sizeof(uint64_t) * BSDB_SCAN_WORDS);
    report[DW_FIRST_BAD] = DUMP_NONE;
}

DumpArgs dump_args(const bsdb_db *db, uint64_t count, const uint64_t *d_ksrc, const uint32_t *d_klen, const uint64_t *d_vsrc,
                   const uint32_t *d_vlen, uint8_t *d_status, uint32_t *d_llen, const uint64_t *d_loff, int sep, uint8_t *d_text,
                   uint64_t text_bytes, uint64_t first, unsigned long long *d_report) {
    DumpArgs a{};
    a.image = db->d_image;
    a.image_bytes = db->image_bytes;
    a.ksrc = d_ksrc, a.vsrc = d_vsrc;
    a.klen = d_klen, a.vlen = d_vlen;
    a.status = d_status;
    a.count = count;
    a.llen = d_llen;
    a.loff = d_loff;
    a.sep = (uint32_t)sep;
    a.text = d_text;
    a.text_bytes = text_bytes;
    a.first = first;
    a.out = d_report;
    return a;
}

int write_all(int fd, const uint8_t *p, uint64_t bytes) {
    while (bytes) {
        const ssize_t w = ::write(fd, p, (size_t)std::min<uint64_t>(bytes, 1ull << 30));
        if (w < 0 && errno == EINTR) continue;
        if (w <= 0) return BSDB_EFILE;
        p += w, bytes -= (uint64_t)w;
    }
    return BSDB_OK;
}

}  // namespace

extern "C" {

int bsdb_dev_db_records(bsdb_db *db, uint64_t first, uint64_t count, uint64_t *d_ksrc, uint32_t *d_klen, uint64_t *d_vsrc,
                        uint32_t *d_vlen, uint8_t *d_status, uint64_t *d_report, void *stream) {
    if (dump_bad_window(db, first, count) || !d_report || ((uintptr_t)d_report & 7) ||
        (count && (!d_ksrc || !d_klen || !d_vsrc || !d_vlen || !d_status)) || (((uintptr_t)d_ksrc | (uintptr_t)d_vsrc) & 7) ||
        (((uintptr_t)d_klen | (uintptr_t)d_vlen) & 3))
        return BSDB_EINVAL;
    bsdb_ctx *c = db_ctx(db);
    if (!c) return BSDB_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    HIP_OK(hipSetDevice(c->device));
    dump_records_launch(c, db, RecordsArgs{first, count, d_ksrc, d_vsrc, d_klen, d_vlen, d_status, (unsigned long long *)d_report},
                        pick(c, stream));
    return launch_status();
}

int bsdb_dev_db_dump_lengths(bsdb_db *db, uint64_t count, const uint32_t *d_klen, const uint32_t *d_vlen, uint8_t *d_status,
                             uint32_t *d_llen, uint64_t *d_loff, void *stream) {
    if (!db || db->approx || !d_loff || ((uintptr_t)d_loff & 7) || (count && (!d_klen || !d_vlen || !d_status || !d_llen)) ||
        (((uintptr_t)d_klen | (uintptr_t)d_vlen | (uintptr_t)d_llen) & 3))
        return BSDB_EINVAL;
    bsdb_ctx *c = db_ctx(db);
    if (!c) return BSDB_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    HIP_OK(hipSetDevice(c->device));
    hipStream_t s = pick(c, stream);
    Ordered ord(c, s);  // (the scan's block sums are the context's)
    return dump_lengths_launch(c, dump_args(db, count, nullptr, d_klen, nullptr, d_vlen, d_status, d_llen, d_loff, 0, nullptr, 0, 0, nullptr),
                               d_loff, s);
}

int bsdb_dev_db_dump_text(bsdb_db *db, uint64_t count, const uint64_t *d_ksrc, const uint32_t *d_klen, const uint64_t *d_vsrc,
                          const uint32_t *d_vlen, const uint32_t *d_llen, const uint64_t *d_loff, int separator, uint8_t *d_text,
                          uint64_t text_bytes, uint8_t *d_status, uint64_t first, uint64_t *d_report, void *stream) {
    if (!db || db->approx || text_bad_separator(separator) || !d_report || ((uintptr_t)d_report & 7) || (text_bytes && !d_text) ||
        (count && (!d_ksrc || !d_klen || !d_vsrc || !d_vlen || !d_llen || !d_loff || !d_status)) ||
        (((uintptr_t)d_ksrc | (uintptr_t)d_vsrc | (uintptr_t)d_loff) & 7) ||
        (((uintptr_t)d_klen | (uintptr_t)d_vlen | (uintptr_t)d_llen) & 3))
        return BSDB_EINVAL;
    bsdb_ctx *c = db_ctx(db);
    if (!c) return BSDB_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    HIP_OK(hipSetDevice(c->device));
    return dump_text_launch(c,
                            dump_args(db, count, d_ksrc, d_klen, d_vsrc, d_vlen, d_status, const_cast<uint32_t *>(d_llen), d_loff,
                                      separator, d_text, text_bytes, first, (unsigned long long *)d_report),
                            pick(c, stream));
}

int bsdb_db_set_text_chunk(bsdb_db *db, uint64_t bytes) {
    if (!db || db->approx || dump_bad_chunk(bytes)) return BSDB_EINVAL;
    bsdb_ctx *c = db_ctx(db);
    if (!c) return BSDB_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    db->text_chunk = bytes;
    return BSDB_OK;
}

int bsdb_db_scan(bsdb_db *db, uint64_t first, uint64_t count, uint64_t key_cap, uint64_t value_cap, uint8_t *h_keys,
                 uint64_t *h_koff, uint8_t *h_values, uint64_t *h_voff, uint8_t *h_status, uint64_t *report) {
    if (dump_bad_window(db, first, count) || !h_koff || !h_voff || !report || (count && !h_status) || (key_cap && !h_keys) ||
        (value_cap && !h_values))
        return BSDB_EINVAL;
    bsdb_ctx *c = db_ctx(db);
    if (!c) return BSDB_EINVAL;  // its MPHF was freed or its context closed
    h_koff[0] = h_voff[0] = 0;
    dump_empty_report(report);
    if (!count) return BSDB_OK;
    std::lock_guard<std::mutex> g(c->mu);
    HIP_OK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    Ordered ord(c, s);
    DumpBufs b;
    int rc = b.zero_reports(s);
    const uint64_t chunk = get_host_chunk(db->batch, 0);
    uint64_t ktotal = 0, vtotal = 0;
    // a chunk of slots: descriptors, the two scans, status and offsets to the host, then -- while they still fit
    // the caps -- the gathers and the chunk's keys and values to the host at the running offsets (as db_get)
    for (uint64_t k0 = 0; k0 < count && !rc; k0 += chunk) {
        const uint64_t nk = std::min(chunk, count - k0), k1 = k0 + nk;
        if ((rc = b.grow(nk))) break;
        const RecordsArgs a = b.records(first + k0, nk, 0);
        dump_records_launch(c, db, a, s);
        if ((rc = edge_offsets_impl(c, a.klen, nk, b.koff.as<uint64_t>(), s)) ||
            (rc = edge_offsets_impl(c, a.vlen, nk, b.voff.as<uint64_t>(), s)))
            break;
        HIP_OK(hipMemcpyAsync(h_status + k0, a.status, nk, hipMemcpyDeviceToHost, s));
        HIP_OK(hipMemcpyAsync(h_koff + k0, b.koff.p, (nk + 1) * 8, hipMemcpyDeviceToHost, s));
        HIP_OK(hipMemcpyAsync(h_voff + k0, b.voff.p, (nk + 1) * 8, hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));
        const uint64_t kb = h_koff[k1], vb = h_voff[k1];  // the chunk's offsets start at 0: stitched to the call's here
        for (uint64_t i = k0; i <= k1; ++i) h_koff[i] += ktotal, h_voff[i] += vtotal;
        struct Part { uint64_t bytes, total, cap; const uint64_t *src, *off; uint8_t *h; };
        for (const Part &p : {Part{kb, ktotal, key_cap, a.ksrc, b.koff.as<const uint64_t>(), h_keys},
                              Part{vb, vtotal, value_cap, a.vsrc, b.voff.as<const uint64_t>(), h_values}}) {
            if (!p.bytes || p.total + p.bytes > p.cap) continue;
            if ((rc = b.out.grow(p.bytes))) break;
            get_gather_launch(c, db, p.src, p.off, nk, b.out.as<uint8_t>(), p.bytes, s);
            HIP_OK(hipMemcpyAsync(p.h + p.total, b.out.p, p.bytes, hipMemcpyDeviceToHost, s));
            HIP_OK(hipStreamSynchronize(s));
        }
        ktotal += kb, vtotal += vb;
        if (!rc) rc = launch_status();
    }
    if (rc) {
        (void)hipStreamSynchronize(s);
        return rc;
    }
    HIP_OK(hipMemcpyAsync(report, b.d_report(0), sizeof(uint64_t) * DW_WORDS, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    return ktotal > key_cap || vtotal > value_cap ? BSDB_E2BIG : BSDB_OK;
}

int bsdb_db_dump_text(bsdb_db *db, const char *path, int separator, uint64_t first, uint64_t count, int append,
                      uint64_t *report) {
    if (dump_bad_window(db, first, count) || !path || text_bad_separator(separator) || !report) return BSDB_EINVAL;
    bsdb_ctx *c = db_ctx(db);
    if (!c) return BSDB_EINVAL;  // its MPHF was freed or its context closed
    dump_empty_report(report);
    Fd out;
    if ((out.fd = ::open(path, O_WRONLY | O_CREAT | (append ? O_APPEND : O_TRUNC), 0644)) < 0) return BSDB_EFILE;
    if (!count) return BSDB_OK;
    DumpBufs b;
    DevBuf &text = b.out;
    std::vector<uint64_t> hloff;
    std::vector<uint8_t> htext;
    uint64_t chunk = 0, cap = 0;
    {
        std::lock_guard<std::mutex> g(c->mu);
        HIP_OK(hipSetDevice(c->device));
        chunk = get_host_chunk(db->batch, 0);
        cap = dump_chunk_bytes(db->text_chunk);
        int rc = b.zero_reports(c->stream);
        if (rc) return rc;
        HIP_OK(hipStreamSynchronize(c->stream));
    }
    // A step: the descriptors and line lengths of up to `chunk` slots from r0, their scan to the host, the cut to
    // the text cap, the text of the records kept and its report; then the text goes to the file.  The records
    // after the cut are seen again by the next step (their first report is the one nobody reads).
    for (uint64_t r0 = first, end = first + count; r0 < end;) {
        const uint64_t nk = std::min(chunk, end - r0);
        uint64_t cut = 0, bytes = 0;
        {
            std::lock_guard<std::mutex> g(c->mu);
            HIP_OK(hipSetDevice(c->device));
            hipStream_t s = c->stream;
            Ordered ord(c, s);
            int rc;
            if ((rc = b.grow(nk)) || (rc = b.llen.grow(4 * nk))) return rc;
            try {
                hloff.resize(nk + 1);
            } catch (const std::bad_alloc &) {
                return BSDB_ENOMEM;
            }
            const RecordsArgs ra = b.records(r0, nk, 1);
            dump_records_launch(c, db, ra, s);
            DumpArgs a = dump_args(db, nk, ra.ksrc, ra.klen, ra.vsrc, ra.vlen, ra.status, b.llen.as<uint32_t>(),
                                   b.koff.as<const uint64_t>(), separator, nullptr, 0, r0, b.d_report(0));
            if ((rc = dump_lengths_launch(c, a, b.koff.as<uint64_t>(), s))) return rc;
            HIP_OK(hipMemcpyAsync(hloff.data(), b.koff.p, (nk + 1) * 8, hipMemcpyDeviceToHost, s));
            HIP_OK(hipStreamSynchronize(s));
            cut = dump_cut(hloff.data(), nk, cap);
            bytes = hloff[cut];
            if ((rc = text.grow(bytes))) return rc;
            try {
                htext.resize(bytes);
            } catch (const std::bad_alloc &) {
                return BSDB_ENOMEM;
            }
            a.count = cut;
            a.text = text.as<uint8_t>();
            a.text_bytes = bytes;
            if ((rc = dump_text_launch(c, a, s))) return rc;
            if (bytes) HIP_OK(hipMemcpyAsync(htext.data(), text.p, bytes, hipMemcpyDeviceToHost, s));
            HIP_OK(hipStreamSynchronize(s));
            if ((rc = launch_status())) return rc;
        }
        if (write_all(out.fd, htext.data(), bytes)) return BSDB_EFILE;
        r0 += cut;
    }
    std::lock_guard<std::mutex> g(c->mu);
    HIP_OK(hipSetDevice(c->device));
    HIP_OK(hipMemcpyAsync(report, b.d_report(0), sizeof(uint64_t) * DW_WORDS, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    return BSDB_OK;
}

}  // extern "C"
