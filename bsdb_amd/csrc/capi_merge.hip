// capi_merge.hip -- resident databases merged into a new directory behind the
// C ABI (kernels: merge_kernels.hip, plan: merge_plan.hpp).  Included by
// bsdb_capi.hip after capi_diff.hip.
//   bsdb_dev_db_merge_status   three status arrays -> the merge's status byte
//   bsdb_dev_db_pack           record descriptors of a resident image -> a kv.db image
//   bsdb_db_merge              base + delta - removed -> kv.db files + index files
// The reference has no merge.  Around the two new launches the pieces are the
// diff's (records, keys gathered, locate, select) and the text build's (the
// placement on sizes alone, pwrite per partition, builder_add_dev, finish).

namespace {

// whose records a pack reads: a resident image and the positions in it
struct RecSrc {
    const bsdb_db *db;
    const uint64_t *ksrc, *vsrc;
    unsigned long long *d_report;  // k_rec_sizes' counts (MW_WORDS), or null
};

TextPackIO rec_pack_io(const uint32_t *d_klen, const uint32_t *d_vlen, uint64_t count, int partitions, uint32_t B,
                       const uint64_t *h_part_size, uint8_t *d_image, uint64_t image_cap, uint64_t *h_run_bytes, uint64_t *d_addr,
                       uint8_t *d_blob, uint64_t blob_cap, uint64_t *d_off, uint64_t *h_blob_bytes, uint64_t *d_value8,
                       uint8_t *d_value_len) {
    return TextPackIO{nullptr, 0, {nullptr, d_klen, nullptr, d_vlen}, count, partitions, B, h_part_size, d_image, image_cap,
                      h_run_bytes, d_addr, d_blob, blob_cap, d_off, h_blob_bytes, d_value8, d_value_len, true};
}

bool rec_pack_bad_args(const RecSrc &r, const TextPackIO &io) {
    return diff_bad_db(r.db) || io.count > MERGE_MAX_COUNT || io.partitions < 1 || io.partitions > TEXT_MAX_PARTS ||
           !io.h_part_size || !io.h_run_bytes || (io.count && (!r.ksrc || !r.vsrc || !io.d.klen || !io.d.vlen)) ||
           (((uintptr_t)r.ksrc | (uintptr_t)r.vsrc) & 7) || (((uintptr_t)io.d.klen | (uintptr_t)io.d.vlen) & 3) ||
           (!io.d_blob != !io.d_off) || (!io.d_value8 != !io.d_value_len) ||
           (((uintptr_t)io.d_addr | (uintptr_t)io.d_off | (uintptr_t)io.d_value8) & 7);
}

// The pack of `count` records of a resident image; the caller holds the
// context's lock and has set the device.  text_pack_impl with the record
// kernels: the placement (shared, capi_text.hip) waits once, for the sizes.
int rec_pack_impl(bsdb_ctx *c, const RecSrc &r, const TextPackIO &io, hipStream_t s) {
    int rc;
    if ((rc = text_pack_empty(io, s)) || !io.count) return rc;
    TextPlacing pl;
    pl.sizes_report = r.d_report;
    if ((rc = text_place(c, io, pl, s))) return rc;
    RecPack pack{r.db->d_image, r.db->image_bytes, r.ksrc, r.vsrc, io.d.klen, io.d.vlen, io.count, nullptr, nullptr, 0};
    if (io.d_image && pl.image_bytes) {
        ProfScope ps(c, s, 6, io.count);  // (bsdb_set_profiling: the image pack alone, tools/merge_rate.py)
        const uint32_t grid = merge_pack_grid(pl.image_bytes, (uint32_t)((uintptr_t)io.d_image & 15), c->num_cus);
        pack.dst = io.d_image, pack.out_bytes = pl.image_bytes;
        if (io.B) {
            k_rec_pack_blocked<<<grid, 256, 0, s>>>(RecPackBlocked{pack, pl.PS, pl.PL, io.B});
        } else {
            pack.off = pl.roff;
            k_rec_pack<true><<<grid, 256, 0, s>>>(pack);
        }
    }
    if (io.d_blob && pl.blob_bytes) {
        pack.off = io.d_off, pack.dst = io.d_blob, pack.out_bytes = pl.blob_bytes;
        k_rec_pack<false><<<merge_pack_grid(pl.blob_bytes, (uint32_t)((uintptr_t)io.d_blob & 15), c->num_cus), 256, 0, s>>>(pack);
    }
    uint64_t *const d_addr = pl.roff ? io.d_addr : nullptr;  // (the blocked addresses are k_blk_place's)
    if (d_addr || io.d_value8)
        k_rec_outputs<<<pl.lgrid, 256, 0, s>>>(pl.runs, r.db->d_image, r.db->image_bytes, r.vsrc, io.d.vlen, pl.roff, io.count, d_addr,
                                                io.d_value8, io.d_value_len);
    return text_pack_done(io, pl);
}

void merge_status_launch(bsdb_ctx *c, const MergeStatusArgs &a, hipStream_t s) {
    if (a.count) k_merge_status<<<merge_lane_grid(a.count, c->num_cus), 256, 0, s>>>(a);
}

// the device buffers of one bsdb_db_merge call (freed when it ends)
struct MergeBufs {
    DevBuf ksrc, vsrc, klen, vlen, st_a, koff, keys;  // a chunk of the side that is listed: descriptors, packed keys
    DevBuf src_b, vlen_b, st_d, st_r, status;         // locate's answers (positions and lengths: nobody reads them); the merge's status
    DevBuf sel, ksrc_o, vsrc_o, klen_o, vlen_o;       // the selection
    DevBuf csize, coff;                               // the cut: the selection's sizes and their scan
    DevBuf image, blob, off, addr, v8, vl;            // a pack's outputs
    DevBuf report;
    ~MergeBufs() {
        for (DevBuf *q : {&ksrc, &vsrc, &klen, &vlen, &st_a, &koff, &keys, &src_b, &vlen_b, &st_d, &st_r, &status, &sel, &ksrc_o,
                          &vsrc_o, &klen_o, &vlen_o, &csize, &coff, &image, &blob, &off, &addr, &v8, &vl, &report})
            q->free();
    }
    int grow(uint64_t nk, bool approximate) {
        int rc;
        for (DevBuf *q : {&ksrc, &vsrc, &src_b, &sel, &ksrc_o, &vsrc_o, &addr, &csize})
            if ((rc = q->grow(8 * nk))) return rc;
        for (DevBuf *q : {&klen, &vlen, &vlen_b, &klen_o, &vlen_o})
            if ((rc = q->grow(4 * nk))) return rc;
        for (DevBuf *q : {&st_a, &st_d, &st_r, &status})
            if ((rc = q->grow(nk))) return rc;
        for (DevBuf *q : {&koff, &coff, &off})
            if ((rc = q->grow(8 * (nk + 1)))) return rc;
        if (approximate && ((rc = v8.grow(8 * nk)) || (rc = vl.grow(nk)))) return rc;
        return BSDB_OK;
    }
    // the reports on the device: the merge's, the records' and locate's (nobody reads those two), nsel
    unsigned long long *d_merge() const { return report.as<unsigned long long>(); }
    unsigned long long *d_records() const { return d_merge() + MW_WORDS; }
    unsigned long long *d_get() const { return d_records() + DW_WORDS; }
    uint64_t *d_nsel() const { return (uint64_t *)(d_get() + GW_WORDS); }
    static constexpr size_t WORDS = MW_WORDS + DW_WORDS + GW_WORDS + 1;
    int zero_reports(hipStream_t s) {
        int rc;
        if ((rc = report.grow(8 * WORDS))) return rc;
        HIP_OK(hipMemsetAsync(report.p, 0, 8 * WORDS, s));
        return BSDB_OK;
    }
};

// What one bsdb_db_merge call keeps from chunk to chunk.
struct MergeRun {
    bsdb_ctx *c;
    bsdb_db *base, *delta, *removed;
    int partitions;
    uint32_t B;  // TextPackIO's
    bool approximate;
    bsdb_builder *builder;
    Fd part[TEXT_MAX_PARTS];
    uint64_t part_size[TEXT_MAX_PARTS] = {};
    MergeBufs b;
    std::vector<uint64_t> hroff;
    std::vector<uint8_t> himg;
};

// Slots [r0, r0 + nk) of `side` listed, and -- for base -- their keys packed
// and located in delta and in removed; the status, the KEPT records selected
// in slot order, and the scan of their sizes to the host (m.hroff): what the
// chunk's packs are cut by.  Under the context's lock.
int merge_select_step(MergeRun &m, bsdb_db *side, uint64_t r0, uint64_t nk, uint64_t &nsel) {
    bsdb_ctx *c = m.c;
    MergeBufs &b = m.b;
    std::lock_guard<std::mutex> g(c->mu);
    HIP_OK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    Ordered ord(c, s);
    int rc;
    if ((rc = b.grow(nk, m.approximate))) return rc;
    const RecordsArgs ra{r0, nk, b.ksrc.as<uint64_t>(), b.vsrc.as<uint64_t>(), b.klen.as<uint32_t>(), b.vlen.as<uint32_t>(),
                         b.st_a.as<uint8_t>(), b.d_records()};
    dump_records_launch(c, side, ra, s);
    const bool is_base = side == m.base;
    const bool lookups = is_base && (m.delta || m.removed);
    if (lookups) {
        if ((rc = edge_offsets_impl(c, ra.klen, nk, b.koff.as<uint64_t>(), s))) return rc;
        uint64_t key_bytes = 0;
        HIP_OK(hipMemcpyAsync(&key_bytes, b.koff.as<uint64_t>() + nk, 8, hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));
        if ((rc = b.keys.grow(key_bytes + 16))) return rc;
        get_gather_launch(c, side, ra.ksrc, b.koff.as<const uint64_t>(), nk, b.keys.as<uint8_t>(), key_bytes, s);
        GetArgs ga{};
        ga.keys = b.keys.as<const uint8_t>();
        ga.off = b.koff.as<const uint64_t>();
        ga.blob_bytes = key_bytes;
        ga.nq = nk;
        ga.src = b.src_b.as<uint64_t>();
        ga.vlen = b.vlen_b.as<uint32_t>();
        ga.out = b.d_get();
        if (m.delta) {
            ga.status = b.st_d.as<uint8_t>();
            get_locate_launch(c, m.delta, ga, s);
        }
        if (m.removed) {
            ga.status = b.st_r.as<uint8_t>();
            get_locate_launch(c, m.removed, ga, s);
        }
    }
    MergeStatusArgs ma{};
    ma.status_base = ra.status;
    ma.status_delta = lookups && m.delta ? b.st_d.as<const uint8_t>() : nullptr;
    ma.status_removed = lookups && m.removed ? b.st_r.as<const uint8_t>() : nullptr;
    ma.status = b.status.as<uint8_t>();
    ma.count = nk;
    ma.delta_side = is_base ? 0 : 1;
    ma.out = b.d_merge();
    merge_status_launch(c, ma, s);
    SelectArgs sa{};
    sa.status = ma.status;
    sa.count = nk;
    sa.mask = MERGE_MASK_KEPT;
    sa.ksrc = ra.ksrc, sa.vsrc = ra.vsrc, sa.klen = ra.klen, sa.vlen = ra.vlen;
    sa.sel = b.sel.as<uint64_t>();
    sa.ksrc_out = b.ksrc_o.as<uint64_t>(), sa.vsrc_out = b.vsrc_o.as<uint64_t>();
    sa.klen_out = b.klen_o.as<uint32_t>(), sa.vlen_out = b.vlen_o.as<uint32_t>();
    sa.nsel = b.d_nsel();
    if ((rc = select_launch(c, sa, s))) return rc;
    HIP_OK(hipMemcpyAsync(&nsel, b.d_nsel(), 8, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    if ((rc = launch_status())) return rc;
    if (nsel > nk) return BSDB_EIO;
    try {
        m.hroff.assign(nsel + 1, 0);
    } catch (const std::bad_alloc &) {
        return BSDB_ENOMEM;
    }
    if (!nsel) return BSDB_OK;
    uint32_t *rsize = b.csize.as<uint32_t>();
    k_rec_sizes<<<merge_lane_grid(nsel, c->num_cus), 256, 0, s>>>(sa.klen_out, sa.vlen_out, nsel, 0, rsize, rsize + nsel, nullptr, nullptr);
    if ((rc = edge_offsets_impl(c, rsize, nsel, b.coff.as<uint64_t>(), s))) return rc;
    HIP_OK(hipMemcpyAsync(m.hroff.data(), b.coff.p, (nsel + 1) * 8, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    return launch_status();
}

// The selection's n records from p0 on: the cut to the cap, and the pack of
// the records before the cut behind the files as they are; the image comes
// back into m.himg.  Under the context's lock.
int merge_pack_step(MergeRun &m, bsdb_db *side, uint64_t p0, uint64_t n, uint64_t record_cap, uint64_t *run_bytes, uint64_t &cut) {
    bsdb_ctx *c = m.c;
    MergeBufs &b = m.b;
    std::lock_guard<std::mutex> g(c->mu);
    HIP_OK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    Ordered ord(c, s);
    int rc;
    const uint32_t *klen = b.klen_o.as<const uint32_t>() + p0, *vlen = b.vlen_o.as<const uint32_t>() + p0;
    cut = merge_cut(m.hroff.data() + p0, n, record_cap);
    const uint64_t record_bytes = m.hroff[p0 + cut] - m.hroff[p0];
    if (record_bytes > cut * (uint64_t)MERGE_MAX_RECORD) return BSDB_EIO;  // (a scan that is none)
    const uint64_t image_max = merge_image_max(record_bytes, m.partitions, m.B), blob_max = std::min(record_bytes, cut * TEXT_MAX_KEY) + 16;
    if ((rc = b.image.grow(image_max)) || (rc = b.blob.grow(blob_max))) return rc;
    const RecSrc src{side, b.ksrc_o.as<const uint64_t>() + p0, b.vsrc_o.as<const uint64_t>() + p0, b.d_merge()};
    const TextPackIO io = rec_pack_io(klen, vlen, cut, m.partitions, m.B, m.part_size, b.image.as<uint8_t>(), image_max, run_bytes,
                                      b.addr.as<uint64_t>(), b.blob.as<uint8_t>(), blob_max, b.off.as<uint64_t>(), nullptr,
                                      m.approximate ? b.v8.as<uint64_t>() : nullptr, m.approximate ? b.vl.as<uint8_t>() : nullptr);
    if ((rc = rec_pack_impl(c, src, io, s))) return rc;
    uint64_t image_bytes = 0;
    for (int p = 0; p < m.partitions; ++p) image_bytes += run_bytes[p];
    try {
        if (m.himg.size() < image_bytes) m.himg.resize(image_bytes);
    } catch (const std::bad_alloc &) {
        return BSDB_ENOMEM;
    }
    if (image_bytes) HIP_OK(hipMemcpyAsync(m.himg.data(), b.image.p, image_bytes, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    return launch_status();
}

// Every slot of `side` in chunks: select, then pack after pack the image's
// runs appended to their files and the records added to the builder.  After
// each chunk the report comes back: a damaged input ends the call there.
int merge_side(MergeRun &m, bsdb_db *side, uint64_t *report) {
    bsdb_ctx *c = m.c;
    uint64_t chunk = 0, record_cap = 0;
    {
        std::lock_guard<std::mutex> g(c->mu);
        chunk = get_host_chunk(side->batch, 0);
        record_cap = merge_record_cap(dump_chunk_bytes(side->text_chunk), m.partitions, m.B);
    }
    const MergeBufs &b = m.b;
    for (uint64_t r0 = 0, n = side->n; r0 < n; r0 += chunk) {
        uint64_t nsel = 0;
        int rc = merge_select_step(m, side, r0, std::min(chunk, n - r0), nsel);
        for (uint64_t p0 = 0; !rc && p0 < nsel;) {
            uint64_t run_bytes[TEXT_MAX_PARTS] = {}, cut = 0;
            if ((rc = merge_pack_step(m, side, p0, nsel - p0, record_cap, run_bytes, cut))) break;
            // the image's runs lie back to back: P plain copies, each appended to its file
            uint64_t at = 0;
            for (int p = 0; p < m.partitions && !rc; ++p) {
                if (!write_all(m.part[p].fd, m.himg.data() + at, run_bytes[p], m.part_size[p])) rc = BSDB_EFILE;
                at += run_bytes[p];
                m.part_size[p] += run_bytes[p];
            }
            if (!rc)
                rc = builder_add_dev(m.builder, b.blob.as<const uint8_t>(), b.off.as<const uint64_t>(), cut, b.addr.as<const uint64_t>(),
                                     m.approximate ? b.v8.as<const uint64_t>() : nullptr,
                                     m.approximate ? b.vl.as<const uint8_t>() : nullptr, c->stream);
            p0 += cut;
        }
        std::lock_guard<std::mutex> g(c->mu);
        if (rc) {
            (void)hipStreamSynchronize(c->stream);
            return rc;
        }
        HIP_OK(hipSetDevice(c->device));
        HIP_OK(hipMemcpyAsync(report, b.d_merge(), sizeof(uint64_t) * MW_WORDS, hipMemcpyDeviceToHost, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
        if (report[MW_BAD_SLOT] || report[MW_BAD_ADDR] || report[MW_DELTA_BAD_SLOT]) return BSDB_EVERIFY;
    }
    return BSDB_OK;
}

}  // namespace

extern "C" {

int bsdb_dev_db_merge_status(bsdb_ctx *c, uint64_t count, const uint8_t *d_status_base, const uint8_t *d_status_delta,
                             const uint8_t *d_status_removed, uint8_t *d_status_out, uint64_t *d_report, void *stream) {
    if (!c || count > MERGE_MAX_COUNT || !d_report || ((uintptr_t)d_report & 7) || (count && (!d_status_base || !d_status_out)))
        return BSDB_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    HIP_OK(hipSetDevice(c->device));
    MergeStatusArgs a{};
    a.status_base = d_status_base;
    a.status_delta = d_status_delta;
    a.status_removed = d_status_removed;
    a.status = d_status_out;
    a.count = count;
    a.out = (unsigned long long *)d_report;
    merge_status_launch(c, a, pick(c, stream));
    return launch_status();
}

int bsdb_dev_db_pack(bsdb_ctx *c, bsdb_db *db, const uint64_t *d_ksrc, const uint32_t *d_klen, const uint64_t *d_vsrc,
                     const uint32_t *d_vlen, uint64_t count, int partitions, int format, uint32_t block_size,
                     const uint64_t *h_part_size, uint8_t *d_image, uint64_t image_cap, uint64_t *h_run_bytes, uint64_t *d_addr,
                     uint8_t *d_blob, uint64_t blob_cap, uint64_t *d_off, uint64_t *h_blob_bytes, uint64_t *d_value8,
                     uint8_t *d_value_len, void *stream) {
    if (!c || (format != 0 && format != 1) || (format == 1 && text_bad_block_size(block_size))) return BSDB_EINVAL;
    const RecSrc r{db, d_ksrc, d_vsrc, nullptr};
    const TextPackIO io = rec_pack_io(d_klen, d_vlen, count, partitions, format == 1 ? block_size : 0, h_part_size, d_image, image_cap,
                                      h_run_bytes, d_addr, d_blob, blob_cap, d_off, h_blob_bytes, d_value8, d_value_len);
    if (rec_pack_bad_args(r, io) || db_ctx(db) != c) return BSDB_EINVAL;  // (an MPHF freed, or another context's database)
    for (int p = 0; format == 1 && p < partitions; ++p)
        if ((h_part_size[p] & (TEXT_PAGE - 1)) || h_part_size[p] > TEXT_MAX_FILE_BLOCKED) return BSDB_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    HIP_OK(hipSetDevice(c->device));
    hipStream_t s = pick(c, stream);
    Ordered ord(c, s);
    return rec_pack_impl(c, r, io, s);
}

int bsdb_db_merge(bsdb_db *base, bsdb_db *delta, bsdb_db *removed, const char *kv_base, int partitions, int format,
                  uint32_t block_size, uint32_t width, int approximate, const char *index_path, const char *index_a_path,
                  uint64_t *report, bsdb_mph **out) {
    if (diff_bad_db(base) || (delta && diff_bad_db(delta)) || (removed && diff_bad_db(removed)) || !kv_base || partitions < 1 ||
        partitions > TEXT_MAX_PARTS || (format != 0 && format != 1) || (format == 1 && text_bad_block_size(block_size)) ||
        width > 64 || !index_path || (approximate && !index_a_path) || !report || !out)
        return BSDB_EINVAL;
    bsdb_ctx *c = db_ctx(base);
    if (!c || (delta && db_ctx(delta) != c) || (removed && db_ctx(removed) != c)) return BSDB_EINVAL;  // freed, closed, or two contexts
    *out = nullptr;
    memset(report, 0, sizeof(uint64_t) * BSDB_MERGE_WORDS);
    MergeRun m{c, base, delta, removed, partitions, format == 1 ? block_size : 0, approximate != 0, nullptr};
    for (int p = 0; p < partitions; ++p) {
        const std::string path = std::string(kv_base) + "." + std::to_string(p);
        if ((m.part[p].fd = ::open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644)) < 0) return BSDB_EFILE;
    }
    int rc;
    {
        std::lock_guard<std::mutex> g(c->mu);
        HIP_OK(hipSetDevice(c->device));
        if ((rc = m.b.zero_reports(c->stream))) return rc;
        HIP_OK(hipStreamSynchronize(c->stream));
    }
    const uint64_t most = base->n + (delta ? delta->n : 0);
    if ((rc = bsdb_builder_open(c, 0, most + 1024, 16 * most + 65536, approximate, 0, 0, &m.builder))) return rc;
    struct BuilderGuard {
        bsdb_builder *b;
        ~BuilderGuard() { (void)bsdb_builder_free(b); }
    } guard{m.builder};
    if ((rc = merge_side(m, base, report))) return rc;
    if (delta && (rc = merge_side(m, delta, report))) return rc;
    for (int p = 0; p < partitions; ++p) {
        const int fd = m.part[p].fd;
        m.part[p].fd = -1;
        if (close(fd) != 0) return BSDB_EFILE;
    }
    return bsdb_builder_finish(m.builder, width, 0, index_path, index_a_path, out, nullptr);
}

}  // extern "C"
