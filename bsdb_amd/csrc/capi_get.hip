// capi_get.hip -- batched get behind the C ABI (kernels: get_kernels.hip, plan:
// get_plan.hpp).  Included by bsdb_capi.hip after capi_verify.hip.
//   bsdb_db_open / info / set_batch / free   a database resident on the device
//   bsdb_db_get_*                            keys in host memory -> packed values
//   bsdb_dev_db_locate_* / bsdb_dev_db_gather  the two kernels on device buffers
// What SyncReader.getAsBytes (read/SyncReader.java:44-57) does one key per
// call.  A bsdb_db borrows its MPHF as a bsdb_index does: freeing the MPHF or
// closing its context detaches the db (calls return BSDB_EINVAL, free is safe).

namespace {

// The context a db works on, or nullptr when its MPHF was freed or the MPHF's
// context was closed.
bsdb_ctx *db_ctx(const bsdb_db *db) {
    std::lock_guard<std::mutex> lg(g_life_mu);
    return db->mph ? db->mph->c : nullptr;
}

MphView db_mph_view(const bsdb_db *db) {
    const bsdb_mph *p = db->mph;
    return MphView{p->E, p->values, p->sigbits, p->n, (uint32_t)(2 * p->m), p->width};
}

GetDb db_view(const bsdb_db *db) {
    GetDb g{};
    g.image = db->d_image;
    g.image_bytes = db->image_bytes;
    g.index = db->d_index;
    g.base = db->d_table;
    g.size = db->d_table + db->partitions;
    g.partitions = (uint32_t)db->partitions;
    g.format = db->format;
    g.approx = db->approx ? 1 : 0;
    return g;
}

void get_locate_launch(bsdb_ctx *c, const bsdb_db *db, const GetArgs &a, hipStream_t s) {
    if (!a.nq) return;
    const uint32_t grid = get_locate_grid(a.nq, c->num_cus);
    const MphView v = db_mph_view(db);
    const GetDb g = db_view(db);
    if (a.off)
        k_get_locate<2><<<grid, 256, 0, s>>>(v, g, a);
    else if (a.key_len == 13)
        k_get_locate<0><<<grid, 256, 0, s>>>(v, g, a);
    else
        k_get_locate<1><<<grid, 256, 0, s>>>(v, g, a);
}

void get_gather_launch(bsdb_ctx *c, const bsdb_db *db, const uint64_t *d_src, const uint64_t *d_voff, uint64_t nq,
                       uint8_t *d_values, uint64_t value_bytes, hipStream_t s) {
    if (!nq || !value_bytes) return;
    GatherArgs a{};
    a.image = db->d_image;
    a.image_bytes = db->image_bytes;
    a.scale = db->approx ? 8 : 1;
    a.src = d_src;
    a.voff = d_voff;
    a.nq = nq;
    a.values = d_values;
    a.value_bytes = value_bytes;
    const uint32_t mis = (uint32_t)((uintptr_t)d_values & 15);
    k_get_gather<<<piece_grid(value_bytes, mis, c->num_cus), 256, 0, s>>>(a);
}

// Releases a db's device memory on its own device (its context may be gone).
void db_destroy(bsdb_db *db, bsdb_ctx *c) {
    if (db->d_image || db->d_index || db->d_table || db->d_report) {
        if (c) {
            std::lock_guard<std::mutex> g(c->mu);
            (void)hipSetDevice(c->device);
            (void)hipStreamSynchronize(c->stream);
        } else {
            (void)hipSetDevice(db->device);
            (void)hipDeviceSynchronize();
        }
        (void)hipFree(db->d_image);
        (void)hipFree(db->d_index);
        (void)hipFree(db->d_table);
        (void)hipFree(db->d_report);
    }
    delete db;
}

struct Fd {
    int fd = -1;
    ~Fd() {
        if (fd >= 0) close(fd);
    }
};

// The files into device memory; the caller holds c->mu and has set the device.
int db_load(bsdb_db *db, bsdb_ctx *c, const char *kv_base, const char *index_path) {
    bsdb_mph *p = db->mph;
    const uint64_t n = p->n;
    Fd ix;
    struct stat st;
    if ((ix.fd = ::open(index_path, O_RDONLY)) < 0 || fstat(ix.fd, &st) != 0) return BSDB_EFILE;
    if ((uint64_t)st.st_size != 8 * n) return BSDB_EVERIFY;  // (verify's flag bit 1)
    uint64_t table[2 * GET_MAX_PARTS] = {};
    Fd part[GET_MAX_PARTS];
    GetLayout lay;
    if (!db->approx) {
        uint64_t *sizes = table + db->partitions;
        for (int pi = 0; pi < db->partitions; ++pi) {
            const std::string path = std::string(kv_base) + "." + std::to_string(pi);
            if ((part[pi].fd = ::open(path.c_str(), O_RDONLY)) < 0 || fstat(part[pi].fd, &st) != 0) return BSDB_EFILE;
            sizes[pi] = (uint64_t)st.st_size;
        }
        lay = get_layout(sizes, db->partitions);
        if (!lay.ok) return BSDB_EINVAL;
        for (int pi = 0; pi < db->partitions; ++pi) table[pi] = lay.base[pi];
    }
    // E first: only a valid E keeps every lookup inside values[] (an imported hash.dump is untrusted)
    if (dmalloc(&db->d_report, BSDB_VERIFY_WORDS * 8) != hipSuccess) return BSDB_ENOMEM;
    HIP_OK(hipMemsetAsync(db->d_report, 0, BSDB_VERIFY_WORDS * 8, c->stream));
    k_verify_structure<<<grid_for(c->num_cus, p->m + 1), 256, 0, c->stream>>>(p->E, p->m, n, db->d_report);
    int rc = launch_status();
    if (rc) return rc;
    uint64_t flags = 0;
    HIP_OK(hipMemcpyAsync(&flags, db->d_report + VW_FLAGS, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    if (flags & 1) return BSDB_EVERIFY;
    HIP_OK(hipMemsetAsync(db->d_report, 0, BSDB_VERIFY_WORDS * 8, c->stream));
    size_t free_b = 0, total_b = 0;
    HIP_OK(hipMemGetInfo(&free_b, &total_b));
    if (!get_open_fits(lay.total, n, db->approx, free_b)) return BSDB_ENOMEM;
    if (db->approx) {
        db->image_bytes = 8 * n;
        if (dmalloc(&db->d_image, std::max<uint64_t>(db->image_bytes, 16)) != hipSuccess) return BSDB_ENOMEM;
        return load_slots(ix.fd, 0, db->d_image, db->image_bytes, c->stream);
    }
    db->image_bytes = lay.total;
    if (dmalloc(&db->d_image, std::max<uint64_t>(lay.total, 16)) != hipSuccess ||
        dmalloc(&db->d_index, std::max<uint64_t>(8 * n, 8)) != hipSuccess ||
        dmalloc(&db->d_table, sizeof(uint64_t) * 2 * db->partitions) != hipSuccess)
        return BSDB_ENOMEM;
    HIP_OK(hipMemcpyAsync(db->d_table, table, sizeof(uint64_t) * 2 * db->partitions, hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));  // (table is a stack buffer)
    if ((rc = load_slots(ix.fd, 0, db->d_index, 8 * n, c->stream))) return rc;
    for (int pi = 0; pi < db->partitions; ++pi)
        if ((rc = load_slots(part[pi].fd, 0, db->d_image + lay.base[pi], table[db->partitions + pi], c->stream))) return rc;
    return BSDB_OK;
}

// Keys in host memory (var-len when h_off, else key_len bytes each), a chunk
// at a time through the feed slots: locate, scan, the chunk's status and
// offsets to the host, then -- while the values still fit value_cap -- gather
// and the chunk's values to the host at the running offset.
int db_get(bsdb_db *db, const uint8_t *h_keys, uint32_t key_len, const uint64_t *h_off, uint64_t nq, uint64_t value_cap,
           uint8_t *h_values, uint64_t *h_voff, uint8_t *h_status, uint64_t *report) {
    bsdb_ctx *c = db_ctx(db);
    if (!c) return BSDB_EINVAL;  // its MPHF was freed or its context closed
    std::lock_guard<std::mutex> g(c->mu);
    HIP_OK(hipSetDevice(c->device));
    Ordered ord(c, c->stream);
    h_voff[0] = 0;
    memset(report, 0, sizeof(uint64_t) * BSDB_GET_WORDS);
    if (!nq) return BSDB_OK;
    HIP_OK(hipMemsetAsync(db->d_report, 0, sizeof(uint64_t) * GW_WORDS, c->stream));
    const uint64_t chunk = get_host_chunk(db->batch, key_len);
    uint64_t total = 0;
    int rc = feed_batches(
        c, nq,
        [&](uint64_t k0) {
            const uint64_t k1 = std::min(nq, k0 + chunk);
            return h_off ? std::min(k1, var_batch_end(h_off, k0, nq)) : k1;
        },
        [&](FeedSlot &f, uint64_t k0, uint64_t k1) {
            return h_off ? upload_var(c, f, h_keys, h_off, k0, k1) : upload_fixed(c, f, h_keys, key_len, k0, k1);
        },
        [&](FeedSlot &f, uint64_t k0, uint64_t k1) {
            const uint64_t nk = k1 - k0;
            int r2;
            if ((r2 = f.buf[2].grow(nk * 8)) || (r2 = f.buf[3].grow(nk * 4)) || (r2 = f.buf[4].grow(nk)) ||
                (r2 = f.buf[5].grow((nk + 1) * 8)))
                return r2;
            GetArgs a{};
            a.keys = f.buf[0].as<const uint8_t>();
            a.off = h_off ? f.buf[1].as<const uint64_t>() : nullptr;
            a.blob_bytes = h_off ? h_off[k1] - h_off[k0] : nk * key_len;
            a.nq = nk;
            a.key_len = key_len;
            a.src = f.buf[2].as<uint64_t>();
            a.vlen = f.buf[3].as<uint32_t>();
            a.status = f.buf[4].as<uint8_t>();
            a.out = db->d_report;
            get_locate_launch(c, db, a, c->stream);
            if ((r2 = edge_offsets_impl(c, a.vlen, nk, f.buf[5].as<uint64_t>(), c->stream))) return r2;
            HIP_OK(hipMemcpyAsync(h_status + k0, a.status, nk, hipMemcpyDeviceToHost, c->stream));
            HIP_OK(hipMemcpyAsync(h_voff + k0, f.buf[5].p, (nk + 1) * 8, hipMemcpyDeviceToHost, c->stream));
            HIP_OK(hipStreamSynchronize(c->stream));
            const uint64_t bytes = h_voff[k1];  // the chunk's offsets start at 0: stitched to the call's here
            if (total)
                for (uint64_t i = k0; i <= k1; ++i) h_voff[i] += total;
            if (bytes && total + bytes <= value_cap) {
                if ((r2 = f.buf[6].grow(bytes))) return r2;
                get_gather_launch(c, db, a.src, f.buf[5].as<const uint64_t>(), nk, f.buf[6].as<uint8_t>(), bytes, c->stream);
                HIP_OK(hipMemcpyAsync(h_values + total, f.buf[6].p, bytes, hipMemcpyDeviceToHost, c->stream));
                HIP_OK(hipStreamSynchronize(c->stream));
            }
            total += bytes;
            return launch_status();
        });
    if (rc) {
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    HIP_OK(hipMemcpyAsync(report, db->d_report, sizeof(uint64_t) * GW_WORDS, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    return total > value_cap ? BSDB_E2BIG : BSDB_OK;
}

int dev_db_locate(bsdb_db *db, const uint8_t *d_keys, const uint64_t *d_off, uint64_t blob_bytes, uint32_t key_len,
                  uint64_t nq, uint64_t *d_src, uint32_t *d_vlen, uint8_t *d_status, uint64_t *d_report, void *stream) {
    if (!db || !d_report || ((uintptr_t)d_report & 7) || (nq && (!d_keys || !d_src || !d_vlen || !d_status)) ||
        ((uintptr_t)d_src & 7) || ((uintptr_t)d_vlen & 3))
        return BSDB_EINVAL;
    bsdb_ctx *c = db_ctx(db);
    if (!c) return BSDB_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    HIP_OK(hipSetDevice(c->device));
    GetArgs a{};
    a.keys = d_keys;
    a.off = d_off;
    a.blob_bytes = blob_bytes;
    a.nq = nq;
    a.key_len = key_len;
    a.src = d_src;
    a.vlen = d_vlen;
    a.status = d_status;
    a.out = (unsigned long long *)d_report;
    get_locate_launch(c, db, a, pick(c, stream));
    return launch_status();
}

}  // namespace

extern "C" {

int bsdb_db_open(bsdb_mph *p, const char *kv_base, int partitions, int format, uint32_t block_size, int approximate,
                 const char *index_path, bsdb_db **out) {
    if (p && !p->c) return BSDB_EINVAL;  // its context was closed
    if (!p || !out || !index_path ||
        (!approximate && (!kv_base || partitions < 1 || partitions > GET_MAX_PARTS || (format != 0 && format != 1) ||
                          (format == 1 && (block_size == 0 || block_size % KV_PAGE)))))
        return BSDB_EINVAL;
    *out = nullptr;
    bsdb_db *db = new (std::nothrow) bsdb_db();
    if (!db) return BSDB_ENOMEM;
    db->mph = p;
    db->device = p->device;
    db->approx = approximate != 0;
    db->partitions = db->approx ? 0 : partitions;
    db->format = db->approx ? 0 : format;
    db->block_size = db->approx ? 0 : block_size;
    db->n = p->n;
    {
        std::lock_guard<std::mutex> lg(g_life_mu);
        p->dbs.push_back(db);
    }
    bsdb_ctx *c = p->c;
    int rc;
    {
        std::lock_guard<std::mutex> g(c->mu);
        rc = hipSetDevice(c->device) == hipSuccess ? BSDB_OK : BSDB_EIO;
        if (!rc) {
            Ordered ord(c, c->stream);
            rc = db_load(db, c, kv_base, index_path);
            if (rc) (void)hipStreamSynchronize(c->stream);
        }
    }
    if (rc) {
        (void)bsdb_db_free(db);  // (takes the context lock itself)
        return rc;
    }
    *out = db;
    return BSDB_OK;
}

int bsdb_db_info(const bsdb_db *db, uint64_t *out) {
    if (!db || !out) return BSDB_EINVAL;
    const uint64_t w[BSDB_DB_INFO_WORDS] = {db->n, (uint64_t)db->partitions, (uint64_t)db->format, db->block_size,
                                            db->approx ? 1u : 0u, db->image_bytes, db->approx ? 0 : 8 * db->n,
                                            get_host_chunk(db->batch, 0)};
    memcpy(out, w, sizeof(w));
    return BSDB_OK;
}

int bsdb_db_set_batch(bsdb_db *db, uint64_t max_queries) {
    if (!db) return BSDB_EINVAL;
    bsdb_ctx *c = db_ctx(db);
    if (!c) return BSDB_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    db->batch = max_queries;
    return BSDB_OK;
}

int bsdb_db_get_fixed(bsdb_db *db, const uint8_t *h_keys, uint32_t key_len, uint64_t nq, uint64_t value_cap,
                      uint8_t *h_values, uint64_t *h_voff, uint8_t *h_status, uint64_t *report) {
    if (!db || bad_key_len(key_len) || !h_voff || !report || (nq && (!h_keys || !h_status)) || (value_cap && !h_values))
        return BSDB_EINVAL;
    return db_get(db, h_keys, key_len, nullptr, nq, value_cap, h_values, h_voff, h_status, report);
}

int bsdb_db_get_var(bsdb_db *db, const uint8_t *h_blob, const uint64_t *h_off, uint64_t nq, uint64_t value_cap,
                    uint8_t *h_values, uint64_t *h_voff, uint8_t *h_status, uint64_t *report) {
    if (!db || !h_voff || !report || (nq && (!h_blob || !h_off || !h_status)) || (value_cap && !h_values))
        return BSDB_EINVAL;
    static const uint64_t zero_off[1] = {0};
    return db_get(db, h_blob, 0, nq ? h_off : zero_off, nq, value_cap, h_values, h_voff, h_status, report);
}

int bsdb_db_free(bsdb_db *db) {
    if (!db) return BSDB_EINVAL;
    bsdb_ctx *c = nullptr;
    {
        std::lock_guard<std::mutex> lg(g_life_mu);
        if (db->mph) {
            auto &v = db->mph->dbs;
            v.erase(std::remove(v.begin(), v.end(), db), v.end());
            c = db->mph->c;
        }
    }
    db_destroy(db, c);
    return BSDB_OK;
}

int bsdb_dev_db_locate_fixed(bsdb_db *db, const uint8_t *d_keys, uint32_t key_len, uint64_t nq, uint64_t *d_src,
                             uint32_t *d_vlen, uint8_t *d_status, uint64_t *d_report, void *stream) {
    if (bad_key_len(key_len) || ((uintptr_t)d_keys & 3)) return BSDB_EINVAL;  // (the key readers load dwords)
    return dev_db_locate(db, d_keys, nullptr, nq * key_len, key_len, nq, d_src, d_vlen, d_status, d_report, stream);
}

int bsdb_dev_db_locate_var(bsdb_db *db, const uint8_t *d_blob, uint64_t blob_bytes, const uint64_t *d_off, uint64_t nq,
                           uint64_t *d_src, uint32_t *d_vlen, uint8_t *d_status, uint64_t *d_report, void *stream) {
    if ((nq && !d_off) || ((uintptr_t)d_off & 7)) return BSDB_EINVAL;
    return dev_db_locate(db, d_blob, d_off, blob_bytes, 0, nq, d_src, d_vlen, d_status, d_report, stream);
}

int bsdb_dev_db_gather(bsdb_db *db, const uint64_t *d_src, const uint64_t *d_voff, uint64_t nq, uint8_t *d_values,
                       uint64_t value_bytes, void *stream) {
    if (!db || (nq && (!d_src || !d_voff)) || (value_bytes && !d_values) || ((uintptr_t)d_src & 7) ||
        ((uintptr_t)d_voff & 7))
        return BSDB_EINVAL;
    bsdb_ctx *c = db_ctx(db);
    if (!c) return BSDB_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    HIP_OK(hipSetDevice(c->device));
    get_gather_launch(c, db, d_src, d_voff, nq, d_values, value_bytes, pick(c, stream));
    return launch_status();
}

}  // extern "C"
