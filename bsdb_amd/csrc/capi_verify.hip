// capi_verify.hip -- the whole-database check behind the C ABI (kernels:
// verify_kernels.hip).  Included by bsdb_capi.hip after capi_kv.hip.
//   bsdb_dev_verify_*        records resident on the device, one fused pass
//   bsdb_mph_verify_index_*  records in host memory, index files from disk
//   bsdb_kv_verify_index     records from the kv.db partition scan
// The index files are checked as a reader sees them: each window of slots is
// read from the file (pooled pinned pieces) into HBM, then every record is
// run against it.  Nothing here trusts the MPHF: E is checked first
// (k_verify_structure), and the record kernels do nothing when it is invalid.

namespace {

struct VerifyWindow {
    uint64_t start = 0, len = 0;
    const uint64_t *d_index = nullptr, *d_index_a = nullptr;
};

void verify_launch(bsdb_ctx *c, const MphView &v, const VerifyArgs &a, hipStream_t s) {
    if (!a.n) return;
    const uint32_t grid = grid_for(c->num_cus, a.n);
    if (a.off)
        k_verify_var<<<grid, 256, 0, s>>>(v, a);
    else if (a.key_len == 13)
        k_verify_fixed<true><<<grid, 256, 0, s>>>(v, a);
    else
        k_verify_fixed<false><<<grid, 256, 0, s>>>(v, a);
}

int dev_verify(bsdb_ctx *c, const uint8_t *d_keys, const uint64_t *d_off, uint64_t blob_bytes, uint32_t key_len,
               uint64_t count, const uint64_t *d_addr, uint64_t addr_base, uint64_t addr_stride, uint64_t first,
               const uint64_t *d_value8, const uint8_t *d_vlen, uint64_t n, uint64_t m, const uint64_t *d_E,
               const uint64_t *d_values, uint32_t width, const uint64_t *d_sigbits, uint64_t start, uint64_t len,
               const uint64_t *d_index, const uint8_t *d_index_a, uint64_t *d_out, void *stream) {
    if (!c || !d_out || m == 0 || m > 0x7FFFFFFFULL || width > 64 || !d_E || !d_values || (width && !d_sigbits) ||
        (count && !d_keys) || (len && !d_index) || (d_index_a && (!d_value8 || !d_vlen)) || ((uintptr_t)d_index_a & 7) ||
        ((uintptr_t)d_out & 7))
        return BSDB_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    HIP_OK(hipSetDevice(c->device));
    hipStream_t s = pick(c, stream);
    unsigned long long *out = (unsigned long long *)d_out;
    k_verify_structure<<<grid_for(c->num_cus, m + 1), 256, 0, s>>>(d_E, m, n, out);
    const MphView v{d_E, d_values, d_sigbits, n, (uint32_t)(2 * m), width};
    VerifyArgs a{};
    a.keys = d_keys;
    a.off = d_off;
    a.blob_bytes = blob_bytes;
    a.n = count;
    a.key_len = key_len;
    a.addr = d_addr;
    a.addr_base = addr_base;
    a.addr_stride = addr_stride;
    a.first = first;
    a.value8 = d_index_a ? d_value8 : nullptr;
    a.vlen = d_index_a ? d_vlen : nullptr;
    a.start = start;
    a.len = len;
    a.index = d_index;
    a.index_a = (const uint64_t *)d_index_a;
    a.out = out;
    verify_launch(c, v, a, s);
    return launch_status();
}

// `bytes` of the file at `file_off` into device memory, through two pooled
// pinned pieces (the read of piece i + 1 beside the DMA of piece i).
int load_slots(int fd, uint64_t file_off, void *d_dst, uint64_t bytes, hipStream_t s) {
    if (!bytes) return BSDB_OK;
    void *pin[2] = {pinned_pool().take(), pinned_pool().take()};
    hipEvent_t ev[2] = {nullptr, nullptr};
    int rc = (pin[0] && pin[1]) ? BSDB_OK : BSDB_ENOMEM;
    for (int i = 0; i < 2 && !rc; ++i)
        if (hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) != hipSuccess) rc = BSDB_EIO;
    bool pending[2] = {false, false};
    for (uint64_t o = 0, k = 0; o < bytes && !rc; o += XFER_PIECE, ++k) {
        const int i = (int)(k & 1);
        const uint64_t len = std::min<uint64_t>(XFER_PIECE, bytes - o);
        if (pending[i] && hipEventSynchronize(ev[i]) != hipSuccess) rc = BSDB_EIO;
        for (uint64_t got = 0; got < len && !rc;) {
            const ssize_t r = pread(fd, (uint8_t *)pin[i] + got, len - got, (off_t)(file_off + o + got));
            if (r < 0 && errno == EINTR) continue;
            if (r <= 0) rc = BSDB_EFILE;  // (shorter than its size said)
            else got += (uint64_t)r;
        }
        if (rc) break;
        if (hipMemcpyAsync((uint8_t *)d_dst + o, pin[i], len, hipMemcpyHostToDevice, s) != hipSuccess ||
            hipEventRecord(ev[i], s) != hipSuccess)
            rc = BSDB_EIO;
        pending[i] = true;
    }
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = BSDB_EIO;
    for (int i = 0; i < 2; ++i) {
        pinned_pool().give(pin[i]);
        if (ev[i]) (void)hipEventDestroy(ev[i]);
    }
    return rc;
}

// One verification: the files, the structure check, then for every window
// begin -> put* -> end.  Each step takes the context's lock itself (the kv.db
// scan threads put concurrently).
struct VerifyRun {
    bsdb_mph *p = nullptr;
    bsdb_ctx *c = nullptr;
    bool approx = false;
    int fd = -1, fda = -1;
    uint64_t windows = 0, cap = 0;  // windows of at most cap slots
    uint64_t *d_index = nullptr, *d_index_a = nullptr;
    unsigned long long *d_out = nullptr;
    VerifyWindow win;
    uint64_t rep[BSDB_VERIFY_WORDS] = {0, 0, 0, 0, 0, UINT64_MAX, 0, 0};

    MphView view() const { return MphView{p->E, p->values, p->sigbits, p->n, (uint32_t)(2 * p->m), p->width}; }

    ~VerifyRun() {
        if (fd >= 0) close(fd);
        if (fda >= 0) close(fda);
        if (d_index || d_index_a || d_out) {
            std::lock_guard<std::mutex> g(c->mu);
            (void)hipSetDevice(c->device);
            (void)hipStreamSynchronize(c->stream);
            (void)hipFree(d_index);
            (void)hipFree(d_index_a);
            (void)hipFree(d_out);
        }
    }

    // BSDB_OK: run the windows; BSDB_EVERIFY: flags set, no record pass
    int open(bsdb_mph *mph, bool approximate, const char *index_path, const char *index_a_path, uint32_t want) {
        p = mph;
        c = mph->c;
        approx = approximate;
        const uint64_t n = p->n;
        struct stat st;
        if ((fd = ::open(index_path, O_RDONLY)) < 0 || fstat(fd, &st) != 0) return BSDB_EFILE;
        if ((uint64_t)st.st_size != 8 * n) rep[VW_FLAGS] |= 2;
        if (approx) {
            if ((fda = ::open(index_a_path, O_RDONLY)) < 0 || fstat(fda, &st) != 0) return BSDB_EFILE;
            if ((uint64_t)st.st_size != 8 * n) rep[VW_FLAGS] |= 2;
        }
        std::lock_guard<std::mutex> g(c->mu);
        HIP_OK(hipSetDevice(c->device));
        Ordered ord(c, c->stream);
        if (dmalloc(&d_out, BSDB_VERIFY_WORDS * 8) != hipSuccess) return BSDB_ENOMEM;
        HIP_OK(hipMemsetAsync(d_out, 0, BSDB_VERIFY_WORDS * 8, c->stream));
        k_verify_structure<<<grid_for(c->num_cus, p->m + 1), 256, 0, c->stream>>>(p->E, p->m, n, d_out);
        int rc = launch_status();
        if (rc) return rc;
        uint64_t flags = 0;
        HIP_OK(hipMemcpyAsync(&flags, d_out + VW_FLAGS, 8, hipMemcpyDeviceToHost, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
        rep[VW_FLAGS] |= flags & 1;
        if (rep[VW_FLAGS]) return BSDB_EVERIFY;
        // the fewest windows whose slots fit half of the free HBM, or the caller's count
        const uint64_t slot_bytes = approx ? 16 : 8;
        if (!want) {
            size_t free_b = 0, total_b = 0;
            HIP_OK(hipMemGetInfo(&free_b, &total_b));
            const uint64_t room = std::max<uint64_t>(slot_bytes, free_b / 2);
            windows = std::max<uint64_t>(1, (n * slot_bytes + room - 1) / room);
        } else {
            windows = std::max<uint64_t>(1, std::min<uint64_t>(want, n));
        }
        cap = (n + windows - 1) / windows + 1;  // window w = ranks [w n / W, (w + 1) n / W)
        if (dmalloc(&d_index, cap * 8) != hipSuccess || (approx && dmalloc(&d_index_a, cap * 8) != hipSuccess))
            return BSDB_ENOMEM;
        return BSDB_OK;
    }

    static uint64_t bound(uint64_t n, uint64_t w, uint64_t W) { return (uint64_t)((unsigned __int128)n * w / W); }

    int begin(uint64_t w) {
        std::lock_guard<std::mutex> g(c->mu);
        HIP_OK(hipSetDevice(c->device));
        Ordered ord(c, c->stream);
        win.start = bound(p->n, w, windows);
        win.len = bound(p->n, w + 1, windows) - win.start;
        win.d_index = d_index;
        win.d_index_a = approx ? d_index_a : nullptr;
        int rc = load_slots(fd, win.start * 8, d_index, win.len * 8, c->stream);
        if (!rc && approx) rc = load_slots(fda, win.start * 8, d_index_a, win.len * 8, c->stream);
        if (rc) return rc;
        const uint64_t init[BSDB_VERIFY_WORDS] = {0, 0, 0, 0, 0, UINT64_MAX, 0, 0};
        HIP_OK(hipMemcpyAsync(d_out, init, sizeof(init), hipMemcpyHostToDevice, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));  // (init is a stack buffer)
        return BSDB_OK;
    }

    // records in host memory (var-len when h_off, else key_len bytes each):
    // uploaded through the feed slots, verified batch by batch; returns after
    // the device finished (the caller may reuse its buffers)
    int put(const uint8_t *h_keys, uint32_t key_len, const uint64_t *h_off, uint64_t count, const uint64_t *h_addr,
            const uint64_t *h_value8, const uint8_t *h_vlen) {
        std::lock_guard<std::mutex> g(c->mu);
        HIP_OK(hipSetDevice(c->device));
        Ordered ord(c, c->stream);
        const MphView v = view();
        const uint64_t batch = h_off ? 0 : fixed_batch(key_len, 128ULL << 20);
        int rc = feed_batches(
            c, count, [&](uint64_t k0) { return h_off ? var_batch_end(h_off, k0, count) : std::min(count, k0 + batch); },
            [&](FeedSlot &f, uint64_t k0, uint64_t k1) {
                return h_off ? upload_var(c, f, h_keys, h_off, k0, k1) : upload_fixed(c, f, h_keys, key_len, k0, k1);
            },
            [&](FeedSlot &f, uint64_t k0, uint64_t k1) {
                const uint64_t nk = k1 - k0;
                int r2 = f.buf[2].grow(nk * 8);
                if (r2) return r2;
                HIP_OK(hipMemcpyAsync(f.buf[2].p, h_addr + k0, nk * 8, hipMemcpyHostToDevice, c->stream));
                if (approx) {
                    if ((r2 = f.buf[3].grow(nk * 8)) || (r2 = f.buf[4].grow(nk))) return r2;
                    HIP_OK(hipMemcpyAsync(f.buf[3].p, h_value8 + k0, nk * 8, hipMemcpyHostToDevice, c->stream));
                    HIP_OK(hipMemcpyAsync(f.buf[4].p, h_vlen + k0, nk, hipMemcpyHostToDevice, c->stream));
                }
                VerifyArgs a{};
                a.keys = f.buf[0].as<const uint8_t>();
                a.off = h_off ? f.buf[1].as<const uint64_t>() : nullptr;
                a.blob_bytes = h_off ? h_off[k1] - h_off[k0] : nk * key_len;
                a.n = nk;
                a.key_len = key_len;
                a.addr = f.buf[2].as<const uint64_t>();
                a.value8 = approx ? f.buf[3].as<const uint64_t>() : nullptr;
                a.vlen = approx ? f.buf[4].as<const uint8_t>() : nullptr;
                a.start = win.start;
                a.len = win.len;
                a.index = win.d_index;
                a.index_a = win.d_index_a;
                a.out = d_out;
                verify_launch(c, v, a, c->stream);
                return launch_status();
            });
        if (rc) {
            (void)hipStreamSynchronize(c->stream);
            return rc;
        }
        HIP_OK(hipStreamSynchronize(c->stream));
        return BSDB_OK;
    }

    // the window's counters into the report: records and rejected from the
    // first pass (every pass sees all records), the window tests summed
    int end(uint64_t w) {
        uint64_t got[BSDB_VERIFY_WORDS];
        {
            std::lock_guard<std::mutex> g(c->mu);
            HIP_OK(hipSetDevice(c->device));
            Ordered ord(c, c->stream);
            HIP_OK(hipMemcpyAsync(got, d_out, sizeof(got), hipMemcpyDeviceToHost, c->stream));
            HIP_OK(hipStreamSynchronize(c->stream));
        }
        if (w == 0) {
            rep[VW_RECORDS] = got[VW_RECORDS];
            rep[VW_REJECTED] = got[VW_REJECTED];
        }
        rep[VW_IN_WINDOW] += got[VW_IN_WINDOW];
        rep[VW_WRONG_ADDR] += got[VW_WRONG_ADDR];
        rep[VW_WRONG_VALUE] += got[VW_WRONG_VALUE];
        rep[VW_MIN_BAD] = std::min(rep[VW_MIN_BAD], got[VW_MIN_BAD]);
        rep[VW_WINDOWS] = w + 1;
        return BSDB_OK;
    }

    // fills `out`; BSDB_EVERIFY when anything is wrong
    int finish(uint64_t *out) {
        if (!(rep[VW_FLAGS] & 3) && rep[VW_RECORDS] != p->n) rep[VW_FLAGS] |= 4;
        memcpy(out, rep, sizeof(rep));
        const bool bad = rep[VW_REJECTED] || rep[VW_WRONG_ADDR] || rep[VW_WRONG_VALUE] || rep[VW_FLAGS] ||
                         rep[VW_IN_WINDOW] != rep[VW_RECORDS] - rep[VW_REJECTED];
        return bad ? BSDB_EVERIFY : BSDB_OK;
    }
};

int mph_verify_index(bsdb_mph *p, const uint8_t *h_keys, uint32_t key_len, const uint64_t *h_off, uint64_t count,
                     const uint64_t *h_addr, const uint64_t *h_value8, const uint8_t *h_vlen, int approximate,
                     const char *index_path, const char *index_a_path, uint32_t windows, uint64_t *out) {
    VerifyRun run;
    int rc = run.open(p, approximate != 0, index_path, index_a_path, windows);
    if (rc == BSDB_EVERIFY) return run.finish(out);
    if (rc) return rc;
    for (uint64_t w = 0; w < run.windows; ++w)
        if ((rc = run.begin(w)) || (rc = run.put(h_keys, key_len, h_off, count, h_addr, h_value8, h_vlen)) ||
            (rc = run.end(w)))
            return rc;
    return run.finish(out);
}

// Every partition file scanned by host threads (one partition per thread at a
// time), each parsed chunk handed to `put` and dropped: host memory holds the
// chunks in flight, never the whole record set.
int kv_scan_chunks(const char *kv_base, int partitions, int format, uint32_t block_size, int threads, bool values,
                   const std::function<int(KvPart &)> &put) {
    uint64_t kv_chunk = 1ull << 21;
    if (const char *e = getenv("BSDB_KV_CHUNK")) kv_chunk = strtoull(e, nullptr, 10) ? strtoull(e, nullptr, 10) : UINT64_MAX;
    const int T = std::max(1, std::min(threads > 0 ? threads : usable_cpus(), partitions));
    std::atomic<int> next{0}, err{BSDB_OK};
    auto worker = [&] {
        for (int pi; !err.load() && (pi = next.fetch_add(1)) < partitions;) {
            int r;
            try {
                KvPart part;
                part.values = values;
                part.chunk = kv_chunk;
                part.flush = [&]() -> int {
                    if (!part.addr.size()) return BSDB_OK;
                    const int f = put(part);
                    part.reset_records();
                    return f;
                };
                r = scan_file(std::string(kv_base) + "." + std::to_string(pi), format, (uint64_t)pi, block_size, part);
                if (!r) r = part.flush();
            } catch (const std::bad_alloc &) {
                r = BSDB_ENOMEM;
            }
            if (r) {
                int expect = BSDB_OK;
                err.compare_exchange_strong(expect, r);
            }
        }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < T; ++t) th.emplace_back(worker);
    worker();
    for (auto &t : th) t.join();
    return err.load();
}

}  // namespace

extern "C" {

int bsdb_dev_verify_fixed(bsdb_ctx *c, const uint8_t *d_keys, uint32_t key_len, uint64_t count, const uint64_t *d_addr,
                          uint64_t addr_base, uint64_t addr_stride, uint64_t first, const uint64_t *d_value8,
                          const uint8_t *d_vlen, uint64_t n, uint64_t num_buckets, const uint64_t *d_E,
                          const uint64_t *d_values, uint32_t width, const uint64_t *d_sigbits, uint64_t start,
                          uint64_t len, const uint64_t *d_index, const uint8_t *d_index_a, uint64_t *d_out,
                          void *stream) {
    if (bad_key_len(key_len) || ((uintptr_t)d_keys & 3)) return BSDB_EINVAL;  // (the key readers load dwords)
    return dev_verify(c, d_keys, nullptr, count * key_len, key_len, count, d_addr, addr_base, addr_stride, first, d_value8,
                      d_vlen, n, num_buckets, d_E, d_values, width, d_sigbits, start, len, d_index, d_index_a, d_out,
                      stream);
}

int bsdb_dev_verify_var(bsdb_ctx *c, const uint8_t *d_blob, uint64_t blob_bytes, const uint64_t *d_offsets,
                        uint64_t count, const uint64_t *d_addr, uint64_t addr_base, uint64_t addr_stride, uint64_t first,
                        const uint64_t *d_value8, const uint8_t *d_vlen, uint64_t n, uint64_t num_buckets,
                        const uint64_t *d_E, const uint64_t *d_values, uint32_t width, const uint64_t *d_sigbits,
                        uint64_t start, uint64_t len, const uint64_t *d_index, const uint8_t *d_index_a, uint64_t *d_out,
                        void *stream) {
    if (count && !d_offsets) return BSDB_EINVAL;
    if (!count) d_offsets = nullptr;  // (nothing is launched)
    return dev_verify(c, d_blob, d_offsets, blob_bytes, 0, count, d_addr, addr_base, addr_stride, first, d_value8, d_vlen,
                      n, num_buckets, d_E, d_values, width, d_sigbits, start, len, d_index, d_index_a, d_out, stream);
}

int bsdb_mph_verify_index_fixed(bsdb_mph *p, const uint8_t *h_keys, uint32_t key_len, uint64_t count,
                                const uint64_t *h_addr, const uint64_t *h_value8, const uint8_t *h_vlen,
                                int approximate, const char *index_path, const char *index_a_path, uint32_t windows,
                                uint64_t *out) {
    if (!p || !p->c || !out || !index_path || bad_key_len(key_len) || (approximate && !index_a_path) ||
        (count && (!h_keys || !h_addr || (approximate && (!h_value8 || !h_vlen)))))
        return BSDB_EINVAL;
    return mph_verify_index(p, h_keys, key_len, nullptr, count, h_addr, h_value8, h_vlen, approximate, index_path,
                            index_a_path, windows, out);
}

int bsdb_mph_verify_index_var(bsdb_mph *p, const uint8_t *h_blob, const uint64_t *h_off, uint64_t count,
                              const uint64_t *h_addr, const uint64_t *h_value8, const uint8_t *h_vlen, int approximate,
                              const char *index_path, const char *index_a_path, uint32_t windows, uint64_t *out) {
    if (!p || !p->c || !out || !index_path || (approximate && !index_a_path) ||
        (count && (!h_blob || !h_off || !h_addr || (approximate && (!h_value8 || !h_vlen)))))
        return BSDB_EINVAL;
    static const uint64_t zero_off[1] = {0};
    return mph_verify_index(p, h_blob, 0, count ? h_off : zero_off, count, h_addr, h_value8, h_vlen, approximate,
                            index_path, index_a_path, windows, out);
}

// The check of a finished database from its own files: hash.db's fields (the
// MPHF handle), index.db / index_a.db as written, and the records of every
// kv.db.<p> through the scan of bsdb_kv_build_index.  More than one window
// means one rescan per window.
int bsdb_kv_verify_index(bsdb_mph *p, const char *kv_base, int partitions, int format, uint32_t block_size, int threads,
                         int approximate, const char *index_path, const char *index_a_path, uint32_t windows,
                         uint64_t *out) {
    if (!p || !p->c || !out || !index_path || !kv_base || partitions < 1 || (format != 0 && format != 1) ||
        (format == 1 && (block_size == 0 || block_size % KV_PAGE)) || (approximate && !index_a_path))
        return BSDB_EINVAL;
    for (int pi = 0; pi < partitions; ++pi) {
        struct stat st;
        if (stat((std::string(kv_base) + "." + std::to_string(pi)).c_str(), &st) != 0) return BSDB_EFILE;
    }
    VerifyRun run;
    int rc = run.open(p, approximate != 0, index_path, index_a_path, windows);
    if (rc == BSDB_EVERIFY) return run.finish(out);
    if (rc) return rc;
    for (uint64_t w = 0; w < run.windows; ++w) {
        if ((rc = run.begin(w))) return rc;
        rc = kv_scan_chunks(kv_base, partitions, format, block_size, threads, approximate != 0, [&](KvPart &part) {
            return run.put(part.blob.data(), 0, part.off.data(), part.addr.size(), part.addr.data(), part.value8.data(),
                           part.vlen.data());
        });
        if (rc || (rc = run.end(w))) return rc;
    }
    return run.finish(out);
}

}  // extern "C"
