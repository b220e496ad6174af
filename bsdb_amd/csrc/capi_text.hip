// capi_text.hip -- the text front end behind the C ABI (kernels:
// text_kernels.hip, plan: text_plan.hpp).  Included by bsdb_capi.hip after
// capi_get.hip.
//   bsdb_dev_text_split / bsdb_dev_text_pack   the kernels on device buffers
//   bsdb_builder_add_dev_var                   a batch in device memory into the streaming builder
//   bsdb_dev_text_pack_blocked                 the pack into the blocked layout (text_blocked_kernels.hip)
//   bsdb_text_set_chunk / bsdb_text_build(_layout)   files of text lines -> kv.db files + index files
// What Builder's put loop and build() do (tools/Builder.java:144-176) one line
// per call on one thread per input file.

namespace {

// u32 counts[m] -> u64 off[m + 1] on s (m = 0: off[0] = 0)
int text_scan(bsdb_ctx *c, const uint32_t *counts, uint64_t m, uint64_t *off, hipStream_t s) {
    if (m) return edge_offsets_impl(c, counts, m, off, s);
    HIP_OK(hipMemsetAsync(off, 0, 8, s));
    return BSDB_OK;
}

// The split of one chunk; the caller holds the context's lock and has set the
// device.  Waits once for the counts of lines and separators.
int text_split_impl(bsdb_ctx *c, const uint8_t *d_text, uint64_t bytes, uint32_t sep, uint64_t cap, uint32_t *d_kpos,
                    uint32_t *d_klen, uint32_t *d_vpos, uint32_t *d_vlen, unsigned long long *d_report, hipStream_t s) {
    if (!bytes) return BSDB_OK;
    const uint64_t nb = text_blocks(bytes);
    int rc;
    if ((rc = c->t_cnt.grow(2 * 4 * nb)) || (rc = c->t_off.grow(2 * 8 * (nb + 1)))) return rc;
    uint32_t *cnt_st = c->t_cnt.as<uint32_t>(), *cnt_sp = cnt_st + nb;
    uint64_t *off_st = c->t_off.as<uint64_t>(), *off_sp = off_st + nb + 1;
    const uint32_t grid = text_count_grid(bytes);
    k_text_count<<<grid, 256, 0, s>>>(d_text, bytes, sep, cnt_st, cnt_sp);
    if ((rc = text_scan(c, cnt_st, nb, off_st, s)) || (rc = text_scan(c, cnt_sp, nb, off_sp, s))) return rc;
    uint64_t lines = 0, seps = 0;
    HIP_OK(hipMemcpyAsync(&lines, off_st + nb, 8, hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(&seps, off_sp + nb, 8, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    if (lines == 0 || lines > bytes || seps > bytes) return BSDB_EIO;  // (byte 0 starts a line)
    if ((rc = c->t_ls.grow(4 * lines)) || (rc = c->t_sp.grow(4 * (seps + 1))) || (rc = c->t_keep.grow(4 * lines)) ||
        (rc = c->t_scan.grow(8 * (lines + 1))))
        return rc;
    k_text_positions<<<grid, 256, 0, s>>>(d_text, bytes, sep, off_st, off_sp, c->t_ls.as<uint32_t>(), lines,
                                          c->t_sp.as<uint32_t>(), seps);
    TextSplit a{};
    a.text = d_text;
    a.bytes = bytes;
    a.ls = c->t_ls.as<const uint32_t>();
    a.lines = lines;
    a.sp = c->t_sp.as<const uint32_t>();
    a.seps = seps;
    a.keep = c->t_keep.as<uint32_t>();
    a.keep_off = c->t_scan.as<const uint64_t>();
    a.kpos = d_kpos;
    a.klen = d_klen;
    a.vpos = d_vpos;
    a.vlen = d_vlen;
    a.cap = cap;
    a.out = d_report;
    const uint32_t lgrid = text_lane_grid(lines, c->num_cus);
    k_text_records<false><<<lgrid, 256, 0, s>>>(a);
    if ((rc = text_scan(c, a.keep, lines, c->t_scan.as<uint64_t>(), s))) return rc;
    k_text_records<true><<<lgrid, 256, 0, s>>>(a);
    return launch_status();
}

struct TextDesc {
    const uint32_t *kpos, *klen, *vpos, *vlen;
};

// What a pack reads and writes: bsdb_dev_text_pack(_blocked)'s arguments.
struct TextPackIO {
    const uint8_t *d_text;
    uint64_t bytes;
    TextDesc d;
    uint64_t count;
    int partitions;
    uint32_t B;  // the blocked layout's block bytes; 0: the compact layout
    const uint64_t *h_part_size;
    uint8_t *d_image;
    uint64_t image_cap, *h_run_bytes, *d_addr;
    uint8_t *d_blob;
    uint64_t blob_cap, *d_off, *h_blob_bytes, *d_value8;
    uint8_t *d_value_len;
    bool from_image = false;  // the records lie in a resident image (capi_merge.hip): d.kpos / d.vpos and d_text are unused
};

bool text_pack_bad_args(const bsdb_ctx *c, const TextPackIO &io) {
    const TextDesc &d = io.d;
    return !c || io.bytes > TEXT_MAX_BYTES || (io.bytes && !io.d_text) || !aligned16(io.d_text) ||
           io.count > text_max_records(io.bytes) || io.partitions < 1 || io.partitions > TEXT_MAX_PARTS || !io.h_part_size ||
           !io.h_run_bytes || (io.count && (!d.kpos || !d.klen || !d.vpos || !d.vlen)) ||
           (((uintptr_t)d.kpos | (uintptr_t)d.klen | (uintptr_t)d.vpos | (uintptr_t)d.vlen) & 3) || (!io.d_blob != !io.d_off) ||
           (!io.d_value8 != !io.d_value_len) || (((uintptr_t)io.d_addr | (uintptr_t)io.d_off | (uintptr_t)io.d_value8) & 7);
}

// A pack under way: what a pack hands to the layout's placement and what the
// placement finds out.  The placement works on sizes alone: whose records they
// are (a chunk of text, a resident image: capi_merge.hip) is the pack's.
struct TextPlacing {
    TextRuns runs{};
    uint32_t *rsize, *ksize;         // [count] the records' bytes in the image and in the key blob
    uint32_t lgrid;                  // a record per lane
    unsigned long long *sizes_report = nullptr;  // k_rec_sizes' (the merge's report), else null: k_text_sizes
    const uint64_t *roff = nullptr;  // compact: the scan of rsize, the addresses' offsets
    const uint64_t *PS = nullptr, *PL = nullptr;  // blocked: k_blk_place's position lists
    uint64_t image_bytes = 0;
    uint64_t blob_bytes = 0;
    uint64_t run[TEXT_MAX_PARTS] = {};
};

// The records' sizes (ssize: the blocked layout's, else null), the layout's
// scan sized -> scan and the key blob's offsets.
int text_sizes(bsdb_ctx *c, const TextPackIO &io, const TextPlacing &pl, uint32_t *ssize, const uint32_t *sized, uint64_t *scan,
               hipStream_t s) {
    if (io.from_image) k_rec_sizes<<<pl.lgrid, 256, 0, s>>>(io.d.klen, io.d.vlen, io.count, io.B, pl.rsize, pl.ksize, ssize, pl.sizes_report);
    else k_text_sizes<<<pl.lgrid, 256, 0, s>>>(io.d.klen, io.d.vlen, io.count, io.B, pl.rsize, pl.ksize, ssize);
    int rc;
    if ((rc = text_scan(c, sized, io.count, scan, s))) return rc;
    return io.d_off ? text_scan(c, pl.ksize, io.count, io.d_off, s) : BSDB_OK;
}

// The placement's one wait: its own read-backs, queued by the caller, and the key blob's size.
int text_sizes_wait(const TextPackIO &io, TextPlacing &pl, hipStream_t s) {
    if (io.d_off) HIP_OK(hipMemcpyAsync(&pl.blob_bytes, io.d_off + io.count, 8, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    return BSDB_OK;
}

bool text_pack_too_large(const TextPackIO &io, const TextPlacing &pl, uint64_t image_bytes) {
    return (io.d_image && image_bytes > io.image_cap) || (io.d_blob && pl.blob_bytes > io.blob_cap);
}

// k_text_pack of the records `a` names into (dst, out_bytes) by the scan `off`
template <bool IMAGE>
void text_pack_launch(bsdb_ctx *c, TextPack a, const uint64_t *off, uint8_t *dst, uint64_t out_bytes, hipStream_t s) {
    a.off = off, a.dst = dst, a.out_bytes = out_bytes;
    k_text_pack<IMAGE><<<piece_grid(out_bytes, (uint32_t)((uintptr_t)dst & 15), c->num_cus), 256, 0, s>>>(a);
}

// The compact layout: a record lies where the scan of the sizes puts it, run p
// appended to a file of h_part_size[p] bytes.
int text_place_compact(bsdb_ctx *c, const TextPackIO &io, TextPlacing &pl, hipStream_t s) {
    int rc;
    if ((rc = c->t_roff.grow(8 * (io.count + 1)))) return rc;
    uint64_t *roff = c->t_roff.as<uint64_t>();
    pl.roff = roff;
    if ((rc = text_sizes(c, io, pl, nullptr, pl.rsize, roff, s))) return rc;
    uint64_t at[TEXT_MAX_PARTS + 1] = {};
    for (int p = 0; p <= io.partitions; ++p)
        HIP_OK(hipMemcpyAsync(&at[p], roff + pl.runs.bound[p], 8, hipMemcpyDeviceToHost, s));
    if ((rc = text_sizes_wait(io, pl, s))) return rc;
    const uint64_t image_bytes = at[io.partitions];
    if (text_pack_too_large(io, pl, image_bytes)) return BSDB_EINVAL;
    for (int p = 0; p < io.partitions; ++p) {
        pl.run[p] = at[p + 1] - at[p];
        if (io.h_part_size[p] > TEXT_MAX_FILE || pl.run[p] > TEXT_MAX_FILE - io.h_part_size[p]) return BSDB_EINVAL;
        pl.runs.file_base[p] = io.h_part_size[p] - at[p];  // (+ roff[r] >= at[p]: the sum never wraps past the file offset)
    }
    pl.image_bytes = image_bytes;
    return BSDB_OK;
}

// The blocked layout (text_blocked_kernels.hip): blocks of B bytes, run p
// appended to a file of h_part_size[p] bytes (a multiple of 4096).  The runs'
// bytes are the events' sums plus the block each run with a small record
// leaves open at its end.
int text_place_blocked(bsdb_ctx *c, const TextPackIO &io, TextPlacing &pl, hipStream_t s) {
    const uint64_t count = io.count;
    const uint32_t B = io.B, tiles = (uint32_t)((count + TEXT_TILE - 1) / TEXT_TILE);
    const TextRuns &runs = pl.runs;
    int rc;
    if ((rc = c->t_blk.grow(text_place_workspace(count)))) return rc;
    // the workspace, 8-byte arrays first
    uint64_t *S = c->t_blk.as<uint64_t>(), *E = S + count + 1, *PS = E + count + 1, *PL = PS + count + 1;
    uint2 *exl = reinterpret_cast<uint2 *>(PL + count + 1);
    uint32_t *ssize = reinterpret_cast<uint32_t *>(exl + count), *next = ssize + count, *ev = next + count, *boff = ev + count,
             *bend = boff + count, *entry = bend + count, *carry = entry + tiles;
    if ((rc = text_sizes(c, io, pl, ssize, ssize, S, s))) return rc;
    HIP_OK(hipMemsetAsync(entry, 0, 2 * 4 * (size_t)tiles, s));
    k_blk_tile<<<tiles, 256, 0, s>>>(runs, S, count, B, next, exl);
    k_blk_chase<<<(uint32_t)io.partitions, 64, 0, s>>>(runs, exl, count, tiles, entry, carry);
    k_blk_flags<<<tiles, 256, 0, s>>>(runs, S, pl.rsize, next, entry, carry, count, B, ev, boff, bend);
    if ((rc = text_scan(c, ev, count, E, s))) return rc;
    uint64_t e_at[TEXT_MAX_PARTS + 1] = {}, s_at[TEXT_MAX_PARTS + 1] = {};
    for (int p = 0; p <= io.partitions; ++p) {
        HIP_OK(hipMemcpyAsync(&e_at[p], E + runs.bound[p], 8, hipMemcpyDeviceToHost, s));
        HIP_OK(hipMemcpyAsync(&s_at[p], S + runs.bound[p], 8, hipMemcpyDeviceToHost, s));
    }
    if ((rc = text_sizes_wait(io, pl, s))) return rc;
    TextBlockedRuns br{};
    uint64_t image_bytes = 0;
    for (int p = 0; p < io.partitions; ++p) {
        pl.run[p] = e_at[p + 1] - e_at[p] + (s_at[p + 1] > s_at[p] ? B : 0);
        if (io.h_part_size[p] > TEXT_MAX_FILE_BLOCKED || pl.run[p] > TEXT_MAX_FILE_BLOCKED - io.h_part_size[p]) return BSDB_EINVAL;
        br.image_base[p] = image_bytes;
        br.file_size[p] = io.h_part_size[p];
        image_bytes += pl.run[p];
    }
    if (text_pack_too_large(io, pl, image_bytes)) return BSDB_EINVAL;
    if (io.d_image || io.d_addr)
        k_blk_place<<<text_lane_grid(count + 1, c->num_cus), 256, 0, s>>>(runs, br, E, pl.rsize, boff, bend, count, B, image_bytes, PS,
                                                                           PL, io.d_addr);
    pl.PS = PS, pl.PL = PL;
    pl.image_bytes = image_bytes;
    return BSDB_OK;
}

// The placement of one chunk's `count` >= 1 records, for either pack: the runs
// of the partition rule, the sizes and the layout's placement, which waits
// once, for the sizes (they go back to the host, and nothing is written before
// they are known to fit).
int text_place(bsdb_ctx *c, const TextPackIO &io, TextPlacing &pl, hipStream_t s) {
    int rc;
    if ((rc = c->t_size.grow(2 * 4 * io.count))) return rc;
    pl.rsize = c->t_size.as<uint32_t>();
    pl.ksize = pl.rsize + io.count;
    pl.lgrid = text_lane_grid(io.count, c->num_cus);
    pl.runs.partitions = (uint32_t)io.partitions;
    for (int p = 0; p <= io.partitions; ++p) pl.runs.bound[p] = text_run_bound(io.count, (uint32_t)io.partitions, (uint32_t)p);
    return io.B ? text_place_blocked(c, io, pl, s) : text_place_compact(c, io, pl, s);
}

// what every pack reports when it has launched everything
int text_pack_done(const TextPackIO &io, const TextPlacing &pl) {
    const int rc = launch_status();
    if (rc) return rc;
    for (int p = 0; p < io.partitions; ++p) io.h_run_bytes[p] = pl.run[p];
    if (io.h_blob_bytes) *io.h_blob_bytes = pl.blob_bytes;
    return BSDB_OK;
}

// a pack of no record
int text_pack_empty(const TextPackIO &io, hipStream_t s) {
    for (int p = 0; p < io.partitions; ++p) io.h_run_bytes[p] = 0;
    if (io.h_blob_bytes) *io.h_blob_bytes = 0;
    if (!io.count && io.d_off) HIP_OK(hipMemsetAsync(io.d_off, 0, 8, s));
    return BSDB_OK;
}

// The pack of one chunk's `count` records; the caller holds the context's lock
// and has set the device.  After the placement the image's kernel is
// launched; the key blob and the value heads follow it.
int text_pack_impl(bsdb_ctx *c, const TextPackIO &io, hipStream_t s) {
    int rc;
    if ((rc = text_pack_empty(io, s)) || !io.count) return rc;
    TextPlacing pl;
    if ((rc = text_place(c, io, pl, s))) return rc;
    const TextPack pack{io.d_text, io.bytes, io.d.kpos, io.d.klen, io.d.vpos, io.d.vlen, io.count, nullptr, nullptr, 0};
    if (io.d_image && !io.B) text_pack_launch<true>(c, pack, pl.roff, io.d_image, pl.image_bytes, s);
    if (io.d_image && io.B && pl.image_bytes) {
        TextPackBlocked b{pack, pl.PS, pl.PL, io.B};
        b.t.dst = io.d_image;
        b.t.out_bytes = pl.image_bytes;
        k_text_pack_blocked<<<piece_grid(pl.image_bytes, (uint32_t)((uintptr_t)io.d_image & 15), c->num_cus), 256, 0, s>>>(b);
    }
    if (io.d_blob && pl.blob_bytes) text_pack_launch<false>(c, pack, io.d_off, io.d_blob, pl.blob_bytes, s);
    uint64_t *const d_addr = pl.roff ? io.d_addr : nullptr;  // (the blocked addresses are k_blk_place's)
    if (d_addr || io.d_value8)
        k_text_outputs<<<pl.lgrid, 256, 0, s>>>(pl.runs, io.d_text, io.bytes, io.d.vpos, io.d.vlen, pl.roff, io.count, d_addr,
                                                 io.d_value8, io.d_value_len);
    return text_pack_done(io, pl);
}

// bsdb_dev_text_pack(_blocked) after their argument checks
int text_pack_locked(bsdb_ctx *c, const TextPackIO &io, void *stream) {
    std::lock_guard<std::mutex> g(c->mu);
    HIP_OK(hipSetDevice(c->device));
    hipStream_t s = pick(c, stream);
    Ordered ord(c, s);
    return text_pack_impl(c, io, s);
}

// A batch in device memory into a streaming builder of variable-length keys:
// builder_add with the key copies device to device on the caller's stream,
// the offsets rebased by k_rebase_offsets, the record arrays copied to the
// builder's host arrays (and its device arrays when it keeps them).  Spill
// mode: the batch through host memory and the host add.
int builder_add_dev(bsdb_builder *b, const uint8_t *d_blob, const uint64_t *d_off, uint64_t count, const uint64_t *d_addr,
                    const uint64_t *d_value8, const uint8_t *d_vlen, hipStream_t s) {
    bsdb_ctx *c = b->c;
    if (!count) return BSDB_OK;
    HIP_OK(hipSetDevice(c->device));
    uint64_t o0 = 0, o1 = 0;  // the batch's first and last offset: its key bytes
    HIP_OK(hipMemcpyAsync(&o0, d_off, 8, hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(&o1, d_off + count, 8, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    if (o1 < o0) return BSDB_EINVAL;
    const uint64_t bytes = o1 - o0;
    std::shared_lock<std::shared_mutex> copying;
    uint64_t n0 = 0, kb0 = 0;
    bool spill = false;
    {
        std::lock_guard<std::mutex> gb(b->mu);
        if (b->failed) return b->failed;
        if (b->finished || b->borrowed_records) return BSDB_EINVAL;
        if ((!b->stride && !d_addr) || (b->approx && (!d_value8 || !d_vlen))) return BSDB_EINVAL;
        int rc = builder_make_room(b, count, bytes);
        if (rc) return b->failed = rc;
        spill = b->spill;
        if (!spill) {
            n0 = b->n;
            kb0 = b->key_bytes;
            b->uniform = false;  // (the lengths stay on the device: the variable-length kernels build it)
            copying = std::shared_lock<std::shared_mutex>(b->grow_mu);  // (before mu is released: no growth between)
            b->n += count;
            b->key_bytes += bytes;
            if (!b->stride) b->addr.n = b->n;
            if (b->approx) b->value8.n = b->vlen.n = b->n;
        }
    }
    if (spill) {
        // correct is enough here: everything to the host, then the host add
        std::vector<uint8_t> blob, vl;
        std::vector<uint64_t> off, addr, v8;
        try {
            blob.resize(std::max<uint64_t>(bytes, 1));
            off.resize(count + 1);
            if (!b->stride) addr.resize(count);
            if (b->approx) {
                v8.resize(count);
                vl.resize(count);
            }
        } catch (const std::bad_alloc &) {
            return BSDB_ENOMEM;
        }
        if (bytes) HIP_OK(hipMemcpyAsync(blob.data(), d_blob + o0, bytes, hipMemcpyDeviceToHost, s));
        HIP_OK(hipMemcpyAsync(off.data(), d_off, (count + 1) * 8, hipMemcpyDeviceToHost, s));
        if (!b->stride) HIP_OK(hipMemcpyAsync(addr.data(), d_addr, count * 8, hipMemcpyDeviceToHost, s));
        if (b->approx) {
            HIP_OK(hipMemcpyAsync(v8.data(), d_value8, count * 8, hipMemcpyDeviceToHost, s));
            HIP_OK(hipMemcpyAsync(vl.data(), d_vlen, count, hipMemcpyDeviceToHost, s));
        }
        HIP_OK(hipStreamSynchronize(s));
        for (uint64_t i = 0; i <= count; ++i) {
            if (off[i] < o0 || (i && off[i] < off[i - 1])) return BSDB_EINVAL;
            off[i] -= o0;
        }
        return bsdb_builder_add_var(b, blob.data(), off.data(), count, b->stride ? nullptr : addr.data(),
                                    b->approx ? v8.data() : nullptr, b->approx ? vl.data() : nullptr);
    }
    hipError_t e = hipSuccess;
    auto copy = [&](void *dst, const void *src, size_t len, hipMemcpyKind kind) {
        if (len && e == hipSuccess) e = hipMemcpyAsync(dst, src, len, kind, s);
    };
    copy(b->d_keys + kb0, d_blob + o0, bytes, hipMemcpyDeviceToDevice);
    uint64_t *dst_off = b->d_off + n0 + 1;
    copy(dst_off, d_off + 1, count * 8, hipMemcpyDeviceToDevice);
    if (e == hipSuccess) {
        k_rebase_offsets<<<grid_for(c->num_cus, count), 256, 0, s>>>(dst_off, count, kb0 - o0);
        e = hipGetLastError();
    }
    if (!b->stride) {
        copy(b->addr.p + n0, d_addr, count * 8, hipMemcpyDeviceToHost);
        if (b->dev_rec) copy((uint64_t *)b->d_raddr + n0, d_addr, count * 8, hipMemcpyDeviceToDevice);
    }
    if (b->approx) {
        copy(b->value8.p + n0, d_value8, count * 8, hipMemcpyDeviceToHost);
        copy(b->vlen.p + n0, d_vlen, count, hipMemcpyDeviceToHost);
        if (b->dev_rec) {
            copy((uint64_t *)b->d_rv8 + n0, d_value8, count * 8, hipMemcpyDeviceToDevice);
            copy((uint8_t *)b->d_rvl + n0, d_vlen, count, hipMemcpyDeviceToDevice);
        }
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);  // the caller may reuse its buffers
    const int rc = e == hipSuccess ? BSDB_OK : hip_fail(e, "builder device add copy", __LINE__);
    if (rc) {
        int expect = BSDB_OK;
        b->copy_failed.compare_exchange_strong(expect, rc);
    }
    copying.unlock();
    if (rc) {
        std::lock_guard<std::mutex> gb(b->mu);
        if (!b->failed) b->failed = rc;
    }
    return rc;
}

// An input file being read: a host buffer of one chunk, its fill, the tail
// carried over a cut.
struct TextReader {
    int fd = -1;
    uint64_t pos = 0;  // file offset of the next read
    bool eof = false;
    ~TextReader() {
        if (fd >= 0) close(fd);
    }
    // up to `want` bytes at buf; 0 at the end of the file, -1 on an error
    int64_t fill(uint8_t *buf, uint64_t want) {
        uint64_t got = 0;
        while (got < want && !eof) {
            const ssize_t r = pread(fd, buf + got, want - got, (off_t)(pos + got));
            if (r < 0 && errno == EINTR) continue;
            if (r < 0) return -1;
            if (r == 0) eof = true;
            else got += (uint64_t)r;
        }
        pos += got;
        return (int64_t)got;
    }
};

// The files of a call, opened in the order given; total_bytes: the sum of their sizes.
int text_open_inputs(const char *const *paths, int nfiles, std::vector<TextReader> &in, uint64_t &total_bytes) {
    total_bytes = 0;
    for (int f = 0; f < nfiles; ++f) {
        struct stat st;
        if ((in[f].fd = ::open(paths[f], O_RDONLY)) < 0 || fstat(in[f].fd, &st) != 0) return BSDB_EFILE;
        total_bytes += (uint64_t)std::max<off_t>(st.st_size, 0);
    }
    return BSDB_OK;
}

// The read loop of bsdb_text_build and bsdb_db_check_text: every file a chunk
// at a time through hbuf (`chunk` bytes), cut after the chunk's last line end
// (text_cut), the tail carried to the next chunk; chunks never span files.
// step(file, file offset of the chunk's first byte, the chunk, its bytes) per
// chunk; BSDB_E2BIG for a line longer than a chunk.
template <class Step>
int text_read_chunks(std::vector<TextReader> &in, std::vector<uint8_t> &hbuf, uint64_t chunk, Step &&step) {
    for (size_t f = 0; f < in.size(); ++f) {
        TextReader &r = in[f];
        uint64_t fill = 0;  // bytes in hbuf: the tail carried over the last cut, then what was read
        for (;;) {
            const int64_t got = r.fill(hbuf.data() + fill, chunk - fill);
            if (got < 0) return BSDB_EFILE;
            fill += (uint64_t)got;
            if (fill == chunk && !r.eof) {  // (a file that ends with the buffer: its last line needs no terminator)
                uint8_t probe;
                const ssize_t pr = pread(r.fd, &probe, 1, (off_t)r.pos);
                if (pr < 0) return BSDB_EFILE;
                r.eof = pr == 0;
            }
            if (!fill) break;  // (the end of the file, nothing carried)
            const uint64_t cut = text_cut(hbuf.data(), fill, r.eof);
            if (!cut) return BSDB_E2BIG;  // a full buffer without a line end: a line longer than the chunk
            const int rc = step((int)f, r.pos - fill, hbuf.data(), cut);
            if (rc) return rc;
            // the tail after the cut opens the next chunk
            fill -= cut;
            if (fill) memmove(hbuf.data(), hbuf.data() + cut, fill);
            if (r.eof && !fill) break;
        }
    }
    return BSDB_OK;
}

// the device buffers of one bsdb_text_build call (freed when it ends)
struct TextBufs {
    DevBuf text, desc, image, blob, off, addr, v8, vl, report;
    ~TextBufs() {
        for (DevBuf *q : {&text, &desc, &image, &blob, &off, &addr, &v8, &vl, &report}) q->free();
    }
};

bool write_all(int fd, const uint8_t *buf, uint64_t bytes, uint64_t off) {
    uint64_t w = 0;
    while (w < bytes) {
        const ssize_t r = pwrite(fd, buf + w, bytes - w, (off_t)(off + w));
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) return false;
        w += (uint64_t)r;
    }
    return true;
}

// What one bsdb_text_build call keeps from chunk to chunk.
struct TextBuild {
    bsdb_ctx *c;
    int sep, partitions;
    uint32_t B;  // TextPackIO's
    bool approximate;
    TextBufs bufs;
    std::vector<uint8_t> himg;  // the last chunk's image, its runs back to back
    uint64_t records = 0;       // kept so far
};

// The device step of one chunk, under the context's lock: the `cut` bytes at
// h_text go up and are split, the report comes back (k = the records this
// chunk adds), the buffers grow to the chunk, the records are packed behind
// files of part_size bytes, and the image comes back into tb.himg.
int text_chunk_step(TextBuild &tb, const uint8_t *h_text, uint64_t cut, const uint64_t *part_size, uint64_t *report,
                    uint64_t *run_bytes, uint64_t &k) {
    bsdb_ctx *c = tb.c;
    TextBufs &bufs = tb.bufs;
    std::lock_guard<std::mutex> g(c->mu);
    HIP_OK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    Ordered ord(c, s);
    const uint64_t cap = text_max_records(cut);
    int rc;
    if ((rc = bufs.text.grow(cut + 16)) || (rc = bufs.desc.grow(4 * 4 * cap))) return rc;
    if ((rc = h2d_bounce(s, bufs.text.p, h_text, cut))) return rc;
    uint32_t *desc = bufs.desc.as<uint32_t>();
    unsigned long long *d_report = bufs.report.as<unsigned long long>();
    if ((rc = text_split_impl(c, bufs.text.as<const uint8_t>(), cut, (uint32_t)tb.sep, cap, desc, desc + cap, desc + 2 * cap,
                              desc + 3 * cap, d_report, s)))
        return rc;
    HIP_OK(hipMemcpyAsync(report, d_report, 8 * TW_WORDS, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    k = report[TW_RECORDS] - tb.records;
    tb.records = report[TW_RECORDS];
    if (k > cap) return BSDB_EIO;
    if (!k) return BSDB_OK;
    const uint64_t image_max = tb.B ? text_image_max_blocked(cut, tb.partitions, tb.B) : text_image_max(cut);
    if ((rc = bufs.image.grow(image_max)) || (rc = bufs.blob.grow(text_blob_max(cut))) || (rc = bufs.off.grow(8 * (k + 1))) ||
        (rc = bufs.addr.grow(8 * k)) || (tb.approximate && ((rc = bufs.v8.grow(8 * k)) || (rc = bufs.vl.grow(k)))))
        return rc;
    const TextPackIO io{bufs.text.as<const uint8_t>(), cut, {desc, desc + cap, desc + 2 * cap, desc + 3 * cap}, k, tb.partitions, tb.B,
                        part_size, bufs.image.as<uint8_t>(), image_max, run_bytes, bufs.addr.as<uint64_t>(),
                        bufs.blob.as<uint8_t>(), text_blob_max(cut), bufs.off.as<uint64_t>(), nullptr,
                        tb.approximate ? bufs.v8.as<uint64_t>() : nullptr, tb.approximate ? bufs.vl.as<uint8_t>() : nullptr};
    uint64_t image_bytes = 0;
    if ((rc = text_pack_impl(c, io, s))) return rc;
    for (int p = 0; p < tb.partitions; ++p) image_bytes += run_bytes[p];
    try {
        if (tb.himg.size() < image_bytes) tb.himg.resize(image_bytes);
    } catch (const std::bad_alloc &) {
        return BSDB_ENOMEM;
    }
    HIP_OK(hipMemcpyAsync(tb.himg.data(), bufs.image.p, image_bytes, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    return launch_status();
}

}  // namespace

extern "C" {

uint64_t bsdb_text_max_records(uint64_t bytes) { return text_max_records(bytes); }

int bsdb_dev_text_split(bsdb_ctx *c, const uint8_t *d_text, uint64_t bytes, int sep, uint64_t cap, uint32_t *d_kpos,
                        uint32_t *d_klen, uint32_t *d_vpos, uint32_t *d_vlen, uint64_t *d_report, void *stream) {
    if (!c || text_bad_separator(sep) || bytes > TEXT_MAX_BYTES || !d_report || ((uintptr_t)d_report & 7) ||
        (bytes && !d_text) || !aligned16(d_text) || cap < text_max_records(bytes) || !d_kpos || !d_klen || !d_vpos ||
        !d_vlen || (((uintptr_t)d_kpos | (uintptr_t)d_klen | (uintptr_t)d_vpos | (uintptr_t)d_vlen) & 3))
        return BSDB_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    HIP_OK(hipSetDevice(c->device));
    hipStream_t s = pick(c, stream);
    Ordered ord(c, s);
    return text_split_impl(c, d_text, bytes, (uint32_t)sep, cap, d_kpos, d_klen, d_vpos, d_vlen,
                           (unsigned long long *)d_report, s);
}

int bsdb_dev_text_pack(bsdb_ctx *c, const uint8_t *d_text, uint64_t bytes, const uint32_t *d_kpos, const uint32_t *d_klen,
                       const uint32_t *d_vpos, const uint32_t *d_vlen, uint64_t count, int partitions,
                       const uint64_t *h_part_size, uint8_t *d_image, uint64_t image_cap, uint64_t *h_run_bytes,
                       uint64_t *d_addr, uint8_t *d_blob, uint64_t blob_cap, uint64_t *d_off, uint64_t *h_blob_bytes,
                       uint64_t *d_value8, uint8_t *d_value_len, void *stream) {
    const TextPackIO io{d_text, bytes, {d_kpos, d_klen, d_vpos, d_vlen}, count, partitions, 0, h_part_size, d_image, image_cap,
                        h_run_bytes, d_addr, d_blob, blob_cap, d_off, h_blob_bytes, d_value8, d_value_len};
    if (text_pack_bad_args(c, io)) return BSDB_EINVAL;
    return text_pack_locked(c, io, stream);
}

uint64_t bsdb_text_image_max(uint64_t bytes, int partitions, int format, uint32_t block_size) {
    return format == 1 ? text_image_max_blocked(bytes, partitions, block_size) : text_image_max(bytes);
}

int bsdb_dev_text_pack_blocked(bsdb_ctx *c, const uint8_t *d_text, uint64_t bytes, const uint32_t *d_kpos, const uint32_t *d_klen,
                               const uint32_t *d_vpos, const uint32_t *d_vlen, uint64_t count, int partitions,
                               uint32_t block_size, const uint64_t *h_part_size, uint8_t *d_image, uint64_t image_cap,
                               uint64_t *h_run_bytes, uint64_t *d_addr, uint8_t *d_blob, uint64_t blob_cap, uint64_t *d_off,
                               uint64_t *h_blob_bytes, uint64_t *d_value8, uint8_t *d_value_len, void *stream) {
    const TextPackIO io{d_text, bytes, {d_kpos, d_klen, d_vpos, d_vlen}, count, partitions, block_size, h_part_size, d_image, image_cap,
                        h_run_bytes, d_addr, d_blob, blob_cap, d_off, h_blob_bytes, d_value8, d_value_len};
    if (text_pack_bad_args(c, io) || text_bad_block_size(block_size)) return BSDB_EINVAL;
    for (int p = 0; p < partitions; ++p)
        if ((h_part_size[p] & (TEXT_PAGE - 1)) || h_part_size[p] > TEXT_MAX_FILE_BLOCKED) return BSDB_EINVAL;
    return text_pack_locked(c, io, stream);
}

int bsdb_builder_add_dev_var(bsdb_builder *b, const uint8_t *d_blob, const uint64_t *d_off, uint64_t count,
                             const uint64_t *d_addr, const uint64_t *d_value8, const uint8_t *d_vlen, void *stream) {
    if (!b || b->key_len || (count && (!d_blob || !d_off)) ||
        (((uintptr_t)d_off | (uintptr_t)d_addr | (uintptr_t)d_value8) & 7))
        return BSDB_EINVAL;
    return builder_add_dev(b, d_blob, d_off, count, d_addr, d_value8, d_vlen, pick(b->c, stream));
}

int bsdb_text_set_chunk(bsdb_ctx *c, uint64_t bytes) {
    if (!c) return BSDB_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    c->text_chunk = bytes;
    return BSDB_OK;
}

int bsdb_text_build(bsdb_ctx *c, const char *const *paths, int nfiles, int sep, const char *kv_base, int partitions,
                    uint32_t width, int approximate, const char *index_path, const char *index_a_path, uint64_t *report,
                    bsdb_mph **out) {
    return bsdb_text_build_layout(c, paths, nfiles, sep, kv_base, partitions, 0, 0, width, approximate, index_path, index_a_path,
                                  report, out);
}

int bsdb_text_build_layout(bsdb_ctx *c, const char *const *paths, int nfiles, int sep, const char *kv_base, int partitions,
                           int format, uint32_t block_size, uint32_t width, int approximate, const char *index_path,
                           const char *index_a_path, uint64_t *report, bsdb_mph **out) {
    if (!c || nfiles < 0 || (nfiles && !paths) || text_bad_separator(sep) || !kv_base || partitions < 1 ||
        partitions > TEXT_MAX_PARTS || width > 64 || !index_path || (approximate && !index_a_path) || !report || !out ||
        (format != 0 && format != 1) || (format == 1 && text_bad_block_size(block_size)))
        return BSDB_EINVAL;
    const bool blocked = format == 1;
    for (int f = 0; f < nfiles; ++f)
        if (!paths[f]) return BSDB_EINVAL;
    *out = nullptr;
    memset(report, 0, sizeof(uint64_t) * BSDB_TEXT_WORDS);
    // the inputs and the partition files
    std::vector<TextReader> in((size_t)nfiles);
    uint64_t total_bytes = 0;
    int rc = text_open_inputs(paths, nfiles, in, total_bytes);
    if (rc) return rc;
    Fd part[TEXT_MAX_PARTS];
    uint64_t part_size[TEXT_MAX_PARTS] = {};
    for (int p = 0; p < partitions; ++p) {
        const std::string path = std::string(kv_base) + "." + std::to_string(p);
        if ((part[p].fd = ::open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644)) < 0) return BSDB_EFILE;
    }
    // the chunk size and the report on the device
    uint64_t chunk = 0;
    TextBuild tb{c, sep, partitions, blocked ? block_size : 0, approximate != 0};
    {
        std::lock_guard<std::mutex> g(c->mu);
        HIP_OK(hipSetDevice(c->device));
        size_t free_b = 0, total_b = 0;
        HIP_OK(hipMemGetInfo(&free_b, &total_b));
        chunk = blocked ? text_chunk_bytes_blocked(c->text_chunk, free_b, partitions, block_size)
                        : text_chunk_bytes(c->text_chunk, free_b);
        if ((rc = tb.bufs.report.grow(8 * TW_WORDS))) return rc;
        HIP_OK(hipMemsetAsync(tb.bufs.report.p, 0, 8 * TW_WORDS, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
    }
    std::vector<uint8_t> hbuf;
    try {
        hbuf.resize(chunk);
    } catch (const std::bad_alloc &) {
        return BSDB_ENOMEM;
    }
    bsdb_builder *b = nullptr;
    if ((rc = bsdb_builder_open(c, 0, total_bytes / 16 + 1024, total_bytes / 2 + 65536, approximate, 0, 0, &b))) return rc;
    struct BuilderGuard {
        bsdb_builder *b;
        ~BuilderGuard() { (void)bsdb_builder_free(b); }
    } guard{b};
    const TextBufs &bufs = tb.bufs;
    rc = text_read_chunks(in, hbuf, chunk, [&](int, uint64_t, const uint8_t *h_text, uint64_t cut) -> int {
        uint64_t run_bytes[TEXT_MAX_PARTS] = {}, k = 0;
        int r2 = text_chunk_step(tb, h_text, cut, part_size, report, run_bytes, k);
        if (r2 || !k) return r2;
        // the image's runs lie back to back: P plain copies, each appended to its file
        uint64_t at = 0;
        for (int p = 0; p < partitions; ++p) {
            if (!write_all(part[p].fd, tb.himg.data() + at, run_bytes[p], part_size[p])) return BSDB_EFILE;
            at += run_bytes[p];
            part_size[p] += run_bytes[p];
        }
        return builder_add_dev(b, bufs.blob.as<const uint8_t>(), bufs.off.as<const uint64_t>(), k, bufs.addr.as<const uint64_t>(),
                               approximate ? bufs.v8.as<const uint64_t>() : nullptr,
                               approximate ? bufs.vl.as<const uint8_t>() : nullptr, c->stream);
    });
    if (rc) return rc;
    for (int p = 0; p < partitions; ++p) {
        const int fd = part[p].fd;
        part[p].fd = -1;
        if (close(fd) != 0) return BSDB_EFILE;
    }
    return bsdb_builder_finish(b, width, 0, index_path, index_a_path, out, nullptr);
}

}  // extern "C"
