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

// The pack of one chunk's `count` records; the caller holds the context's lock
// and has set the device.  Waits for the scans (the sizes go back to the
// host, and nothing is written before they are known to fit).
int text_pack_impl(bsdb_ctx *c, const uint8_t *d_text, uint64_t bytes, const TextDesc &d, uint64_t count, int partitions,
                   const uint64_t *h_part_size, uint8_t *d_image, uint64_t image_cap, uint64_t *h_run_bytes,
                   uint64_t *d_addr, uint8_t *d_blob, uint64_t blob_cap, uint64_t *d_off, uint64_t *h_blob_bytes,
                   uint64_t *d_value8, uint8_t *d_value_len, hipStream_t s) {
    for (int p = 0; p < partitions; ++p) h_run_bytes[p] = 0;
    if (h_blob_bytes) *h_blob_bytes = 0;
    if (!count) {
        if (d_off) HIP_OK(hipMemsetAsync(d_off, 0, 8, s));
        return BSDB_OK;
    }
    int rc;
    if ((rc = c->t_size.grow(2 * 4 * count)) || (rc = c->t_roff.grow(8 * (count + 1)))) return rc;
    uint32_t *rsize = c->t_size.as<uint32_t>(), *ksize = rsize + count;
    uint64_t *roff = c->t_roff.as<uint64_t>();
    const uint32_t lgrid = text_lane_grid(count, c->num_cus);
    k_text_sizes<<<lgrid, 256, 0, s>>>(d.klen, d.vlen, count, rsize, ksize);
    if ((rc = text_scan(c, rsize, count, roff, s))) return rc;
    if (d_off && (rc = text_scan(c, ksize, count, d_off, s))) return rc;
    TextRuns runs{};
    runs.partitions = (uint32_t)partitions;
    uint64_t at[TEXT_MAX_PARTS + 1] = {}, blob_bytes = 0;
    for (int p = 0; p <= partitions; ++p) {
        runs.bound[p] = text_run_bound(count, (uint32_t)partitions, (uint32_t)p);
        HIP_OK(hipMemcpyAsync(&at[p], roff + runs.bound[p], 8, hipMemcpyDeviceToHost, s));
    }
    if (d_off) HIP_OK(hipMemcpyAsync(&blob_bytes, d_off + count, 8, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    const uint64_t image_bytes = at[partitions];
    if ((d_image && image_bytes > image_cap) || (d_blob && blob_bytes > blob_cap)) return BSDB_EINVAL;
    for (int p = 0; p < partitions; ++p) {
        const uint64_t run = at[p + 1] - at[p];
        if (h_part_size[p] > TEXT_MAX_FILE || run > TEXT_MAX_FILE - h_part_size[p]) return BSDB_EINVAL;
        runs.file_base[p] = h_part_size[p] - at[p];  // (+ roff[r] >= at[p]: the sum never wraps past the file offset)
    }
    TextPack a{};
    a.text = d_text;
    a.bytes = bytes;
    a.kpos = d.kpos;
    a.klen = d.klen;
    a.vpos = d.vpos;
    a.vlen = d.vlen;
    a.count = count;
    if (d_image) {
        a.off = roff;
        a.dst = d_image;
        a.out_bytes = image_bytes;
        k_text_pack<true><<<text_pack_grid(image_bytes, (uint32_t)((uintptr_t)d_image & 15), c->num_cus), 256, 0, s>>>(a);
    }
    if (d_blob && blob_bytes) {
        a.off = d_off;
        a.dst = d_blob;
        a.out_bytes = blob_bytes;
        k_text_pack<false><<<text_pack_grid(blob_bytes, (uint32_t)((uintptr_t)d_blob & 15), c->num_cus), 256, 0, s>>>(a);
    }
    if (d_addr || d_value8)
        k_text_outputs<<<lgrid, 256, 0, s>>>(runs, d_text, bytes, d.vpos, d.vlen, roff, count, d_addr, d_value8, d_value_len);
    if ((rc = launch_status())) return rc;
    for (int p = 0; p < partitions; ++p) h_run_bytes[p] = at[p + 1] - at[p];
    if (h_blob_bytes) *h_blob_bytes = blob_bytes;
    return BSDB_OK;
}

// text_pack_impl for the blocked layout (text_blocked_kernels.hip): blocks of
// `B` bytes, run p appended to a file of h_part_size[p] bytes (a multiple of
// 4096).  Waits once, for the placement: the runs' bytes are the events' sums
// plus the block each run with a small record leaves open at its end.
int text_pack_blocked_impl(bsdb_ctx *c, const uint8_t *d_text, uint64_t bytes, const TextDesc &d, uint64_t count, int partitions,
                           uint32_t B, const uint64_t *h_part_size, uint8_t *d_image, uint64_t image_cap,
                           uint64_t *h_run_bytes, uint64_t *d_addr, uint8_t *d_blob, uint64_t blob_cap, uint64_t *d_off,
                           uint64_t *h_blob_bytes, uint64_t *d_value8, uint8_t *d_value_len, hipStream_t s) {
    for (int p = 0; p < partitions; ++p) h_run_bytes[p] = 0;
    if (h_blob_bytes) *h_blob_bytes = 0;
    if (!count) {
        if (d_off) HIP_OK(hipMemsetAsync(d_off, 0, 8, s));
        return BSDB_OK;
    }
    int rc;
    if ((rc = c->t_size.grow(2 * 4 * count)) || (rc = c->t_blk.grow(text_place_workspace(count)))) return rc;
    const uint32_t tiles = (uint32_t)((count + TEXT_TILE - 1) / TEXT_TILE);
    uint32_t *rsize = c->t_size.as<uint32_t>(), *ksize = rsize + count;
    // the workspace, 8-byte arrays first
    uint64_t *S = c->t_blk.as<uint64_t>(), *E = S + count + 1, *PS = E + count + 1, *PL = PS + count + 1;
    uint2 *exl = reinterpret_cast<uint2 *>(PL + count + 1);
    uint32_t *ssize = reinterpret_cast<uint32_t *>(exl + count), *next = ssize + count, *ev = next + count, *boff = ev + count,
             *bend = boff + count, *entry = bend + count, *carry = entry + tiles;
    const uint32_t lgrid = text_lane_grid(count, c->num_cus);
    TextRuns runs{};
    runs.partitions = (uint32_t)partitions;
    for (int p = 0; p <= partitions; ++p) runs.bound[p] = text_run_bound(count, (uint32_t)partitions, (uint32_t)p);
    k_blk_sizes<<<lgrid, 256, 0, s>>>(d.klen, d.vlen, count, B, rsize, ksize, ssize);
    if ((rc = text_scan(c, ssize, count, S, s))) return rc;
    if (d_off && (rc = text_scan(c, ksize, count, d_off, s))) return rc;
    HIP_OK(hipMemsetAsync(entry, 0, 2 * 4 * (size_t)tiles, s));
    k_blk_tile<<<tiles, 256, 0, s>>>(runs, S, count, B, next, exl);
    k_blk_chase<<<(uint32_t)partitions, 64, 0, s>>>(runs, exl, count, tiles, entry, carry);
    k_blk_flags<<<tiles, 256, 0, s>>>(runs, S, rsize, next, entry, carry, count, B, ev, boff, bend);
    if ((rc = text_scan(c, ev, count, E, s))) return rc;
    uint64_t e_at[TEXT_MAX_PARTS + 1] = {}, s_at[TEXT_MAX_PARTS + 1] = {}, blob_bytes = 0;
    for (int p = 0; p <= partitions; ++p) {
        HIP_OK(hipMemcpyAsync(&e_at[p], E + runs.bound[p], 8, hipMemcpyDeviceToHost, s));
        HIP_OK(hipMemcpyAsync(&s_at[p], S + runs.bound[p], 8, hipMemcpyDeviceToHost, s));
    }
    if (d_off) HIP_OK(hipMemcpyAsync(&blob_bytes, d_off + count, 8, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    TextBlockedRuns br{};
    uint64_t run[TEXT_MAX_PARTS] = {}, image_bytes = 0;
    for (int p = 0; p < partitions; ++p) {
        run[p] = e_at[p + 1] - e_at[p] + (s_at[p + 1] > s_at[p] ? B : 0);
        if (h_part_size[p] > TEXT_MAX_FILE_BLOCKED || run[p] > TEXT_MAX_FILE_BLOCKED - h_part_size[p]) return BSDB_EINVAL;
        br.image_base[p] = image_bytes;
        br.file_size[p] = h_part_size[p];
        image_bytes += run[p];
    }
    if ((d_image && image_bytes > image_cap) || (d_blob && blob_bytes > blob_cap)) return BSDB_EINVAL;
    if (d_image || d_addr)
        k_blk_place<<<text_lane_grid(count + 1, c->num_cus), 256, 0, s>>>(runs, br, E, rsize, boff, bend, count, B, image_bytes,
                                                                           PS, PL, d_addr);
    TextPack a{};
    a.text = d_text;
    a.bytes = bytes;
    a.kpos = d.kpos;
    a.klen = d.klen;
    a.vpos = d.vpos;
    a.vlen = d.vlen;
    a.count = count;
    if (d_image && image_bytes) {
        TextPackBlocked b{};
        b.t = a;
        b.t.dst = d_image;
        b.t.out_bytes = image_bytes;
        b.PS = PS;
        b.PL = PL;
        b.B = B;
        k_text_pack_blocked<<<text_pack_grid(image_bytes, (uint32_t)((uintptr_t)d_image & 15), c->num_cus), 256, 0, s>>>(b);
    }
    if (d_blob && blob_bytes) {
        a.off = d_off;
        a.dst = d_blob;
        a.out_bytes = blob_bytes;
        k_text_pack<false><<<text_pack_grid(blob_bytes, (uint32_t)((uintptr_t)d_blob & 15), c->num_cus), 256, 0, s>>>(a);
    }
    if (d_value8)
        k_text_outputs<<<lgrid, 256, 0, s>>>(runs, d_text, bytes, d.vpos, d.vlen, nullptr, count, nullptr, d_value8, d_value_len);
    if ((rc = launch_status())) return rc;
    for (int p = 0; p < partitions; ++p) h_run_bytes[p] = run[p];
    if (h_blob_bytes) *h_blob_bytes = blob_bytes;
    return BSDB_OK;
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
    if (!c || bytes > TEXT_MAX_BYTES || (bytes && !d_text) || !aligned16(d_text) || count > text_max_records(bytes) ||
        partitions < 1 || partitions > TEXT_MAX_PARTS || !h_part_size || !h_run_bytes ||
        (count && (!d_kpos || !d_klen || !d_vpos || !d_vlen)) ||
        (((uintptr_t)d_kpos | (uintptr_t)d_klen | (uintptr_t)d_vpos | (uintptr_t)d_vlen) & 3) || (!d_blob != !d_off) ||
        (!d_value8 != !d_value_len) || (((uintptr_t)d_addr | (uintptr_t)d_off | (uintptr_t)d_value8) & 7))
        return BSDB_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    HIP_OK(hipSetDevice(c->device));
    hipStream_t s = pick(c, stream);
    Ordered ord(c, s);
    const TextDesc d{d_kpos, d_klen, d_vpos, d_vlen};
    return text_pack_impl(c, d_text, bytes, d, count, partitions, h_part_size, d_image, image_cap, h_run_bytes, d_addr,
                          d_blob, blob_cap, d_off, h_blob_bytes, d_value8, d_value_len, s);
}

uint64_t bsdb_text_image_max(uint64_t bytes, int partitions, int format, uint32_t block_size) {
    return format == 1 ? text_image_max_blocked(bytes, partitions, block_size) : text_image_max(bytes);
}

int bsdb_dev_text_pack_blocked(bsdb_ctx *c, const uint8_t *d_text, uint64_t bytes, const uint32_t *d_kpos, const uint32_t *d_klen,
                               const uint32_t *d_vpos, const uint32_t *d_vlen, uint64_t count, int partitions,
                               uint32_t block_size, const uint64_t *h_part_size, uint8_t *d_image, uint64_t image_cap,
                               uint64_t *h_run_bytes, uint64_t *d_addr, uint8_t *d_blob, uint64_t blob_cap, uint64_t *d_off,
                               uint64_t *h_blob_bytes, uint64_t *d_value8, uint8_t *d_value_len, void *stream) {
    if (!c || bytes > TEXT_MAX_BYTES || (bytes && !d_text) || !aligned16(d_text) || count > text_max_records(bytes) ||
        partitions < 1 || partitions > TEXT_MAX_PARTS || text_bad_block_size(block_size) || !h_part_size || !h_run_bytes ||
        (count && (!d_kpos || !d_klen || !d_vpos || !d_vlen)) ||
        (((uintptr_t)d_kpos | (uintptr_t)d_klen | (uintptr_t)d_vpos | (uintptr_t)d_vlen) & 3) || (!d_blob != !d_off) ||
        (!d_value8 != !d_value_len) || (((uintptr_t)d_addr | (uintptr_t)d_off | (uintptr_t)d_value8) & 7))
        return BSDB_EINVAL;
    for (int p = 0; p < partitions; ++p)
        if ((h_part_size[p] & (TEXT_PAGE - 1)) || h_part_size[p] > TEXT_MAX_FILE_BLOCKED) return BSDB_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    HIP_OK(hipSetDevice(c->device));
    hipStream_t s = pick(c, stream);
    Ordered ord(c, s);
    const TextDesc d{d_kpos, d_klen, d_vpos, d_vlen};
    return text_pack_blocked_impl(c, d_text, bytes, d, count, partitions, block_size, h_part_size, d_image, image_cap,
                                  h_run_bytes, d_addr, d_blob, blob_cap, d_off, h_blob_bytes, d_value8, d_value_len, s);
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
    for (int f = 0; f < nfiles; ++f) {
        struct stat st;
        if ((in[f].fd = ::open(paths[f], O_RDONLY)) < 0 || fstat(in[f].fd, &st) != 0) return BSDB_EFILE;
        total_bytes += (uint64_t)std::max<off_t>(st.st_size, 0);
    }
    Fd part[TEXT_MAX_PARTS];
    uint64_t part_size[TEXT_MAX_PARTS] = {};
    for (int p = 0; p < partitions; ++p) {
        const std::string path = std::string(kv_base) + "." + std::to_string(p);
        if ((part[p].fd = ::open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644)) < 0) return BSDB_EFILE;
    }
    // the chunk size and the report on the device
    uint64_t chunk = 0;
    TextBufs bufs;
    {
        std::lock_guard<std::mutex> g(c->mu);
        HIP_OK(hipSetDevice(c->device));
        size_t free_b = 0, total_b = 0;
        HIP_OK(hipMemGetInfo(&free_b, &total_b));
        chunk = blocked ? text_chunk_bytes_blocked(c->text_chunk, free_b, partitions, block_size)
                        : text_chunk_bytes(c->text_chunk, free_b);
        int rc = bufs.report.grow(8 * TW_WORDS);
        if (rc) return rc;
        HIP_OK(hipMemsetAsync(bufs.report.p, 0, 8 * TW_WORDS, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
    }
    std::vector<uint8_t> hbuf, himg;
    try {
        hbuf.resize(chunk);
    } catch (const std::bad_alloc &) {
        return BSDB_ENOMEM;
    }
    bsdb_builder *b = nullptr;
    int rc = bsdb_builder_open(c, 0, total_bytes / 16 + 1024, total_bytes / 2 + 65536, approximate, 0, 0, &b);
    if (rc) return rc;
    struct BuilderGuard {
        bsdb_builder *b;
        ~BuilderGuard() { (void)bsdb_builder_free(b); }
    } guard{b};
    uint64_t records = 0;
    for (int f = 0; f < nfiles; ++f) {
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
            uint64_t run_bytes[TEXT_MAX_PARTS] = {}, blob_bytes = 0, k = 0, image_bytes = 0;
            {
                std::lock_guard<std::mutex> g(c->mu);
                HIP_OK(hipSetDevice(c->device));
                hipStream_t s = c->stream;
                Ordered ord(c, s);
                const uint64_t cap = text_max_records(cut);
                if ((rc = bufs.text.grow(cut + 16)) || (rc = bufs.desc.grow(4 * 4 * cap))) return rc;
                if ((rc = h2d_bounce(s, bufs.text.p, hbuf.data(), cut))) return rc;
                uint32_t *desc = bufs.desc.as<uint32_t>();
                const TextDesc d{desc, desc + cap, desc + 2 * cap, desc + 3 * cap};
                unsigned long long *d_report = bufs.report.as<unsigned long long>();
                if ((rc = text_split_impl(c, bufs.text.as<const uint8_t>(), cut, (uint32_t)sep, cap, desc, desc + cap,
                                          desc + 2 * cap, desc + 3 * cap, d_report, s)))
                    return rc;
                HIP_OK(hipMemcpyAsync(report, d_report, 8 * TW_WORDS, hipMemcpyDeviceToHost, s));
                HIP_OK(hipStreamSynchronize(s));
                k = report[TW_RECORDS] - records;
                records = report[TW_RECORDS];
                if (k > cap) return BSDB_EIO;
                if (k) {
                    const uint64_t image_max = blocked ? text_image_max_blocked(cut, partitions, block_size) : text_image_max(cut);
                    if ((rc = bufs.image.grow(image_max)) || (rc = bufs.blob.grow(text_blob_max(cut))) ||
                        (rc = bufs.off.grow(8 * (k + 1))) || (rc = bufs.addr.grow(8 * k)) ||
                        (approximate && ((rc = bufs.v8.grow(8 * k)) || (rc = bufs.vl.grow(k)))))
                        return rc;
                    uint64_t *const v8 = approximate ? bufs.v8.as<uint64_t>() : nullptr;
                    uint8_t *const vl = approximate ? bufs.vl.as<uint8_t>() : nullptr;
                    rc = blocked ? text_pack_blocked_impl(c, bufs.text.as<const uint8_t>(), cut, d, k, partitions, block_size,
                                                          part_size, bufs.image.as<uint8_t>(), image_max, run_bytes,
                                                          bufs.addr.as<uint64_t>(), bufs.blob.as<uint8_t>(), text_blob_max(cut),
                                                          bufs.off.as<uint64_t>(), &blob_bytes, v8, vl, s)
                                 : text_pack_impl(c, bufs.text.as<const uint8_t>(), cut, d, k, partitions, part_size,
                                                  bufs.image.as<uint8_t>(), image_max, run_bytes, bufs.addr.as<uint64_t>(),
                                                  bufs.blob.as<uint8_t>(), text_blob_max(cut), bufs.off.as<uint64_t>(),
                                                  &blob_bytes, v8, vl, s);
                    if (rc) return rc;
                    for (int p = 0; p < partitions; ++p) image_bytes += run_bytes[p];
                    try {
                        if (himg.size() < image_bytes) himg.resize(image_bytes);
                    } catch (const std::bad_alloc &) {
                        return BSDB_ENOMEM;
                    }
                    HIP_OK(hipMemcpyAsync(himg.data(), bufs.image.p, image_bytes, hipMemcpyDeviceToHost, s));
                    HIP_OK(hipStreamSynchronize(s));
                    if ((rc = launch_status())) return rc;
                }
            }
            if (k) {
                // the image's runs lie back to back: P plain copies, each appended to its file
                uint64_t at = 0;
                for (int p = 0; p < partitions; ++p) {
                    if (!write_all(part[p].fd, himg.data() + at, run_bytes[p], part_size[p])) return BSDB_EFILE;
                    at += run_bytes[p];
                    part_size[p] += run_bytes[p];
                }
                if ((rc = builder_add_dev(b, bufs.blob.as<const uint8_t>(), bufs.off.as<const uint64_t>(), k,
                                          bufs.addr.as<const uint64_t>(), approximate ? bufs.v8.as<const uint64_t>() : nullptr,
                                          approximate ? bufs.vl.as<const uint8_t>() : nullptr, c->stream)))
                    return rc;
            }
            // the tail after the cut opens the next chunk
            fill -= cut;
            if (fill) memmove(hbuf.data(), hbuf.data() + cut, fill);
            if (r.eof && !fill) break;
        }
    }
    for (int p = 0; p < partitions; ++p) {
        const int fd = part[p].fd;
        part[p].fd = -1;
        if (close(fd) != 0) return BSDB_EFILE;
    }
    return bsdb_builder_finish(b, width, 0, index_path, index_a_path, out, nullptr);
}

}  // extern "C"
