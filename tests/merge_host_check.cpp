// merge_host_check.cpp -- runs the kernels of the merge of resident databases
// (bsdb_amd/csrc/merge_kernels.hip, included unchanged) on the host, a
// workgroup as the fibers of tests/hostwave/hip/hip_runtime.h, so that ASan +
// UBSan see every address and every shift they make.  Built and run by
// tests/test_merge_host_cpu.py as a program of its own; no GPU, no HIP.  One
// case per line of stdin as key=value tokens (lists: comma separated, the
// image: hex), one JSON line per case.
//
// No slack: the image and every array a kernel reads sit in a heap allocation
// of exactly their length; every output is a view between guard bytes at the
// case's misalignment, and the line says whether every guard byte survived.
// Ground truth is the test's, in Python: this program computes none.
//
// The sequences restate rec_pack_impl and merge_select_step (capi_merge.hip)
// with text_place_compact / text_place_blocked (capi_text.hip); whoever
// changes one changes the other.  op=status: k_merge_status, then the
// selection with mask 1 << KEPT (k_diff_select_flags, a plain prefix sum where
// the library runs k_scan_*, k_diff_select_scatter).  op=pack: k_rec_sizes,
// the scans, for the blocked layout the placement kernels, k_rec_pack<true> or
// k_rec_pack_blocked, k_rec_pack<false>, k_rec_outputs; roff=...: the compact
// image's scan is replaced by the case's list (a size scan that is no scan).
#include "host_check_util.hpp"

#include "diff_kernels.hip"
#include "merge_kernels.hip"

using namespace bsdb;
using namespace hostcheck;

namespace {

template <class T>
void scan(const T *v, uint64_t n, uint64_t *off) {
    uint64_t s = 0;
    for (uint64_t i = 0; i < n; ++i) off[i] = s, s += v[i];
    off[n] = s;
}

int run_status(const Case &c) {
    const std::vector<uint8_t> base = c.list<uint8_t>("base"), delta = c.list<uint8_t>("delta"), removed = c.list<uint8_t>("removed");
    const uint64_t count = base.size();
    const int cus = (int)c.num("cus", 256);
    const bool has_d = c.has("delta"), has_r = c.has("removed");
    if ((has_d && delta.size() != count) || (has_r && removed.size() != count)) return 2;
    Exact<uint8_t> d_base(base), d_delta(delta), d_removed(removed);
    Exact<uint32_t> klen(count), vlen(count), flag(count);
    Exact<uint64_t> ksrc(count), vsrc(count), soff(count + 1);
    for (uint64_t i = 0; i < count; ++i) ksrc[i] = 1000 + i, vsrc[i] = 2000 + i, klen[i] = (uint32_t)(i % 255 + 1), vlen[i] = (uint32_t)(i * 7);
    Guarded<uint8_t> st(count, (uint32_t)c.num("mis", 3));
    Guarded<unsigned long long> report(MW_WORDS, 8);
    Guarded<uint64_t> sel(count, 8), ksrc_out(count, 8), vsrc_out(count, 8), nsel(1, 8);
    Guarded<uint32_t> klen_out(count, 4), vlen_out(count, 12);
    memset(report.view(), 0, 8 * MW_WORDS);
    nsel.view()[0] = 0;
    if (count) {
        MergeStatusArgs a{};
        a.status_base = d_base.p;
        a.status_delta = has_d ? d_delta.p : nullptr;
        a.status_removed = has_r ? d_removed.p : nullptr;
        a.status = st.view();
        a.count = count;
        a.delta_side = (uint32_t)c.num("delta_side", 0);
        a.out = report.view();
        const uint32_t lgrid = merge_lane_grid(count, cus);
        hostwave::launch(lgrid, 256, k_merge_status, a);
        SelectArgs sa{};
        sa.status = st.view();
        sa.count = count;
        sa.mask = MERGE_MASK_KEPT;
        sa.ksrc = ksrc.p, sa.vsrc = vsrc.p, sa.klen = klen.p, sa.vlen = vlen.p;
        sa.flag = flag.p;
        sa.soff = soff.p;
        sa.sel = sel.view();
        sa.ksrc_out = ksrc_out.view(), sa.vsrc_out = vsrc_out.view();
        sa.klen_out = klen_out.view(), sa.vlen_out = vlen_out.view();
        sa.nsel = nsel.view();
        hostwave::launch(lgrid, 256, k_diff_select_flags, sa);
        scan(flag.p, count, soff.p);
        hostwave::launch(lgrid, 256, k_diff_select_scatter, sa);
    }
    const uint64_t k = std::min<uint64_t>(nsel.view()[0], count);
    printf("{\"nsel\":%llu,", (unsigned long long)nsel.view()[0]);
    put_list("status", st.view(), count);
    put_list("report", report.view(), MW_WORDS);
    put_list("sel", sel.view(), k);
    put_list("ksrc", ksrc_out.view(), k);
    put_list("vlen", vlen_out.view(), k);
    printf("\"guard\":%d}\n", (int)(st.intact() && report.intact() && sel.intact() && ksrc_out.intact() && vsrc_out.intact() &&
                                    klen_out.intact() && vlen_out.intact() && nsel.intact()));
    return 0;
}

int run_pack(const Case &c) {
    const uint32_t mis = (uint32_t)c.num("mis", 0), bmis = (uint32_t)c.num("bmis", mis);
    const int cus = (int)c.num("cus", 256);
    const std::vector<uint8_t> image_in = c.hex("image");
    const std::vector<uint64_t> ksrc = c.list<uint64_t>("ksrc"), vsrc = c.list<uint64_t>("vsrc");
    const std::vector<uint32_t> klen = c.list<uint32_t>("klen"), vlen = c.list<uint32_t>("vlen");
    std::vector<uint64_t> before = c.list<uint64_t>("before");
    const uint64_t count = ksrc.size(), bytes = image_in.size();
    const uint32_t P = (uint32_t)c.num("parts", 1), B = (uint32_t)c.num("B", 0);
    before.resize(P, 0);
    if (!count || klen.size() != count || vsrc.size() != count || vlen.size() != count || P < 1 || P > (uint32_t)TEXT_MAX_PARTS ||
        (B && text_bad_block_size(B)))
        return 2;
    Exact<uint8_t> d_image(image_in);
    Exact<uint64_t> d_ksrc(ksrc), d_vsrc(vsrc);
    Exact<uint32_t> d_klen(klen), d_vlen(vlen);
    // text_place + rec_pack_impl
    Exact<uint32_t> rsize(count), ksize(count);
    const uint32_t lgrid = text_lane_grid(count, cus);
    TextRuns runs{};
    runs.partitions = P;
    for (uint32_t p = 0; p <= P; ++p) runs.bound[p] = text_run_bound(count, P, p);
    RecPack pack{d_image.p, bytes, d_ksrc.p, d_vsrc.p, d_klen.p, d_vlen.p, count, nullptr, nullptr, 0};
    Guarded<uint64_t> off(count + 1, 8), addr(count, 8), value8(count, 8);
    Guarded<uint8_t> value_len(count, 7);
    Guarded<unsigned long long> report(MW_WORDS, 8);
    memset(report.view(), 0, 8 * MW_WORDS);
    std::vector<uint64_t> run(P, 0);
    uint64_t image_bytes = 0;
    Exact<uint64_t> roff(B ? 0 : count + 1);
    Guarded<uint8_t> *image = nullptr;
    if (!B) {  // text_place_compact
        hostwave::launch(lgrid, 256, k_rec_sizes, (const uint32_t *)d_klen.p, (const uint32_t *)d_vlen.p, count, B, rsize.p, ksize.p,
                         (uint32_t *)nullptr, report.view());
        scan(rsize.p, count, roff.p);
        scan(ksize.p, count, off.view());
        image_bytes = roff[runs.bound[P]];
        for (uint32_t p = 0; p < P; ++p) {
            run[p] = roff[runs.bound[p + 1]] - roff[runs.bound[p]];
            runs.file_base[p] = before[p] - roff[runs.bound[p]];
        }
        if (c.has("roff")) {
            const std::vector<uint64_t> given = c.list<uint64_t>("roff");
            if (given.size() != count + 1) return 2;
            memcpy(roff.p, given.data(), 8 * (count + 1));
        }
        image = new Guarded<uint8_t>(image_bytes, mis);
        memset(image->view(), 0xEE, image_bytes);  // (the library's buffer is not zeroed: the pack writes every byte)
        RecPack a = pack;
        a.off = roff.p, a.dst = image->view(), a.out_bytes = image_bytes;
        if (image_bytes) hostwave::launch(merge_pack_grid(image_bytes, mis, cus), 256, k_rec_pack<true>, a);
    } else {  // text_place_blocked
        const uint32_t tiles = (uint32_t)((count + TEXT_TILE - 1) / TEXT_TILE);
        Exact<uint64_t> S(count + 1), E(count + 1), PS(count + 1), PL(count + 1);
        Exact<uint2> exl(count);
        Exact<uint32_t> ssize(count), next(count), ev(count), boff(count), bend(count), entry(tiles), carry(tiles);
        hostwave::launch(lgrid, 256, k_rec_sizes, (const uint32_t *)d_klen.p, (const uint32_t *)d_vlen.p, count, B, rsize.p, ksize.p, ssize.p,
                         report.view());
        scan(ssize.p, count, S.p);
        scan(ksize.p, count, off.view());
        memset(entry.p, 0, 4 * (size_t)tiles);
        memset(carry.p, 0, 4 * (size_t)tiles);
        hostwave::launch(tiles, 256, k_blk_tile, runs, (const uint64_t *)S.p, count, B, next.p, exl.p);
        hostwave::launch(P, 64, k_blk_chase, runs, (const uint2 *)exl.p, count, tiles, entry.p, carry.p);
        hostwave::launch(tiles, 256, k_blk_flags, runs, (const uint64_t *)S.p, (const uint32_t *)rsize.p, (const uint32_t *)next.p,
                         (const uint32_t *)entry.p, (const uint32_t *)carry.p, count, B, ev.p, boff.p, bend.p);
        scan(ev.p, count, E.p);
        TextBlockedRuns br{};
        for (uint32_t p = 0; p < P; ++p) {
            const uint64_t b0 = runs.bound[p], b1 = runs.bound[p + 1];
            run[p] = E[b1] - E[b0] + (S[b1] > S[b0] ? B : 0);
            br.image_base[p] = image_bytes;
            br.file_size[p] = before[p];
            image_bytes += run[p];
        }
        image = new Guarded<uint8_t>(image_bytes, mis);
        memset(image->view(), 0xEE, image_bytes);
        hostwave::launch(text_lane_grid(count + 1, cus), 256, k_blk_place, runs, br, (const uint64_t *)E.p, (const uint32_t *)rsize.p,
                         (const uint32_t *)boff.p, (const uint32_t *)bend.p, count, B, image_bytes, PS.p, PL.p, addr.view());
        if (image_bytes) {
            RecPackBlocked b{pack, PS.p, PL.p, B};
            b.t.dst = image->view();
            b.t.out_bytes = image_bytes;
            hostwave::launch(merge_pack_grid(image_bytes, mis, cus), 256, k_rec_pack_blocked, b);
        }
    }
    const uint64_t blob_bytes = off.view()[count];
    Guarded<uint8_t> blob(blob_bytes, bmis);
    if (blob_bytes) {
        RecPack a = pack;
        a.off = off.view(), a.dst = blob.view(), a.out_bytes = blob_bytes;
        hostwave::launch(merge_pack_grid(blob_bytes, bmis, cus), 256, k_rec_pack<false>, a);
    }
    hostwave::launch(lgrid, 256, k_rec_outputs, runs, (const uint8_t *)d_image.p, bytes, (const uint64_t *)d_vsrc.p,
                     (const uint32_t *)d_vlen.p, B ? (const uint64_t *)nullptr : (const uint64_t *)roff.p, count,
                     B ? (uint64_t *)nullptr : addr.view(), value8.view(), value_len.view());
    printf("{");
    put_hex("image", image->view(), image_bytes);
    put_hex("blob", blob.view(), blob_bytes);
    put_list("run_bytes", run.data(), P);
    put_list("off", off.view(), count + 1);
    put_list("addr", addr.view(), count);
    put_list("value8", value8.view(), count);
    put_list("value_len", value_len.view(), count);
    put_list("report", report.view(), MW_WORDS);
    printf("\"guard\":%d}\n", (int)(image->intact() && blob.intact() && off.intact() && addr.intact() && value8.intact() &&
                                    value_len.intact() && report.intact()));
    delete image;
    return 0;
}

}  // namespace

int main() {
    return run_lines([](const Case &c) { return c.str("op") == "status" ? run_status(c) : run_pack(c); });
}
