// piece_host_check.cpp -- runs the output-driven copy kernels (piece_copy.hpp:
// k_get_gather, k_text_pack, k_text_pack_blocked) and the text split and
// block placement kernels on the host, a workgroup as the fibers of
// tests/hostwave/hip/hip_runtime.h, so that ASan + UBSan see every address and
// every shift they make.  Built and run by tests/test_piece_host_cpu.py as a
// program of its own; no GPU, no HIP.  One case per line of stdin as key=value
// tokens (lists: comma separated, the text: hex), one JSON line per case.
//
// No slack: every buffer a kernel reads is a heap allocation of its own,
// exactly as long as the kernel is told (the text and the image 16-byte
// aligned); every buffer a kernel writes for the caller is a view, at the
// requested misalignment, inside an allocation filled with guard bytes, and the
// line reports whether every guard byte survived.  Ground truth is the test's,
// in Python: this program computes none.
//
// The modes restate launch sequences of the library; whoever changes one
// changes the other:
//   gather        get_gather_launch (capi_get.hip): k_get_gather.  Image byte i
//                 is (i * 131 + 7) & 0xFF.
//   pack          text_pack_impl + text_place_compact (capi_text.hip)
//   pack_blocked  text_pack_impl + text_place_blocked (capi_text.hip)
//   split         text_split_impl (capi_text.hip)
// with a plain prefix sum where the library runs k_scan_* (edge_offsets_impl).
#include "host_check_util.hpp"

#include "get_kernels.hip"
#include "text_blocked_kernels.hip"

using namespace bsdb;
using namespace hostcheck;

namespace {

// the exclusive scan of counts[m] into off[m + 1]: what k_scan_* computes
template <class T>
void scan(const T *counts, size_t m, uint64_t *off) {
    uint64_t s = 0;
    for (size_t i = 0; i < m; ++i) off[i] = s, s += counts[i];
    off[m] = s;
}

int run_gather(const Case &c) {
    const uint32_t mis = (uint32_t)c.num("mis", 0);
    const std::vector<uint64_t> voff = c.list<uint64_t>("voff"), src = c.list<uint64_t>("src");
    if (voff.size() != src.size() + 1) return 2;
    const uint64_t image_bytes = c.num("image_bytes", 0), value_bytes = c.num("value_bytes", voff.back());
    Exact<uint8_t> image(image_bytes);
    for (uint64_t i = 0; i < image_bytes; ++i) image[i] = (uint8_t)((i * 131 + 7) & 0xFF);
    Exact<uint64_t> d_voff(voff), d_src(src);
    Guarded<uint8_t> out(value_bytes, mis);
    if (src.size() && value_bytes) {
        GatherArgs a{};
        a.image = image.p;
        a.image_bytes = image_bytes;
        a.scale = (uint32_t)c.num("scale", 1);
        a.src = d_src.p;
        a.voff = d_voff.p;
        a.nq = src.size();
        a.values = out.view();
        a.value_bytes = value_bytes;
        hostwave::launch(piece_grid(value_bytes, mis, (int)c.num("cus", 256)), 256, k_get_gather, a);
    }
    printf("{");
    put_hex("out", out.view(), value_bytes);
    printf("\"guard\":%d}\n", (int)out.intact());
    return 0;
}

// text_pack_too_large: the library refuses (BSDB_EINVAL) before it writes when the sizes pass the caller's buffers
bool too_large(const Case &c, uint64_t image_bytes, uint64_t blob_bytes) {
    if (image_bytes <= c.num("image_cap", UINT64_MAX) && blob_bytes <= c.num("blob_cap", UINT64_MAX)) return false;
    printf("{\"refused\":1,\"image_bytes\":%llu,\"blob_bytes\":%llu}\n", (unsigned long long)image_bytes,
           (unsigned long long)blob_bytes);
    return true;
}

int run_pack(const Case &c, bool blocked) {
    const uint32_t mis = (uint32_t)c.num("mis", 0), bmis = (uint32_t)c.num("bmis", mis);
    const int cus = (int)c.num("cus", 256);
    const std::vector<uint8_t> text = c.hex("text");
    const std::vector<uint32_t> kpos = c.list<uint32_t>("kpos"), klen = c.list<uint32_t>("klen"), vpos = c.list<uint32_t>("vpos"),
                                vlen = c.list<uint32_t>("vlen");
    std::vector<uint64_t> before = c.list<uint64_t>("before");
    const uint64_t count = kpos.size(), bytes = text.size();
    const uint32_t P = (uint32_t)c.num("parts", 1), B = blocked ? (uint32_t)c.num("B", 4096) : 0;
    before.resize(P, 0);
    if (!count || klen.size() != count || vpos.size() != count || vlen.size() != count || P < 1 || P > (uint32_t)TEXT_MAX_PARTS ||
        count > text_max_records(bytes) || (blocked && text_bad_block_size(B)))
        return 2;
    Exact<uint8_t> d_text(text);
    Exact<uint32_t> d_kpos(kpos), d_klen(klen), d_vpos(vpos), d_vlen(vlen);
    // text_pack_impl
    Exact<uint32_t> rsize(count), ksize(count);
    const uint32_t lgrid = text_lane_grid(count, cus);
    TextRuns runs{};
    runs.partitions = P;
    for (uint32_t p = 0; p <= P; ++p) runs.bound[p] = text_run_bound(count, P, p);
    TextPack pack{d_text.p, bytes, d_kpos.p, d_klen.p, d_vpos.p, d_vlen.p, count, nullptr, nullptr, 0};
    Guarded<uint64_t> off(count + 1, 8), addr(count, 8), value8(count, 8);
    Guarded<uint8_t> value_len(count, 7);
    std::vector<uint64_t> run(P, 0);
    uint64_t image_bytes = 0;
    Exact<uint64_t> roff(blocked ? 0 : count + 1);
    Guarded<uint8_t> *image = nullptr;
    if (!blocked) {  // text_place_compact
        hostwave::launch(lgrid, 256, k_text_sizes, d_klen.p, d_vlen.p, count, B, rsize.p, ksize.p, (uint32_t *)nullptr);
        scan(rsize.p, count, roff.p);
        scan(ksize.p, count, off.view());
        image_bytes = roff[runs.bound[P]];
        for (uint32_t p = 0; p < P; ++p) {
            run[p] = roff[runs.bound[p + 1]] - roff[runs.bound[p]];
            runs.file_base[p] = before[p] - roff[runs.bound[p]];
        }
        if (too_large(c, image_bytes, off.view()[count])) return 0;
        image = new Guarded<uint8_t>(image_bytes, mis);
        TextPack a = pack;
        a.off = roff.p, a.dst = image->view(), a.out_bytes = image_bytes;
        hostwave::launch(piece_grid(image_bytes, mis, cus), 256, k_text_pack<true>, a);
    } else {  // text_place_blocked
        const uint32_t tiles = (uint32_t)((count + TEXT_TILE - 1) / TEXT_TILE);
        Exact<uint64_t> S(count + 1), E(count + 1), PS(count + 1), PL(count + 1);
        Exact<uint2> exl(count);
        Exact<uint32_t> ssize(count), next(count), ev(count), boff(count), bend(count), entry(tiles), carry(tiles);
        hostwave::launch(lgrid, 256, k_text_sizes, d_klen.p, d_vlen.p, count, B, rsize.p, ksize.p, ssize.p);
        scan(ssize.p, count, S.p);
        scan(ksize.p, count, off.view());
        memset(entry.p, 0, 4 * (size_t)tiles);
        memset(carry.p, 0, 4 * (size_t)tiles);
        hostwave::launch(tiles, 256, k_blk_tile, runs, S.p, count, B, next.p, exl.p);
        hostwave::launch(P, 64, k_blk_chase, runs, exl.p, count, tiles, entry.p, carry.p);
        hostwave::launch(tiles, 256, k_blk_flags, runs, S.p, rsize.p, next.p, entry.p, carry.p, count, B, ev.p, boff.p, bend.p);
        scan(ev.p, count, E.p);
        TextBlockedRuns br{};
        for (uint32_t p = 0; p < P; ++p) {
            const uint64_t b0 = runs.bound[p], b1 = runs.bound[p + 1];
            run[p] = E[b1] - E[b0] + (S[b1] > S[b0] ? B : 0);
            br.image_base[p] = image_bytes;
            br.file_size[p] = before[p];
            image_bytes += run[p];
        }
        if (too_large(c, image_bytes, off.view()[count])) return 0;
        image = new Guarded<uint8_t>(image_bytes, mis);
        hostwave::launch(text_lane_grid(count + 1, cus), 256, k_blk_place, runs, br, E.p, rsize.p, boff.p, bend.p, count, B, image_bytes,
                         PS.p, PL.p, addr.view());
        if (image_bytes) {
            TextPackBlocked b{pack, PS.p, PL.p, B};
            b.t.dst = image->view();
            b.t.out_bytes = image_bytes;
            hostwave::launch(piece_grid(image_bytes, mis, cus), 256, k_text_pack_blocked, b);
        }
    }
    const uint64_t blob_bytes = off.view()[count];
    Guarded<uint8_t> blob(blob_bytes, bmis);
    if (blob_bytes) {
        TextPack a = pack;
        a.off = off.view(), a.dst = blob.view(), a.out_bytes = blob_bytes;
        hostwave::launch(piece_grid(blob_bytes, bmis, cus), 256, k_text_pack<false>, a);
    }
    hostwave::launch(lgrid, 256, k_text_outputs, runs, d_text.p, bytes, d_vpos.p, d_vlen.p, blocked ? (const uint64_t *)nullptr : roff.p,
                     count, blocked ? (uint64_t *)nullptr : addr.view(), value8.view(), value_len.view());
    printf("{");
    put_hex("image", image->view(), image_bytes);
    put_hex("blob", blob.view(), blob_bytes);
    put_list("run_bytes", run.data(), P);
    put_list("off", off.view(), count + 1);
    put_list("addr", addr.view(), count);
    put_list("value8", value8.view(), count);
    put_list("value_len", value_len.view(), count);
    printf("\"guard\":%d}\n", (int)(image->intact() && blob.intact() && off.intact() && addr.intact() && value8.intact() &&
                                    value_len.intact()));
    delete image;
    return 0;
}

int run_split(const Case &c) {
    const std::vector<uint8_t> text = c.hex("text");
    const uint64_t bytes = text.size(), cap = text_max_records(bytes);
    const uint32_t sep = (uint32_t)c.num("sep", 32);
    const int cus = (int)c.num("cus", 256);
    if (text_bad_separator((int)sep)) return 2;
    Exact<uint8_t> d_text(text);
    Guarded<uint32_t> kpos(cap, 4), klen(cap, 4), vpos(cap, 4), vlen(cap, 4);
    Guarded<unsigned long long> report(TW_WORDS, 8);
    memset(report.view(), 0, 8 * TW_WORDS);
    uint64_t records = 0;
    if (bytes) {  // text_split_impl
        const uint64_t nb = text_blocks(bytes);
        Exact<uint32_t> cnt_st(nb), cnt_sp(nb);
        Exact<uint64_t> off_st(nb + 1), off_sp(nb + 1);
        const uint32_t grid = text_count_grid(bytes);
        hostwave::launch(grid, 256, k_text_count, (const uint8_t *)d_text.p, bytes, sep, cnt_st.p, cnt_sp.p);
        scan(cnt_st.p, nb, off_st.p);
        scan(cnt_sp.p, nb, off_sp.p);
        const uint64_t lines = off_st[nb], seps = off_sp[nb];
        if (lines == 0 || lines > bytes || seps > bytes) return 3;
        Exact<uint32_t> ls(lines), sp(seps), keep(lines);
        Exact<uint64_t> keep_off(lines + 1);
        hostwave::launch(grid, 256, k_text_positions, (const uint8_t *)d_text.p, bytes, sep, (const uint64_t *)off_st.p,
                         (const uint64_t *)off_sp.p, ls.p, lines, sp.p, seps);
        TextSplit a{};
        a.text = d_text.p;
        a.bytes = bytes;
        a.ls = ls.p;
        a.lines = lines;
        a.sp = sp.p;
        a.seps = seps;
        a.keep = keep.p;
        a.keep_off = keep_off.p;
        a.kpos = kpos.view();
        a.klen = klen.view();
        a.vpos = vpos.view();
        a.vlen = vlen.view();
        a.cap = cap;
        a.out = report.view();
        const uint32_t lgrid = text_lane_grid(lines, cus);
        hostwave::launch(lgrid, 256, k_text_records<false>, a);
        scan(keep.p, lines, keep_off.p);
        hostwave::launch(lgrid, 256, k_text_records<true>, a);
        records = keep_off[lines];
        if (records > cap) return 3;
    }
    printf("{");
    put_list("kpos", kpos.view(), records);
    put_list("klen", klen.view(), records);
    put_list("vpos", vpos.view(), records);
    put_list("vlen", vlen.view(), records);
    put_list("report", report.view(), TW_WORDS);
    printf("\"guard\":%d}\n", (int)(kpos.intact() && klen.intact() && vpos.intact() && vlen.intact() && report.intact()));
    return 0;
}

}  // namespace

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream ss(line);
        std::string tok;
        Case c;
        while (ss >> tok) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) return 2;
            c.kv[tok.substr(0, eq)] = tok.substr(eq + 1);
        }
        const std::string mode = c.has("mode") ? c.kv["mode"] : "";
        int rc = 2;
        if (mode == "gather") rc = run_gather(c);
        else if (mode == "pack") rc = run_pack(c, false);
        else if (mode == "pack_blocked") rc = run_pack(c, true);
        else if (mode == "split") rc = run_split(c);
        if (rc) return rc;
        fflush(stdout);
    }
    return 0;
}
