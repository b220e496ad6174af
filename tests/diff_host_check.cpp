// diff_host_check.cpp -- runs the kernels of the diff of two resident databases
// (bsdb_amd/csrc/diff_kernels.hip, included unchanged) on the host, a workgroup
// as the fibers of tests/hostwave/hip/hip_runtime.h, so that ASan + UBSan see
// every address and every shift they make.  Built and run by
// tests/test_diff_host_cpu.py as a program of its own; no GPU, no HIP.  One
// case per line of stdin as key=value tokens (lists: comma separated, images:
// hex), one JSON line per case.
//
// No slack: both images and every array a kernel reads sit in a heap
// allocation of exactly their length (the images 16-byte aligned); the status
// array, the report and the selection's outputs are views between guard bytes,
// and the line says whether every guard byte survived.  Ground truth is the
// test's, in Python: this program computes none.
//
// The sequences restate diff_launch and select_launch (capi_diff.hip); whoever
// changes one changes the other.  op=diff: k_diff_lengths, the scan (a plain
// prefix sum where the library runs k_scan_*), k_diff_values, k_diff_report;
// coff=...: the scan is replaced by the case's list (offsets that are no
// scan).  op=select: k_diff_select_flags, the scan, k_diff_select_scatter.
#include "host_check_util.hpp"

#include "diff_kernels.hip"

using namespace bsdb;
using namespace hostcheck;

namespace {

int run_diff(const Case &c) {
    const std::vector<uint8_t> image_a = c.hex("image_a"), image_b = c.hex("image_b"), status = c.list<uint8_t>("status"),
                               status_a = c.list<uint8_t>("status_a");
    const std::vector<uint32_t> vlen_a = c.list<uint32_t>("vlen_a"), vlen_b = c.list<uint32_t>("vlen_b");
    const std::vector<uint64_t> vsrc_a = c.list<uint64_t>("vsrc_a"), src_b = c.list<uint64_t>("src_b");
    const uint64_t count = status.size();
    const int cus = (int)c.num("cus", 256);
    if (vlen_a.size() != count || vlen_b.size() != count || vsrc_a.size() != count || src_b.size() != count || status_a.size() != count)
        return 2;
    Exact<uint8_t> d_image_a(image_a), d_image_b(image_b), d_status_a(status_a);
    Exact<uint32_t> d_vlen_a(vlen_a), d_vlen_b(vlen_b), cmp_len(count);
    Exact<uint64_t> d_vsrc_a(vsrc_a), d_src_b(src_b), coff(count + 1);
    Guarded<uint8_t> st(count, (uint32_t)c.num("mis", 3));
    Guarded<unsigned long long> report(FW_WORDS, 8);
    memset(report.view(), 0, 8 * FW_WORDS);
    report.view()[FW_FIRST_DIFF] = DIFF_NONE;
    if (count) {  // diff_launch
        memcpy(st.view(), status.data(), count);
        DiffArgs a{};
        a.image_a = d_image_a.p, a.bytes_a = image_a.size();
        a.image_b = d_image_b.p, a.bytes_b = image_b.size();
        a.vsrc_a = d_vsrc_a.p, a.vlen_a = d_vlen_a.p, a.status_a = d_status_a.p;
        a.src_b = d_src_b.p, a.vlen_b = d_vlen_b.p;
        a.status = st.view();
        a.count = count;
        a.cmp_len = cmp_len.p;
        a.coff = coff.p;
        a.slot_base = c.num("slot_base", 0);
        a.out = report.view();
        const uint32_t lgrid = diff_lane_grid(count, cus);
        hostwave::launch(lgrid, 256, k_diff_lengths, a);
        uint64_t s = 0;
        for (uint64_t i = 0; i < count; ++i) coff.p[i] = s, s += cmp_len.p[i];
        coff.p[count] = s;
        if (c.has("coff")) {
            const std::vector<uint64_t> given = c.list<uint64_t>("coff");
            if (given.size() != count + 1) return 2;
            memcpy(coff.p, given.data(), 8 * (count + 1));
        }
        // (the library's grid covers count * 65 535 bytes; the loop is grid-stride, so a smaller one computes the same)
        hostwave::launch(std::min<uint32_t>(diff_values_grid(count, cus), (uint32_t)c.num("vgrid", 8)), 256, k_diff_values, a);
        hostwave::launch(lgrid, 256, k_diff_report, a);
    }
    printf("{");
    put_list("status", st.view(), count);
    put_list("report", report.view(), FW_WORDS);
    printf("\"guard\":%d}\n", (int)(st.intact() && report.intact()));
    return 0;
}

int run_select(const Case &c) {
    const std::vector<uint8_t> status = c.list<uint8_t>("status");
    const std::vector<uint32_t> klen = c.list<uint32_t>("klen"), vlen = c.list<uint32_t>("vlen");
    const std::vector<uint64_t> ksrc = c.list<uint64_t>("ksrc"), vsrc = c.list<uint64_t>("vsrc");
    const uint64_t count = status.size();
    const int cus = (int)c.num("cus", 256);
    if (klen.size() != count || vlen.size() != count || ksrc.size() != count || vsrc.size() != count) return 2;
    Exact<uint8_t> d_status(status);
    Exact<uint32_t> d_klen(klen), d_vlen(vlen), flag(count);
    Exact<uint64_t> d_ksrc(ksrc), d_vsrc(vsrc), soff(count + 1);
    Guarded<uint64_t> sel(count, 8), ksrc_out(count, 8), vsrc_out(count, 8), nsel(1, 8);
    Guarded<uint32_t> klen_out(count, 4), vlen_out(count, 12);
    for (Guarded<uint64_t> *g : {&sel, &ksrc_out, &vsrc_out}) memset(g->view(), 0xEE, 8 * count);
    for (Guarded<uint32_t> *g : {&klen_out, &vlen_out}) memset(g->view(), 0xEE, 4 * count);
    nsel.view()[0] = 0;
    if (count) {  // select_launch
        SelectArgs a{};
        a.status = d_status.p;
        a.count = count;
        a.mask = (uint32_t)c.num("mask", 0);
        a.ksrc = d_ksrc.p, a.vsrc = d_vsrc.p, a.klen = d_klen.p, a.vlen = d_vlen.p;
        a.flag = flag.p;
        a.soff = soff.p;
        a.sel = sel.view();
        a.ksrc_out = ksrc_out.view(), a.vsrc_out = vsrc_out.view();
        a.klen_out = klen_out.view(), a.vlen_out = vlen_out.view();
        a.nsel = nsel.view();
        const uint32_t lgrid = diff_lane_grid(count, cus);
        hostwave::launch(lgrid, 256, k_diff_select_flags, a);
        uint64_t s = 0;
        for (uint64_t i = 0; i < count; ++i) soff.p[i] = s, s += flag.p[i];
        soff.p[count] = s;
        hostwave::launch(lgrid, 256, k_diff_select_scatter, a);
    }
    const uint64_t k = std::min<uint64_t>(nsel.view()[0], count);
    printf("{\"nsel\":%llu,", (unsigned long long)nsel.view()[0]);
    put_list("sel", sel.view(), k);
    put_list("ksrc", ksrc_out.view(), k);
    put_list("klen", klen_out.view(), k);
    put_list("vsrc", vsrc_out.view(), k);
    put_list("vlen", vlen_out.view(), k);
    bool untouched = true;  // nothing past the selection was written
    for (uint64_t i = k; i < count; ++i) untouched = untouched && sel.view()[i] == 0xEEEEEEEEEEEEEEEEull && klen_out.view()[i] == 0xEEEEEEEEu;
    printf("\"guard\":%d}\n", (int)(untouched && sel.intact() && ksrc_out.intact() && vsrc_out.intact() && klen_out.intact() &&
                                    vlen_out.intact() && nsel.intact()));
    return 0;
}

}  // namespace

int main() {
    return run_lines([](const Case &c) { return c.str("op") == "select" ? run_select(c) : run_diff(c); });
}
