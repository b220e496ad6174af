// check_host_check.cpp -- runs the kernels of the check of a database against
// text input (bsdb_amd/csrc/check_kernels.hip, included unchanged) on the host,
// a workgroup as the fibers of tests/hostwave/hip/hip_runtime.h, so that ASan +
// UBSan see every address and every shift they make.  Built and run by
// tests/test_check_host_cpu.py as a program of its own; no GPU, no HIP.  One
// case per line of stdin as key=value tokens (lists: comma separated, text and
// image: hex), one JSON line per case.
//
// No slack: the text, the image and every array a kernel reads sit in a heap
// allocation of exactly their length (text and image 16-byte aligned); the
// status array and the report are views between guard bytes, and the line
// says whether every guard byte survived.  Ground truth is the test's, in
// Python: this program computes none.
//
// The sequence restates check_launch (capi_check.hip); whoever changes one
// changes the other: k_check_lengths, the scan (a plain prefix sum where the
// library runs k_scan_*), k_check_values, k_check_report; approx=1:
// k_check_approx, k_check_report.  coff=...: the scan is replaced by the
// case's list (offsets that are no scan).
#include "host_check_util.hpp"

#include "check_kernels.hip"

using namespace bsdb;
using namespace hostcheck;

namespace {

int run_check(const Case &c) {
    const std::vector<uint8_t> text = c.hex("text"), image = c.hex("image"), status = c.list<uint8_t>("status");
    const std::vector<uint32_t> vpos = c.list<uint32_t>("vpos"), vlen = c.list<uint32_t>("vlen"), dbvlen = c.list<uint32_t>("dbvlen");
    const std::vector<uint64_t> src = c.list<uint64_t>("src");
    const uint64_t count = status.size();
    const int cus = (int)c.num("cus", 256);
    const bool approx = c.num("approx", 0) != 0;
    if (vpos.size() != count || vlen.size() != count || dbvlen.size() != count || src.size() != count) return 2;
    Exact<uint8_t> d_text(text), d_image(image);
    Exact<uint32_t> d_vpos(vpos), d_vlen(vlen), d_dbvlen(dbvlen), cmp_len(count);
    Exact<uint64_t> d_src(src), coff(count + 1);
    Guarded<uint8_t> st(count, (uint32_t)c.num("mis", 3));
    Guarded<unsigned long long> report(CW_WORDS, 8);
    memset(report.view(), 0, 8 * CW_WORDS);
    report.view()[CW_FIRST_BAD] = CHECK_NONE;
    if (count) {  // check_launch
        memcpy(st.view(), status.data(), count);
        CheckArgs a{};
        a.text = d_text.p;
        a.text_bytes = text.size();
        a.image = d_image.p;
        a.image_bytes = image.size();
        a.vpos = d_vpos.p;
        a.vlen = d_vlen.p;
        a.src = d_src.p;
        a.dbvlen = d_dbvlen.p;
        a.status = st.view();
        a.count = count;
        a.cmp_len = cmp_len.p;
        a.coff = coff.p;
        a.record_base = c.num("record_base", 0);
        a.out = report.view();
        const uint32_t lgrid = check_lane_grid(count, cus);
        if (approx) {
            hostwave::launch(lgrid, 256, k_check_approx, a);
        } else {
            hostwave::launch(lgrid, 256, k_check_lengths, a);
            uint64_t s = 0;
            for (uint64_t i = 0; i < count; ++i) coff.p[i] = s, s += cmp_len.p[i];
            coff.p[count] = s;
            if (c.has("coff")) {
                const std::vector<uint64_t> given = c.list<uint64_t>("coff");
                if (given.size() != count + 1) return 2;
                memcpy(coff.p, given.data(), 8 * (count + 1));
            }
            hostwave::launch(check_values_grid(text.size(), cus), 256, k_check_values, a);
        }
        hostwave::launch(lgrid, 256, k_check_report, (const uint8_t *)st.view(), count, a.record_base, report.view());
    }
    printf("{\"status\":[");
    for (uint64_t i = 0; i < count; ++i) printf("%s%u", i ? "," : "", (unsigned)st.view()[i]);
    printf("],\"report\":[");
    for (int i = 0; i < CW_WORDS; ++i) printf("%s%llu", i ? "," : "", report.view()[i]);
    printf("],\"guard\":%d}\n", (int)(st.intact() && report.intact()));
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
        const int rc = run_check(c);
        if (rc) return rc;
        fflush(stdout);
    }
    return 0;
}
