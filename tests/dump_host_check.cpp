// dump_host_check.cpp -- runs the kernels of the enumeration of a resident
// database (bsdb_amd/csrc/dump_kernels.hip, included unchanged) on the host, a
// workgroup as the fibers of tests/hostwave/hip/hip_runtime.h, so that ASan +
// UBSan see every address and every shift they make.  Built and run by
// tests/test_dump_host_cpu.py as a program of its own; no GPU, no HIP.  One
// case per line of stdin as key=value tokens (lists: comma separated, image:
// hex), one JSON line per case.
//
// No slack: the image, index.db and every array a kernel only reads sit in a
// heap allocation of exactly their length; every output is a view between
// guard bytes (the text and the status at misalignment `mis`, 0 - 15, the
// word arrays at `mis` rounded down to their alignment), and the line says
// whether every guard byte survived.  Ground truth is the test's, in Python:
// this program computes none.
//
// Two stages, each restating its launch in capi_dump.hip; whoever changes one
// changes the other:
//   index=...  k_db_records over slots [first, first + count) of the index
//              (addresses as numbers; stored big-endian as index.db holds them)
//              with the partition table base= / size= and format=
//   sep=...    k_dump_lengths, the scan (a plain prefix sum where the library
//              runs k_scan_*; loff=...: replaced by the case's list, offsets
//              that are no scan), k_dump_text over text_bytes = loff[count]
//              (or text_bytes=...) and k_dump_report; over the first stage's
//              descriptors, or over ksrc= klen= vsrc= vlen= status= given
#include "host_check_util.hpp"

#include "dump_kernels.hip"

using namespace bsdb;
using namespace hostcheck;

namespace {

template <class T>
void print_list(const char *name, const T *p, size_t n) {
    printf("\"%s\":[", name);
    for (size_t i = 0; i < n; ++i) printf("%s%llu", i ? "," : "", (unsigned long long)p[i]);
    printf("],");
}

int run_case(const Case &c) {
    const std::vector<uint8_t> image = c.hex("image");
    const int cus = (int)c.num("cus", 256);
    const uint32_t mis = (uint32_t)c.num("mis", 0);
    const bool stage1 = c.has("index"), stage2 = c.has("sep");
    const uint64_t first = c.num("first", 0);
    std::vector<uint64_t> index = c.list<uint64_t>("index");
    const uint64_t count = stage1 ? c.num("count", index.size() - first) : c.list<uint8_t>("status").size();
    if (stage1 && (first > index.size() || count > index.size() - first)) return 2;
    Exact<uint8_t> d_image(image);
    Guarded<uint64_t> ksrc(count, mis), vsrc(count, mis), loff(count + 1, mis);
    Guarded<uint32_t> klen(count, mis), vlen(count, mis), llen(count, mis);
    Guarded<uint8_t> status(count, mis);
    Guarded<unsigned long long> rep1(DW_WORDS, 8), rep2(DW_WORDS, 8);
    for (Guarded<unsigned long long> *r : {&rep1, &rep2}) {
        memset(r->view(), 0, 8 * DW_WORDS);
        r->view()[DW_FIRST_BAD] = DUMP_NONE;
    }
    bool guard = true;
    printf("{");
    if (stage1) {  // bsdb_dev_db_records
        const std::vector<uint64_t> base = c.list<uint64_t>("base"), size = c.list<uint64_t>("size");
        if (base.empty() || base.size() != size.size()) return 2;
        for (uint64_t &w : index) w = __builtin_bswap64(w);
        Exact<uint64_t> d_index(index), d_base(base), d_size(size);
        GetDb db{};
        db.image = d_image.p;
        db.image_bytes = image.size();
        db.index = d_index.p;
        db.base = d_base.p;
        db.size = d_size.p;
        db.partitions = (uint32_t)c.num("dparts", base.size());
        db.format = (int)c.num("format", 0);
        if (count)
            hostwave::launch(dump_lane_grid(count, cus), 256, k_db_records, db,
                             RecordsArgs{first, count, ksrc.view(), vsrc.view(), klen.view(), vlen.view(), status.view(), rep1.view()});
        print_list("r_ksrc", ksrc.view(), count), print_list("r_vsrc", vsrc.view(), count);
        print_list("r_klen", klen.view(), count), print_list("r_vlen", vlen.view(), count);
        print_list("r_status", status.view(), count), print_list("r_report", rep1.view(), DW_WORDS);
    } else {
        const std::vector<uint64_t> ks = c.list<uint64_t>("ksrc"), vs = c.list<uint64_t>("vsrc");
        const std::vector<uint32_t> kl = c.list<uint32_t>("klen"), vl = c.list<uint32_t>("vlen");
        if (ks.size() != count || vs.size() != count || kl.size() != count || vl.size() != count) return 2;
        ksrc.fill(ks), vsrc.fill(vs), klen.fill(kl), vlen.fill(vl), status.fill(c.list<uint8_t>("status"));
    }
    if (stage2) {  // bsdb_dev_db_dump_lengths, bsdb_dev_db_dump_text
        DumpArgs a{};
        a.image = d_image.p;
        a.image_bytes = image.size();
        a.ksrc = ksrc.view(), a.vsrc = vsrc.view();
        a.klen = klen.view(), a.vlen = vlen.view();
        a.status = status.view();
        a.count = count;
        a.llen = llen.view();
        a.loff = loff.view();
        a.sep = (uint32_t)c.num("sep", 32);
        a.first = first;
        a.out = rep2.view();
        loff.view()[0] = 0;
        if (count) {
            hostwave::launch(dump_lane_grid(count, cus), 256, k_dump_lengths, a);
            uint64_t s = 0;
            for (uint64_t i = 0; i < count; ++i) loff.view()[i] = s, s += llen.view()[i];
            loff.view()[count] = s;
        }
        if (c.has("loff")) {
            const std::vector<uint64_t> given = c.list<uint64_t>("loff");
            if (given.size() != count + 1) return 2;
            loff.fill(given);
        }
        const uint64_t text_bytes = c.num("text_bytes", loff.view()[count]);
        Guarded<uint8_t> text(text_bytes, mis);
        memset(text.view(), 0xEE, text_bytes);
        a.text = text.view();
        a.text_bytes = text_bytes;
        if (count) {  // dump_text_launch
            if (text_bytes) hostwave::launch(dump_text_grid(text_bytes, mis & 15, cus), 256, k_dump_text, a);
            hostwave::launch(dump_lane_grid(count, cus), 256, k_dump_report, a);
        }
        printf("\"text\":\"");
        for (uint64_t i = 0; i < text_bytes; ++i) printf("%02x", text.view()[i]);
        printf("\",");
        print_list("llen", llen.view(), count), print_list("status", status.view(), count);
        print_list("report", rep2.view(), DW_WORDS);
        guard = guard && text.intact();
    }
    guard = guard && ksrc.intact() && vsrc.intact() && loff.intact() && klen.intact() && vlen.intact() && llen.intact() &&
            status.intact() && rep1.intact() && rep2.intact();
    printf("\"guard\":%d}\n", (int)guard);
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
        const int rc = run_case(c);
        if (rc) return rc;
        fflush(stdout);
    }
    return 0;
}
