// locate_host_check.cpp -- runs the kernels that decide whether an address is
// safe to touch on the host: k_get_locate<0|1|2> (get_kernels.hip),
// k_verify_structure, k_verify_fixed<true|false>, k_verify_var
// (verify_kernels.hip), k_lookup, k_sign, k_index_scatter (mph_kernels.hip),
// all included unchanged, a workgroup as the fibers of
// tests/hostwave/hip/hip_runtime.h, so that ASan + UBSan see every address and
// every shift they make.  Built and run by tests/test_locate_host_cpu.py as a
// program of its own; no GPU, no HIP.  One case per line of stdin as key=value
// tokens (lists: comma separated; the image and the keys: hex), one JSON line
// per case.
//
// No slack: E (m + 1 words), values, the checksum bit list, the signatures, the
// index slots, the partition table, the image (layout.total bytes, 16-byte
// aligned) and the keys each end with the last byte of a heap allocation of
// their own, as long as the case says; the keys start at the case's `kmis`
// bytes past a 16-byte aligned address.  Every array a kernel writes (src,
// vlen, status, the reports, the lookup's out, the sign's bit list, index and
// index_a) is a view between guard bytes, and the line says whether every
// guard byte survived ("intact").  Ground truth is the test's, in Python
// (tests/locate_cases.py): this program computes none.
//
// What this proves of the kernels: addressing, arithmetic, uniform control
// flow.  What it does not: the memory model, races between lanes, code
// generation, speed (the shim's opening comment).
//
// The modes restate launch lines of the library; whoever changes one changes
// the other.  The grid is the case's (the test restates get_locate_grid /
// grid_for with a small number of CUs):
//   structure  k_verify_structure (capi_verify.hip dev_verify, capi_get.hip db_load)
//   lookup     bsdb_dev_lookup (bsdb_capi.hip): k_lookup
//   sign       bsdb_dev_sign: k_sign into a zeroed bit list
//   scatter    bsdb_dev_index_scatter: k_index_scatter
//   count      count_nonzero_pairs_wide and count_nonzero_pairs on their own,
//              through the one-line kernel k_count below (the library has no
//              launch of its own for them)
//   decode     get_decode (get_plan.hpp), the host and device function the
//              locate kernel calls, on its own
//   locate     get_locate_launch (capi_get.hip): kind 2 with offsets, kind 0
//              for 13-byte keys, else kind 1; the report zeroed
//   verify     dev_verify (capi_verify.hip): k_verify_structure, then
//              verify_launch's kernel of the kind; the report zeroed, [5] all ones
#include "host_check_util.hpp"

#include "get_kernels.hip"

using namespace bsdb;
using namespace hostcheck;

namespace {

constexpr int VERIFY_WORDS = VW_WINDOWS + 1;  // BSDB_VERIFY_WORDS

__global__ void k_count(const uint64_t *a, const uint64_t *span, uint64_t pairs, uint64_t *wide, uint64_t *narrow) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < pairs) wide[i] = count_nonzero_pairs_wide(span[2 * i], span[2 * i + 1], a), narrow[i] = count_nonzero_pairs(span[2 * i], span[2 * i + 1], a);
}

struct HostMph {
    Exact<uint64_t> E, values, sigs;
    uint64_t n, m;
    uint32_t width;
    bool has_sigs;
    explicit HostMph(const Case &c)
        : E(c.list<uint64_t>("E")), values(c.num("no_values", 0) ? std::vector<uint64_t>() : c.list<uint64_t>("values"), (uint32_t)c.num("vmis", 0)),
          sigs(c.list<uint64_t>("sigbits")), n(c.num("n", 0)), m(E.n - 1), width((uint32_t)c.num("width", 0)), has_sigs(c.has("sigbits")) {}
    MphView view() const { return MphView{E.p, values.p, has_sigs ? sigs.p : nullptr, n, (uint32_t)(2 * m), width}; }
};

void put_signed(const char *name, const int64_t *p, size_t n, const char *end = ",") {
    printf("\"%s\":[", name);
    for (size_t i = 0; i < n; ++i) printf("%s%lld", i ? "," : "", (long long)p[i]);
    printf("]%s", end);
}

int run_structure(const Case &c) {
    const Exact<uint64_t> E(c.list<uint64_t>("E"));
    if (!E.n) return 2;
    Guarded<unsigned long long> out(VERIFY_WORDS, 8);
    memset(out.view(), 0, 8 * VERIFY_WORDS);
    hostwave::launch((uint32_t)c.num("grid", 1), 256, k_verify_structure, (const uint64_t *)E.p, (uint64_t)(E.n - 1), c.num("n", 0), out.view());
    printf("{");
    put_list("report", out.view(), VERIFY_WORDS);
    printf("\"intact\":%d}\n", (int)out.intact());
    return 0;
}

int run_lookup(const Case &c) {
    const HostMph mph(c);
    const Exact<uint64_t> sig(c.list<uint64_t>("sig"));
    const uint64_t nq = sig.n / 2;
    Guarded<int64_t> out(nq, 8);
    if (nq) hostwave::launch((uint32_t)c.num("grid", 1), 256, k_lookup, mph.view(), (const uint64_t *)sig.p, nq, (int)c.num("check", 1), out.view());
    printf("{");
    put_signed("out", out.view(), nq);
    printf("\"intact\":%d}\n", (int)out.intact());
    return 0;
}

int run_sign(const Case &c) {
    const HostMph mph(c);
    const Exact<uint64_t> sig(c.list<uint64_t>("sig"));
    const uint64_t n = sig.n / 2, words = c.num("words", 0);
    Guarded<uint64_t> out(words, 8);
    memset(out.view(), 0, 8 * words);
    if (n) hostwave::launch((uint32_t)c.num("grid", 1), 256, k_sign, mph.view(), (const uint64_t *)sig.p, n, out.view());
    printf("{");
    put_list("out", out.view(), words);
    printf("\"intact\":%d}\n", (int)out.intact());
    return 0;
}

int run_scatter(const Case &c) {
    const Exact<int64_t> rank(c.list<int64_t>("rank"));
    const Exact<uint64_t> addr(c.list<uint64_t>("addr")), value8(c.list<uint64_t>("value8"));
    const Exact<uint8_t> value_len(c.list<uint8_t>("value_len"));
    const uint64_t count = rank.n, start = c.num("start", 0), len = c.num("len", 0);
    const bool approx = c.num("approx", 0) != 0;
    if (addr.n != count || (approx && (value8.n != count || value_len.n != count))) return 2;
    Guarded<uint64_t> index(len, 8);
    Guarded<uint8_t> index_a(approx ? 8 * len : 0, 8);
    memset(index.view(), (int)c.num("fill", 0), 8 * len);
    if (approx) memset(index_a.view(), (int)c.num("fill", 0), 8 * len);
    if (count)
        hostwave::launch((uint32_t)c.num("grid", 1), 256, k_index_scatter, (const int64_t *)rank.p, (const uint64_t *)addr.p, count, start, len,
                         index.view(), approx ? (const uint64_t *)value8.p : nullptr, approx ? (const uint8_t *)value_len.p : nullptr,
                         approx ? index_a.view() : nullptr);
    printf("{");
    put_list("index", index.view(), len);
    put_hex("index_a", index_a.view(), approx ? 8 * len : 0);
    printf("\"intact\":%d}\n", (int)(index.intact() && index_a.intact()));
    return 0;
}

int run_count(const Case &c) {
    const Exact<uint64_t> a(c.list<uint64_t>("values"), (uint32_t)c.num("vmis", 0)), span(c.list<uint64_t>("span"));
    const uint64_t pairs = span.n / 2;
    Guarded<uint64_t> wide(pairs, 8), narrow(pairs, 8);
    if (pairs) hostwave::launch((uint32_t)((pairs + 255) / 256), 256, k_count, (const uint64_t *)a.p, (const uint64_t *)span.p, pairs, wide.view(), narrow.view());
    printf("{");
    put_list("wide", wide.view(), pairs);
    put_list("narrow", narrow.view(), pairs);
    printf("\"intact\":%d}\n", (int)(wide.intact() && narrow.intact()));
    return 0;
}

int run_decode(const Case &c) {
    const std::vector<uint64_t> words = c.list<uint64_t>("words");
    const Exact<uint64_t> size(c.list<uint64_t>("size"));
    std::vector<uint64_t> ok, part, pos, limit;
    for (const uint64_t w : words) {
        const GetRecord r = get_decode(w, (int)c.num("format", 0), size.p, (uint32_t)size.n);
        ok.push_back(r.ok), part.push_back(r.ok ? r.part : 0), pos.push_back(r.ok ? r.pos : 0), limit.push_back(r.ok ? r.limit : 0);
    }
    printf("{");
    put_list("ok", ok.data(), ok.size());
    put_list("part", part.data(), part.size());
    put_list("pos", pos.data(), pos.size());
    put_list("limit", limit.data(), limit.size(), "}\n");
    return 0;
}

// the keys of a case: `kmis` past a 16-byte aligned address, ending with their allocation
struct Keys {
    Exact<uint8_t> bytes;
    Exact<uint64_t> off;
    bool var;
    explicit Keys(const Case &c) : bytes(c.hex("keys"), (uint32_t)c.num("kmis", 0)), off(c.list<uint64_t>("off")), var(c.has("off")) {}
};

int run_locate(const Case &c) {
    const HostMph mph(c);
    const Keys keys(c);
    const Exact<uint8_t> image(c.hex("image"));
    const Exact<uint64_t> index(c.list<uint64_t>("index")), base(c.list<uint64_t>("base")), size(c.list<uint64_t>("size"));
    const uint64_t nq = c.num("nq", 0);
    const uint32_t key_len = (uint32_t)c.num("key_len", 0);
    if (base.n != size.n || (keys.var ? keys.off.n != nq + 1 : keys.bytes.n != nq * key_len)) return 2;
    GetDb db{};
    db.image = image.p;
    db.image_bytes = image.n;
    db.index = index.p;
    db.base = base.p;
    db.size = size.p;
    db.partitions = (uint32_t)base.n;
    db.format = (int)c.num("format", 0);
    db.approx = (int)c.num("approx", 0);
    Guarded<uint64_t> src(nq, 8);
    Guarded<uint32_t> vlen(nq, 4);
    Guarded<uint8_t> status(nq, (uint32_t)c.num("mis", 3));
    Guarded<unsigned long long> report(GW_WORDS, 8);
    memset(report.view(), 0, 8 * GW_WORDS);
    GetArgs a{};
    a.keys = keys.bytes.p;
    a.off = keys.var ? keys.off.p : nullptr;
    a.blob_bytes = keys.bytes.n;
    a.nq = nq;
    a.key_len = key_len;
    a.src = src.view();
    a.vlen = vlen.view();
    a.status = status.view();
    a.out = report.view();
    if (nq) {  // get_locate_launch
        const uint32_t grid = (uint32_t)c.num("grid", 1);
        if (a.off)
            hostwave::launch(grid, 256, k_get_locate<2>, mph.view(), db, a);
        else if (a.key_len == 13)
            hostwave::launch(grid, 256, k_get_locate<0>, mph.view(), db, a);
        else
            hostwave::launch(grid, 256, k_get_locate<1>, mph.view(), db, a);
    }
    printf("{");
    put_list("src", src.view(), nq);
    put_list("vlen", vlen.view(), nq);
    put_list("status", status.view(), nq);
    put_list("report", report.view(), GW_WORDS);
    printf("\"intact\":%d}\n", (int)(src.intact() && vlen.intact() && status.intact() && report.intact()));
    return 0;
}

int run_verify(const Case &c) {
    const HostMph mph(c);
    const Keys keys(c);
    const Exact<uint64_t> addr(c.list<uint64_t>("addr")), value8(c.list<uint64_t>("value8")), index(c.list<uint64_t>("index")),
        index_a(c.list<uint64_t>("index_a"));
    const Exact<uint8_t> vlen(c.list<uint8_t>("vlen"));
    const uint64_t count = c.num("count", 0);
    const uint32_t key_len = (uint32_t)c.num("key_len", 0), grid = (uint32_t)c.num("grid", 1);
    const bool approx = c.has("index_a");
    if (keys.var ? keys.off.n != count + 1 : keys.bytes.n != count * key_len) return 2;
    if ((c.has("addr") && addr.n != count) || (approx && (value8.n != count || vlen.n != count))) return 2;
    Guarded<unsigned long long> report(VERIFY_WORDS, 8);
    memset(report.view(), 0, 8 * VERIFY_WORDS);
    report.view()[VW_MIN_BAD] = ~0ULL;
    hostwave::launch((uint32_t)c.num("sgrid", 1), 256, k_verify_structure, (const uint64_t *)mph.E.p, mph.m, mph.n, report.view());
    VerifyArgs a{};
    a.keys = keys.bytes.p;
    a.off = keys.var ? keys.off.p : nullptr;
    a.blob_bytes = keys.bytes.n;
    a.n = count;
    a.key_len = key_len;
    a.addr = c.has("addr") ? addr.p : nullptr;
    a.addr_base = c.num("addr_base", 0);
    a.addr_stride = c.num("addr_stride", 0);
    a.first = c.num("first", 0);
    a.value8 = approx ? value8.p : nullptr;
    a.vlen = approx ? vlen.p : nullptr;
    a.start = c.num("start", 0);
    a.len = c.num("len", 0);
    a.index = index.p;
    a.index_a = approx ? index_a.p : nullptr;
    a.out = report.view();
    if (count) {  // verify_launch
        if (a.off)
            hostwave::launch(grid, 256, k_verify_var, mph.view(), a);
        else if (a.key_len == 13)
            hostwave::launch(grid, 256, k_verify_fixed<true>, mph.view(), a);
        else
            hostwave::launch(grid, 256, k_verify_fixed<false>, mph.view(), a);
    }
    printf("{");
    put_list("report", report.view(), VERIFY_WORDS);
    printf("\"intact\":%d}\n", (int)report.intact());
    return 0;
}

int run_case(const Case &c) {
    const std::string mode = c.str("mode");
    if (mode == "structure") return run_structure(c);
    if (mode == "lookup") return run_lookup(c);
    if (mode == "sign") return run_sign(c);
    if (mode == "scatter") return run_scatter(c);
    if (mode == "count") return run_count(c);
    if (mode == "decode") return run_decode(c);
    if (mode == "locate") return run_locate(c);
    if (mode == "verify") return run_verify(c);
    return 2;
}

}  // namespace

int main() { return run_lines(run_case); }
