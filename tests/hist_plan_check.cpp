// hist_plan_check.cpp -- prints the histogram's launch plans (hist_plan.hpp)
// as JSON lines for the cases on stdin, one case per line of name=value
// tokens (HistIn's fields; unnamed ones keep their defaults).  Each line
// carries the plan, sums over all its launches (the launches are enumerated,
// not derived; skipped past `enum_max` launches), and the launches themselves
// when there are at most `detail` of them.  Built and run by tests/test_hist_plan_cpu.py; no GPU, no HIP.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../bsdb_amd/csrc/hist_plan.hpp"

using namespace bsdb;

static const char *kind_name(P1Kind k) {
    return k == P1Kind::D13 ? "d13" : k == P1Kind::D13E ? "d13e" : k == P1Kind::VARE ? "vare" : "none";
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        HistIn in;
        uint64_t detail = 0, enum_max = UINT64_MAX;
        std::istringstream ss(line);
        std::string tok;
        while (ss >> tok) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) return 2;
            const std::string k = tok.substr(0, eq);
            const long long sv = strtoll(tok.c_str() + eq + 1, nullptr, 10);
            const uint64_t v = strtoull(tok.c_str() + eq + 1, nullptr, 10);
            if (k == "var") in.var = v;
            else if (k == "key_len") in.key_len = (uint32_t)v;
            else if (k == "n") in.n = v;
            else if (k == "m") in.m = v;
            else if (k == "blob_bytes") in.blob_bytes = v;
            else if (k == "seed0") in.seed0 = v;
            else if (k == "hist_mode") in.hist_mode = (int)sv;
            else if (k == "frontend") in.frontend = (int)sv;
            else if (k == "d13_variant") in.d13_variant = (int)sv;
            else if (k == "d13_copies") in.d13_copies = (int)sv;
            else if (k == "chunk_keys") in.chunk_keys = v;
            else if (k == "span_max") in.span_max = v;
            else if (k == "pipe") in.pipe = v;
            else if (k == "pipe_chunks") in.pipe_chunks = v;
            else if (k == "pipe_cus") in.pipe_cus = (uint32_t)v;
            else if (k == "no_fixed_window") in.no_fixed_window = v;
            else if (k == "no_seed0") in.no_seed0 = v;
            else if (k == "d13_grid") in.d13_grid = sv;
            else if (k == "num_cus") in.num_cus = (int)sv;
            else if (k == "wg_per_cu") in.wg_per_cu = (int)sv;
            else if (k == "free_bytes") in.free_bytes = v;
            else if (k == "ids_bytes") in.ids_bytes = v;
            else if (k == "detail") detail = v;
            else if (k == "enum_max") enum_max = v;
            else return 2;
        }
        HistPlan p = pass1_select(in);
        hist_size(in, p);
        printf("{\"atomic\":%d,\"kind\":\"%s\",\"k_key_len\":%u,\"k_seed0\":%d,\"variant\":%d,\"nt\":%d,\"tile\":%" PRIu64
               ",\"binned\":%d,\"windowed\":%d,\"nparts\":%u,\"bin_shift\":%u,\"capb\":%u",
               p.atomic_mode, kind_name(p.k.kind), p.k.key_len, p.k.seed0, p.k.variant, p.k.nt(), p.k.tile(),
               p.k.binned(), p.k.windowed(), p.nparts, p.bin_shift, p.capb);
        if (p.atomic_mode) {
            printf("}\n");
            continue;
        }
        printf(",\"nmain\":%u,\"ntail\":%u,\"grid_d13\":%u,\"cap\":%" PRIu64 ",\"cap_tail\":%" PRIu64 ",\"keys_per_copy\":%" PRIu64
               ",\"launch\":%" PRIu64 ",\"per_span\":%" PRIu64 ",\"pipe\":%d,\"nbuf\":%u,\"p2_cus\":%u,\"bottomed_out\":%d",
               p.nmain, p.ntail, p.grid_d13, p.cap, p.cap_tail, p.keys_per_copy, p.launch, p.per_span, p.pipe, p.nbuf,
               p.p2_cus, p.bottomed_out);
        printf(",\"set_elems\":%zu,\"tail_elems\":%zu,\"ids_per_buf\":%zu,\"cur_per_buf\":%zu,\"ids_bytes\":%zu,\"cursor_bytes\":%zu,"
               "\"prefix_bytes\":%zu,\"spans\":%" PRIu64,
               p.set_elems(), p.tail_elems(), p.ids_per_buf(), p.cur_per_buf(), p.ids_bytes(), p.cursor_bytes(),
               p.prefix_bytes(), p.spans());
        if ((in.n + p.launch - 1) / p.launch > enum_max) {  // (too many launches to walk: the plan alone)
            printf("}\n");
            continue;
        }
        // every launch of the call, in order
        const uint64_t tile = p.k.kind == P1Kind::NONE ? (uint64_t)P1_TILE : p.k.tile();
        const uint64_t over = p.k.windowed() ? 16 - in.key_len : 0;
        uint64_t next = 0, launches = 0, tails = 0, tail_only = 0, nonlast_tails = 0, max_span_launches = 0;
        uint64_t bad_cover = 0, bad_split = 0, bad_blob = 0, bad_window = 0, bad_grid = 0, bad_pipe_grid = 0, bad_buf = 0;
        uint64_t max_copy_keys = 0, max_copy_tiles = 0;
        std::vector<uint64_t> copy_keys(p.nmain), copy_tiles(p.nmain);
        std::string spans_js, launches_js;
        char buf[512];
        const uint64_t nspans = p.spans();
        for (uint64_t i = 0; i < nspans; ++i) {
            const HistSpan sp = p.span(i);
            if (sp.r.k0 != next) ++bad_cover;
            if (sp.buf >= p.nbuf) ++bad_buf;
            max_span_launches = std::max(max_span_launches, sp.launches);
            std::fill(copy_keys.begin(), copy_keys.end(), 0);
            std::fill(copy_tiles.begin(), copy_tiles.end(), 0);
            if (nspans <= detail) {
                snprintf(buf, sizeof buf, "%s[%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%u,%u]", spans_js.empty() ? "" : ",",
                         sp.r.k0, sp.r.nk, sp.r.blob, sp.launches, sp.buf, sp.p2_grid);
                spans_js += buf;
            }
            for (uint64_t j = 0; j < sp.launches; ++j, ++launches) {
                const HistLaunch l = p.launch_of(sp, j);
                if (l.r.k0 != next || l.r.nk == 0) ++bad_cover;
                next = l.r.k0 + l.r.nk;
                const bool has_kernel = p.k.kind != P1Kind::NONE;
                const uint64_t fast = has_kernel ? l.tiles * tile : l.r.nk;
                if (l.tail.nk) {
                    ++tails;
                    if (!l.tiles) ++tail_only;
                    if (j + 1 != sp.launches) ++nonlast_tails;
                    if (!has_kernel || l.tail.k0 != l.r.k0 + fast || l.tail.k0 + l.tail.nk != next) ++bad_split;
                    if (l.tail_tiles != p1_tiles(l.tail.nk)) ++bad_split;
                    if (!in.var && l.tail.blob > in.blob_bytes - l.tail.k0 * in.key_len) ++bad_blob;
                } else if (fast != l.r.nk || (!has_kernel && l.tiles != p1_tiles(l.r.nk))) {
                    ++bad_split;
                }
                if (!in.var && (l.r.blob > in.blob_bytes - l.r.k0 * in.key_len || l.r.blob < l.r.nk * in.key_len)) ++bad_blob;
                if (has_kernel && p.k.windowed() && l.tiles && l.tiles * tile * in.key_len + over > l.r.blob) ++bad_window;
                if (has_kernel && l.tiles && (l.grid < 1 || l.grid > l.tiles)) ++bad_grid;
                if (p.pipe && l.r.k0 != 0 && l.tiles && l.grid > (uint32_t)in.num_cus - p.p2_cus) ++bad_pipe_grid;
                // the launch's tiles dealt round-robin over the copies, from copy 0 on
                const uint64_t T = (l.r.nk + tile - 1) / tile;
                for (uint32_t cidx = 0; cidx < p.nmain; ++cidx) {
                    const uint64_t t = T > cidx ? (T - cidx + p.nmain - 1) / p.nmain : 0;
                    copy_tiles[cidx] += t;
                    copy_keys[cidx] += t * tile - (t && (T - 1) % p.nmain == cidx ? T * tile - l.r.nk : 0);
                }
                if (launches < detail) {
                    snprintf(buf, sizeof buf,
                             "%s[%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%u,%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%" PRIu64 "]",
                             launches_js.empty() ? "" : ",", i, l.r.k0, l.r.nk, l.r.blob, l.grid, l.tiles, l.tail.k0, l.tail.nk,
                             l.tail.blob, l.tail_tiles);
                    launches_js += buf;
                }
            }
            if (next != sp.r.k0 + sp.r.nk) ++bad_cover;
            for (uint32_t cidx = 0; cidx < p.nmain; ++cidx) {
                max_copy_keys = std::max(max_copy_keys, copy_keys[cidx]);
                max_copy_tiles = std::max(max_copy_tiles, copy_tiles[cidx]);
            }
        }
        if (next != in.n) ++bad_cover;
        printf(",\"launches\":%" PRIu64 ",\"tails\":%" PRIu64 ",\"tail_only\":%" PRIu64 ",\"nonlast_tails\":%" PRIu64
               ",\"max_span_launches\":%" PRIu64 ",\"max_copy_keys\":%" PRIu64 ",\"max_copy_tiles\":%" PRIu64,
               launches, tails, tail_only, nonlast_tails, max_span_launches, max_copy_keys, max_copy_tiles);
        printf(",\"bad_cover\":%" PRIu64 ",\"bad_split\":%" PRIu64 ",\"bad_blob\":%" PRIu64 ",\"bad_window\":%" PRIu64
               ",\"bad_grid\":%" PRIu64 ",\"bad_pipe_grid\":%" PRIu64 ",\"bad_buf\":%" PRIu64,
               bad_cover, bad_split, bad_blob, bad_window, bad_grid, bad_pipe_grid, bad_buf);
        if (launches <= detail) printf(",\"span_list\":[%s],\"launch_list\":[%s]", spans_js.c_str(), launches_js.c_str());
        printf("}\n");
    }
    return 0;
}
