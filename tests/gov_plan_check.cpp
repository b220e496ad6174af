// gov_plan_check.cpp -- prints the GOV build's plans (gov_plan.hpp) as JSON
// lines for the cases on stdin, one case per line of name=value tokens.  A
// line that starts with "parse" runs the knob parsers instead: spec=STR,
// fvs=STR, percu=STR (a name left out: the variable is unset; "spec=" is the
// empty string), exact=1, one=1.  Every other line is a build: the group
// plan, the solve plan for n_local keys, the big plan for the status words
// st1 / st3.  Built and run by tests/test_gov_plan_cpu.py; no GPU, no HIP.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "../bsdb_amd/csrc/gov_plan.hpp"

using namespace bsdb;

static const char *class_name(GovClass c) {
    switch (c) {
        case GovClass::COPY_COUNTS: return "copy_counts";
        case GovClass::SEL: return "sel";
        case GovClass::SMALL: return "small";
        case GovClass::MID: return "mid";
        case GovClass::LARGE: return "large";
        default: return "none";
    }
}

static void J(const char *k, unsigned long long v, const char *end = ",") { printf("\"%s\":%llu%s", k, v, end); }

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream ss(line);
        std::string tok;
        if (line.compare(0, 5, "parse") == 0) {
            std::string spec, fvs, percu;
            bool has_spec = false, has_fvs = false, has_percu = false, exact = false, one = false;
            ss >> tok;
            while (ss >> tok) {
                const size_t eq = tok.find('=');
                if (eq == std::string::npos) return 2;
                const std::string k = tok.substr(0, eq), v = tok.substr(eq + 1);
                if (k == "spec") spec = v, has_spec = true;
                else if (k == "fvs") fvs = v, has_fvs = true;
                else if (k == "percu") percu = v, has_percu = true;
                else if (k == "exact") exact = v == "1";
                else if (k == "one") one = v == "1";
                else return 2;
            }
            printf("{");
            J("spec", gov_parse_spec(has_spec ? spec.c_str() : nullptr));
            J("fvs_max", gov_parse_fvs_max(has_fvs ? fvs.c_str() : nullptr, exact));
            J("per_cu", (unsigned)gov_parse_per_cu(one, has_percu ? percu.c_str() : nullptr), "}\n");
            continue;
        }
        GovGroupIn in;
        GovKnobs kn;
        GovSizes sz;
        uint64_t n_local = 0, want_pos = 0, width = 0, st1 = 0, st3 = 0;
        bool has_n_local = false;
        while (ss >> tok) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) return 2;
            const std::string k = tok.substr(0, eq);
            const uint64_t v = strtoull(tok.c_str() + eq + 1, nullptr, 10);
            if (k == "n_src") in.n_src = v;
            else if (k == "from_keys") in.from_keys = v;
            else if (k == "counts_all") in.counts_all = v;
            else if (k == "b_lo") in.b_lo = v;
            else if (k == "b_hi") in.b_hi = v;
            else if (k == "n_global") in.n_global = v;
            else if (k == "num_cus") in.num_cus = (int)v;
            else if (k == "n_local") n_local = v, has_n_local = true;
            else if (k == "want_pos") want_pos = v;
            else if (k == "width") width = v;
            else if (k == "per_cu") kn.per_cu = (int)v;
            else if (k == "lds") sz.solve_lds = v;
            else if (k == "scratch_words") sz.scratch_words = v;
            else if (k == "mid_scratch_words") sz.mid_scratch_words = v;
            else if (k == "big_slab") sz.big_slab_bytes = v;
            else if (k == "st1") st1 = v;
            else if (k == "st3") st3 = v;
            else return 2;
        }
        if (!has_n_local) n_local = in.n_src;
        const GovGroupPlan g = gov_group_plan(in);
        const GovSolvePlan s = gov_solve_plan(g, n_local, want_pos != 0, (uint32_t)width, kn, sz);
        const GovBigPlan b = gov_big_plan((uint32_t)st1, (uint32_t)st3, s.big_cap, in.num_cus, sz);
        printf("{\"cls\":\"%s\",", class_name(g.cls));
        J("m", g.m), J("nb", g.nb), J("mult", g.mult), J("mid_g", g.mid_g), J("cw_bytes", g.cw_bytes);
        J("mid_bytes", g.mid_bytes), J("count_grid", g.count_grid), J("col_grid", g.col_grid), J("base_grid", g.base_grid);
        J("counts_bytes", g.counts_bytes), J("cursor_bytes", g.cursor_bytes), J("status_bytes", g.status_bytes);
        J("values_bytes", g.values_bytes);
        J("sorted_bytes", s.sorted_bytes), J("need_pay", s.need_pay), J("pay_bytes", s.pay_bytes), J("big_cap", s.big_cap);
        J("big_bytes", s.big_bytes), J("per_cu", (unsigned)s.per_cu), J("lds_pad", s.lds_pad), J("solve_grid", s.solve_grid);
        J("scratch_bytes", s.scratch_bytes), J("cursor_grid", s.cursor_grid), J("scatter_grid", s.scatter_grid);
        J("sort_grid", s.sort_grid), J("list_grid", s.list_grid), J("verify_grid", s.verify_grid);
        J("led_fail", s.led.fail), J("led_claim", s.led.claim), J("led_won", s.led.won), J("led_done", s.led.done);
        J("led_active", s.led.active), J("led_zero", s.led.zero_bytes), J("led_ones", s.led.ones_bytes), J("led_bytes", s.led.bytes);
        J("sigbits_bytes", s.sigbits_bytes);
        J("nbig", b.nbig), J("nhuge", b.nhuge), J("big_sort_grid", b.sort_grid), J("mid_grid", b.mid_grid);
        J("big_grid", b.big_grid), J("slabs_bytes", b.slabs_bytes), J("midscr_bytes", b.midscr_bytes, "}\n");
    }
    return 0;
}
