// gov_plan.hpp -- what a GOV build allocates and launches, decided on the host
// from plain numbers, in the three steps the build's two host synchronisations
// leave: the grouping of a range's keys by bucket (gov_group_plan), the solve
// once the range's key count is known (gov_solve_plan), and the oversized
// buckets once the device has listed them (gov_big_plan).  capi_gov.hip fills
// the inputs from the call, the context and the environment (gov_knobs) and
// enqueues what the plans say.  Host-only C++17: no HIP, no getenv, no kernel
// type (the sizes of the device structs come in as GovSizes), so the
// arithmetic runs (and is checked, tests/gov_plan_check.cpp) without a GPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "gov_geometry.hpp"

namespace bsdb {

// The environment's knobs of a build, read once per call by gov_knobs().
struct GovKnobs {
    int per_cu = GS_PER_CU;         // solver workgroups per CU (measurement only: fewer than GS_PER_CU)
    uint32_t fvs_max = FVS_NH_MAX;  // SolveArgs::fvs_max; bit 31: the exact-rounds FVS picks (a test aid)
    uint32_t spec = 2;              // SolveArgs::spec
    bool profile = false;           // BSDB_GOV_PROFILE: k_gov_solve<true>, phase totals on stderr
};

// SolveArgs::spec from BSDB_GOV_SPEC = "K[,P]": at most K seeds of a bucket in
// flight before a speculating workgroup adds one (0: no limit), P = 1: the
// speculative attempts at a lower wave priority.  Default K = 2: at C1 (667
// buckets on 512 workgroups) the solve takes 5.1 ms against 6.4 ms with no
// limit (every extra seed in flight shares a CU with the attempt that decides
// its bucket); the priority did not help (6.6 ms).
inline uint32_t gov_parse_spec(const char *v) {
    if (!v) return 2;
    uint32_t spec = (uint32_t)std::max(0, std::min(atoi(v), 255));
    if (const char *c = strchr(v, ','); c && atoi(c + 1)) spec |= 0x100u;
    return spec;
}
// BSDB_GOV_FVS_MAX (unset: FVS_NH_MAX) and BSDB_GOV_PICK_EXACT
inline uint32_t gov_parse_fvs_max(const char *v, bool pick_exact) {
    const uint32_t lim = v ? (uint32_t)std::max(2, std::min(atoi(v), (int)FVS_NH_MAX)) : FVS_NH_MAX;
    return pick_exact ? lim | 0x80000000u : lim;
}
// BSDB_GOV_ONE_PER_CU=1 / BSDB_GOV_PER_CU=k (measurement only): k < GS_PER_CU
// solver workgroups per CU (grid and LDS padding), to price the others
inline int gov_parse_per_cu(bool one_per_cu, const char *v) {
    return v ? std::max(1, std::min(GS_PER_CU, atoi(v))) : one_per_cu ? 1 : GS_PER_CU;
}

// What the plans need of the device structs (gov_kernels.hip).
struct GovSizes {
    size_t solve_lds = 0;          // sizeof(SolveLds)
    size_t scratch_words = 0;      // solve_scratch_words<SolveLds>()
    size_t mid_scratch_words = 0;  // solve_scratch_words<SolveMid>()
    size_t big_slab_bytes = 0;     // big_slab_bytes()
};

inline uint64_t gov_values_words(uint64_t n) { return (2 * (1 + ((n * 281) >> 8)) + 63) / 64; }

// workgroups of a 256-thread grid-stride kernel over n elements
inline uint32_t grid_for(int num_cus, uint64_t n) {
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, (uint64_t)num_cus * 16));
}

// How a range's keys are counted per bucket and scattered to their buckets:
// the two steps always take the same class.
enum class GovClass {
    NONE,         // no key: nothing to count or scatter
    COPY_COUNTS,  // keys, every bucket's count known: copied; scatter by k_sel<1>
    SEL,          // keys re-hashed and filtered to the range: k_sel<0>, k_sel<1>
    SMALL,        // signatures, nb <= SMALL_NB: LDS counters per chunk of SMALL_CHUNK keys
    MID,          // signatures, nb <= MID_NB, n < 2^32: per-workgroup 16-bit counts and bases, no per-key global atomics
    LARGE,        // signatures, any range: per-key global atomics (k_bucket_count, k_bucket_scatter)
};

// workgroups of a class's counting or scatter kernel over n keys (0: nothing to launch)
inline uint32_t gov_class_grid(GovClass cls, int num_cus, uint64_t n, uint32_t mid_g) {
    switch (cls) {
        case GovClass::NONE: return 0;
        case GovClass::SMALL: return (uint32_t)((n + SMALL_CHUNK - 1) / SMALL_CHUNK);
        case GovClass::MID: return mid_g;
        default: return n ? grid_for(num_cus, n) : 0;  // k_sel, k_bucket_count, k_bucket_scatter
    }
}

struct GovGroupIn {
    uint64_t n_src = 0;       // signatures of the range, or keys of the whole set
    bool from_keys = false;
    bool counts_all = false;  // (key sources) every bucket's count is given
    uint64_t b_lo = 0, b_hi = 0, n_global = 0;
    int num_cus = 256;
};

struct GovGroupPlan {
    GovClass cls = GovClass::NONE;
    GovGroupIn in;
    uint64_t m = 0, nb = 0;
    uint32_t mult = 0;  // 2 m
    // MID: the workgroups, and g_mid = [mid_g][nb] u16 counts (cw_bytes, rounded to 256), then [mid_g][nb] u32 bases
    uint32_t mid_g = 1;
    size_t cw_bytes = 0, mid_bytes = 0;
    uint32_t count_grid = 0;  // the class's counting kernel (COPY_COUNTS: a copy, no kernel)
    uint32_t col_grid = 0;    // k_mid_colsum, k_mid_colscan: a thread per bucket
    uint32_t base_grid = 0;   // k_add_base over Eb[0..nb]
    size_t counts_bytes = 0, cursor_bytes = 0, status_bytes = 16;  // g_counts (+1: k_bucket_count_mid's flag), g_cursor, g_status
    size_t values_bytes = 0;  // d_values of the whole structure (a full build zeroes it before anything else)
};

inline GovGroupPlan gov_group_plan(const GovGroupIn &in) {
    GovGroupPlan p;
    const uint64_t n = in.n_src, nb = in.b_hi - in.b_lo;
    p.in = in;
    p.m = in.n_global / BUCKET_SIZE + 1;
    p.nb = nb;
    p.mult = (uint32_t)(2 * p.m);
    p.mid_g = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)in.num_cus, n / 65536));
    if (in.from_keys)
        p.cls = in.counts_all ? GovClass::COPY_COUNTS : n ? GovClass::SEL : GovClass::NONE;
    else if (!n)
        p.cls = GovClass::NONE;
    else if (nb <= SMALL_NB)
        p.cls = GovClass::SMALL;
    else if (nb <= MID_NB && n < (1ULL << 32))
        p.cls = GovClass::MID;
    else
        p.cls = GovClass::LARGE;
    if (p.cls == GovClass::MID) {
        p.cw_bytes = ((size_t)p.mid_g * nb * 2 + 255) & ~(size_t)255;
        p.mid_bytes = p.cw_bytes + (size_t)p.mid_g * nb * 4;
    }
    p.count_grid = p.cls == GovClass::COPY_COUNTS ? 0 : gov_class_grid(p.cls, in.num_cus, n, p.mid_g);
    p.col_grid = (uint32_t)((nb + 255) / 256);
    p.base_grid = grid_for(in.num_cus, nb + 1);
    p.counts_bytes = (size_t)(nb + 1) * 4;
    p.cursor_bytes = (size_t)std::max<uint64_t>(nb, 1) * 8;
    p.values_bytes = (size_t)gov_values_words(in.n_global) * 8;
    return p;
}

// The solver's seed ledger (SeedLedger) in one buffer: fail (4 u64 per
// bucket), claim, won, done (u32 per bucket), zeroed; active (u32 per solver
// workgroup), all ones.  Byte offsets.
struct GovLedger {
    size_t fail = 0, claim = 0, won = 0, done = 0, active = 0;
    size_t zero_bytes = 0;  // from 0: fail .. done
    size_t ones_bytes = 0;  // from active
    size_t bytes = 0;
};

struct GovSolvePlan {
    size_t sorted_bytes = 0;  // g_sorted: the range's signatures
    bool need_pay = false;    // g_pay: the input position of each sorted signature
    size_t pay_bytes = 0;
    uint32_t big_cap = 0;     // g_big: entries of the oversized buckets' list
    size_t big_bytes = 0;
    int per_cu = GS_PER_CU;
    size_t lds_pad = 0;       // dynamic LDS that keeps a CU to per_cu solver workgroups
    uint32_t solve_grid = 0;
    size_t scratch_bytes = 0;  // g_scratch
    uint32_t cursor_grid = 0, scatter_grid = 0, sort_grid = 0, list_grid = 0, verify_grid = 0;
    GovLedger led;
    size_t sigbits_bytes = 0;  // d_sigbits of the whole structure (0: no checksum bits)
};

inline GovSolvePlan gov_solve_plan(const GovGroupPlan &g, uint64_t n_local, bool want_positions, uint32_t width,
                                   const GovKnobs &k, const GovSizes &sz) {
    GovSolvePlan p;
    const uint64_t nb = g.nb;
    const int num_cus = g.in.num_cus;
    p.sorted_bytes = (size_t)std::max<uint64_t>(n_local, 1) * 16;
    p.need_pay = want_positions || g.in.from_keys;  // (a key source always records positions)
    p.pay_bytes = (size_t)std::max<uint64_t>(n_local, 1) * 8;
    p.big_cap = (uint32_t)(n_local / (GS_CMAX + 1) + 1);
    p.big_bytes = (size_t)p.big_cap * 4;
    p.per_cu = k.per_cu;
    if (k.per_cu < GS_PER_CU) {
        // the LDS of a workgroup, padded past 1 / (per_cu + 1) of the CU's
        const size_t share = CU_LDS_BYTES / (size_t)(k.per_cu + 1) + 1024;
        p.lds_pad = share > sz.solve_lds ? (share - sz.solve_lds) & ~(size_t)1023 : 0;
    }
    p.solve_grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(nb, (uint64_t)num_cus * k.per_cu));
    p.scratch_bytes = (size_t)p.solve_grid * sz.scratch_words * 8;
    p.cursor_grid = grid_for(num_cus, nb);
    // (k_sel<1> runs over every key of the source, the signature kernels over the range's)
    p.scatter_grid = gov_class_grid(g.cls, num_cus, g.in.from_keys ? g.in.n_src : n_local, g.mid_g);
    p.sort_grid = (uint32_t)std::min<uint64_t>(nb, (uint64_t)num_cus * 8);
    p.list_grid = grid_for(num_cus, nb);
    p.verify_grid = grid_for(num_cus, n_local);
    p.led.fail = 0;
    p.led.claim = (size_t)nb * 32;
    p.led.won = p.led.claim + (size_t)nb * 4;
    p.led.done = p.led.won + (size_t)nb * 4;
    p.led.active = p.led.done + (size_t)nb * 4;
    p.led.zero_bytes = p.led.active;
    p.led.ones_bytes = (size_t)p.solve_grid * 4;
    p.led.bytes = p.led.zero_bytes + p.led.ones_bytes + 64;
    p.sigbits_bytes = width ? (size_t)((g.in.n_global * width + 63) / 64 + 1) * 8 : 0;
    return p;
}

// Oversized buckets, from the device's status words: st3 of them listed, st1
// of those over GM_CMAX keys.  Those up to GM_CMAX keys (all of a random set)
// are solved in LDS, one workgroup per CU (k_gov_solve_mid); larger ones in
// global slabs (k_gov_solve_big, 8 workgroups).
struct GovBigPlan {
    uint32_t nbig = 0, nhuge = 0;
    uint32_t sort_grid = 0, mid_grid = 0, big_grid = 0;
    size_t slabs_bytes = 0;   // g_slabs: per-workgroup slabs for the sort, then the global-slab solver's state
    size_t midscr_bytes = 0;  // g_midscr
};

inline GovBigPlan gov_big_plan(uint32_t st1, uint32_t st3, uint32_t big_cap, int num_cus, const GovSizes &sz) {
    GovBigPlan p;
    p.nbig = std::min(st3, big_cap);
    p.nhuge = std::min(st1, p.nbig);
    p.sort_grid = std::min<uint32_t>(p.nbig, (uint32_t)num_cus);
    p.mid_grid = std::min<uint32_t>(p.nbig - p.nhuge, (uint32_t)num_cus);
    p.big_grid = std::min<uint32_t>(p.nhuge, 8);
    if (p.nbig) {
        const size_t sort_bytes = (size_t)p.sort_grid * GB_CMAX * (16 + 8);  // signatures + payloads
        p.slabs_bytes = std::max(sort_bytes, (size_t)p.big_grid * sz.big_slab_bytes);
        p.midscr_bytes = (size_t)p.mid_grid * sz.mid_scratch_words * 8;
    }
    return p;
}

}  // namespace bsdb
