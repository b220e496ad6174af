"""The GOV build's plans (bsdb_amd/csrc/gov_plan.hpp) without a GPU:
tests/gov_plan_check.cpp is built with the system C++ compiler under
ASan + UBSan and run as a program of its own; it prints one JSON line per case
(group plan, solve plan, big plan) or per set of knob strings.  Asserted here:
the invariants every plan must keep, over a grid of ranges, key counts, devices,
knobs and struct sizes, the knob parsers' values, and the plans of C1, C2 and a
C4 pass as the build computed them before the plan existed."""
import itertools
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "gov_plan_check.cpp")

GS_PER_CU, GS_CMAX, GB_CMAX = 2, 1664, 16384
SMALL_NB, SMALL_CHUNK, MID_NB, FVS_NH_MAX = 4096, 4096, 80_000, 380
CU_LDS = 160 * 1024
# the device structs of the library as built (gfx950): sizeof(SolveLds), solve_scratch_words<SolveLds>(),
# solve_scratch_words<SolveMid>(), big_slab_bytes().  After a change of SolveLdsT (gov_kernels.hip) refresh them: a
# host program that includes the kernel files as bsdb_capi.hip does and prints the four expressions, or the
# "LDS ... B each" figure of a BSDB_GOV_PROFILE=1 run for the first; the pinned plans below follow from them.
REAL = dict(lds=81_432, scratch_words=89_856, mid_scratch_words=135_168, big_slab=68_170_240)
U32 = 1 << 32


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler on this machine")
    exe = str(tmp_path_factory.mktemp("gov_plan") / "gov_plan_check")
    # The sanitizer runtimes are linked into the program (g++ needs the two flags, clang does so by itself and
    # does not know them), so it starts whatever else the environment preloads; the environment is passed on as it is.
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-o", exe, SRC]
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True)
    probe = subprocess.run([exe], input="", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the sanitized program does not start in this environment: " + probe.stderr.strip()[-300:])

    def run(lines):
        r = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        out = [json.loads(line) for line in r.stdout.splitlines()]
        assert len(out) == len(lines)
        return out

    def plans(cases):
        return run([" ".join(f"{k}={int(v)}" for k, v in c.items()) for c in cases])

    plans.parse = lambda sets: run(["parse " + " ".join(f"{k}={v}" for k, v in s.items()) for s in sets])
    return plans


def case(n_src, b_lo, b_hi, from_keys=0, counts_all=0, num_cus=256, per_cu=GS_PER_CU, n_local=None, **kw):
    c = dict(n_src=n_src, from_keys=from_keys, counts_all=counts_all, b_lo=b_lo, b_hi=b_hi, n_global=max(b_hi * 1500, n_src),
             num_cus=num_cus, per_cu=per_cu, want_pos=0, width=4, st1=0, st3=0, **REAL)
    if n_local is not None:
        c["n_local"] = n_local
    c.update(kw)
    return c


def grid_for(cus, n):
    return max(1, min((n + 255) // 256, cus * 16))


def expected_class(c):
    n, nb = c["n_src"], c["b_hi"] - c["b_lo"]
    if c["from_keys"]:
        return "copy_counts" if c["counts_all"] else "sel" if n else "none"
    if not n:
        return "none"
    if nb <= SMALL_NB:
        return "small"
    return "mid" if nb <= MID_NB and n < U32 else "large"


def check(c, p):
    ctx = (c, p)
    n, nb, cus, per_cu = c["n_src"], c["b_hi"] - c["b_lo"], c["num_cus"], c["per_cu"]
    n_local = c.get("n_local", n)
    cls = p["cls"]
    assert cls == expected_class(c), ctx
    assert (p["m"], p["nb"], p["mult"]) == (c["n_global"] // 1500 + 1, nb, 2 * (c["n_global"] // 1500 + 1)), ctx
    # the grouping: both steps' grids belong to the one class
    assert 1 <= p["mid_g"] <= cus and p["mid_g"] == max(1, min(cus, n // 65536)), ctx
    count = {"none": 0, "copy_counts": 0, "sel": grid_for(cus, n), "large": grid_for(cus, n),
             "small": -(-n // SMALL_CHUNK), "mid": p["mid_g"]}[cls]
    scatter = {"none": 0, "copy_counts": grid_for(cus, n) if n else 0, "sel": grid_for(cus, n),
               "large": grid_for(cus, n_local), "small": -(-n_local // SMALL_CHUNK), "mid": p["mid_g"]}[cls]
    assert (p["count_grid"], p["scatter_grid"]) == (count, scatter), ctx
    launched = [p["base_grid"], p["cursor_grid"], p["sort_grid"], p["list_grid"], p["verify_grid"], p["solve_grid"]]
    launched += [g for g in (count, scatter) if cls not in ("none", "copy_counts")]
    if cls == "mid":
        launched.append(p["col_grid"])
        # g_mid: [mid_g][nb] u16, padded, then [mid_g][nb] u32
        assert p["cw_bytes"] >= p["mid_g"] * nb * 2 and p["cw_bytes"] % 256 == 0 and p["cw_bytes"] - p["mid_g"] * nb * 2 < 256, ctx
        assert p["mid_bytes"] == p["cw_bytes"] + p["mid_g"] * nb * 4, ctx
    else:
        assert p["mid_bytes"] == 0, ctx
    assert all(1 <= g < U32 for g in launched), ctx
    assert (p["col_grid"], p["base_grid"], p["cursor_grid"], p["list_grid"], p["verify_grid"]) == (
        -(-nb // 256), grid_for(cus, nb + 1), grid_for(cus, nb), grid_for(cus, nb), grid_for(cus, n_local)), ctx
    assert p["sort_grid"] == min(nb, cus * 8), ctx
    assert (p["counts_bytes"], p["cursor_bytes"], p["status_bytes"]) == ((nb + 1) * 4, max(nb, 1) * 8, 16), ctx
    assert p["values_bytes"] == (2 * (1 + (c["n_global"] * 281 >> 8)) + 63) // 64 * 8, ctx
    assert p["sigbits_bytes"] == (((c["n_global"] * c["width"] + 63) // 64 + 1) * 8 if c["width"] else 0), ctx
    # the solve
    assert (p["sorted_bytes"], p["pay_bytes"]) == (max(n_local, 1) * 16, max(n_local, 1) * 8), ctx
    assert p["need_pay"] == int(bool(c["want_pos"] or c["from_keys"])), ctx
    assert p["big_cap"] >= n_local // (GS_CMAX + 1) + 1 and p["big_bytes"] == 4 * p["big_cap"], ctx
    assert p["solve_grid"] == max(1, min(nb, cus * per_cu)) and p["per_cu"] == per_cu, ctx
    assert p["scratch_bytes"] == p["solve_grid"] * c["scratch_words"] * 8, ctx
    assert p["lds_pad"] % 1024 == 0 and p["lds_pad"] < CU_LDS, ctx  # (no wrap)
    if per_cu >= GS_PER_CU:
        assert p["lds_pad"] == 0, ctx
    elif c["lds"] <= CU_LDS:  # per_cu workgroups fit a CU and one more does not, whatever the struct's size
        u = c["lds"] + p["lds_pad"]
        assert per_cu * u <= CU_LDS < (per_cu + 1) * u, ctx
    else:
        assert p["lds_pad"] == 0, ctx
    # the ledger: fail, claim, won, done, active in this order, disjoint, inside the buffer
    arrays = [("led_fail", nb * 32, 8), ("led_claim", nb * 4, 4), ("led_won", nb * 4, 4), ("led_done", nb * 4, 4),
              ("led_active", p["solve_grid"] * 4, 4)]
    end = 0
    for name, size, align in arrays:
        assert p[name] >= end and p[name] % align == 0, (name, ctx)
        end = p[name] + size
    assert end <= p["led_bytes"], ctx
    assert p["led_fail"] == 0 and p["led_zero"] == p["led_active"] == nb * 44 and p["led_ones"] == p["solve_grid"] * 4, ctx
    # the oversized buckets
    assert p["nhuge"] <= p["nbig"] <= p["big_cap"], ctx
    assert (p["nbig"], p["nhuge"]) == (min(c["st3"], p["big_cap"]), min(c["st1"], c["st3"], p["big_cap"])), ctx
    assert p["big_sort_grid"] == min(p["nbig"], cus) and p["mid_grid"] == min(p["nbig"] - p["nhuge"], cus), ctx
    assert p["big_grid"] == min(p["nhuge"], 8), ctx
    if p["nbig"]:
        assert p["slabs_bytes"] >= p["big_sort_grid"] * GB_CMAX * 24 and p["slabs_bytes"] >= p["big_grid"] * c["big_slab"], ctx
        assert p["midscr_bytes"] == p["mid_grid"] * c["mid_scratch_words"] * 8, ctx
    else:
        assert p["slabs_bytes"] == p["midscr_bytes"] == 0, ctx


NBS = (1, 2, 667, SMALL_NB, SMALL_NB + 1, 66_667, MID_NB, MID_NB + 1, 8_795_859)
NS = (0, 1, 4095, 4096, 4097, 65_535, 65_536, 1_000_000, U32 - 1, U32, 13_193_787_549)
SOURCES = ((0, 0), (1, 0), (1, 1))  # signatures, keys, keys with every bucket's count
STATUS = ((0, 0), (0, 1), (1, 1), (3, 9), (9, 3), (0, 300), (40, 300), (1, U32 - 1))


def grid_cases():
    out = []
    for nb, n, (fk, ca), cus, per_cu in itertools.product(NBS, NS, SOURCES, (1, 8, 256, 304), (1, 2)):
        for b_lo in (0, 500):
            out.append(case(n, b_lo, b_lo + nb, fk, ca, cus, per_cu, want_pos=(nb + n) & 1, width=(0, 4, 64)[(nb + n) % 3]))
    # a key source finds its own key count
    for nb, n, n_local in itertools.product(NBS, NS[1:], (0, 1, 1664, 1665, 3_000_000)):
        out.append(case(n, 7, 7 + nb, 1, n & 1, n_local=min(n, n_local)))
    # struct sizes on both sides of the LDS shares, the oversized buckets' counts
    sizes = [dict(lds=l, scratch_words=s, mid_scratch_words=2 * s, big_slab=b)
             for l, (s, b) in itertools.product((0, 1000, 81_432, 81_856, 81_857, 81_920, 82_943, 82_944, 82_945, 163_840, 200_000),
                                                ((1, 256), (89_856, 68_170_240)))]
    for sz, (st1, st3), n, cus, per_cu in itertools.product(sizes, STATUS, (1, 1_000_000, U32), (1, 256), (1, 2)):
        out.append(case(n, 0, 70_000, num_cus=cus, per_cu=per_cu, st1=st1, st3=st3, **sz))
    return out


def test_invariants_over_the_grid(planner):
    cases = grid_cases()
    plans = planner(cases)
    for c, p in zip(cases, plans):
        check(c, p)
    assert {p["cls"] for p in plans} == {"none", "copy_counts", "sel", "small", "mid", "large"}
    assert any(p["lds_pad"] for p in plans) and any(p["nhuge"] for p in plans) and any(p["mid_grid"] for p in plans)
    assert len(cases) > 5000


def test_class_thresholds(planner):
    """One class for counting and scatter, on both sides of each threshold."""
    n = 1_000_000
    want = [(case(n, 0, 4096), "small"), (case(n, 0, 4097), "mid"), (case(n, 0, 80_000), "mid"),
            (case(n, 0, 80_001), "large"), (case(n, 500, 80_500), "mid"), (case(n, 500, 80_501), "large"),
            (case(U32 - 1, 0, 80_000), "mid"), (case(U32, 0, 80_000), "large"), (case(U32, 0, 4096), "small"),
            (case(0, 0, 80_000), "none"), (case(0, 0, 1), "none"),
            (case(n, 0, 80_000, 1, 0), "sel"), (case(n, 0, 80_000, 1, 1), "copy_counts"),
            (case(0, 0, 80_000, 1, 0), "none"), (case(0, 0, 80_000, 1, 1), "copy_counts")]
    for (c, w), p in zip(want, planner([c for c, _ in want])):
        assert p["cls"] == w, c


def test_knob_strings(planner):
    specs = [({}, 2), ({"spec": ""}, 0), ({"spec": "0"}, 0), ({"spec": "2"}, 2), ({"spec": "2,1"}, 0x102),
             ({"spec": "999"}, 255), ({"spec": "-3"}, 0), ({"spec": "7,0"}, 7)]
    assert [p["spec"] for p in planner.parse([s for s, _ in specs])] == [w for _, w in specs]
    fvs = [({}, FVS_NH_MAX), ({"fvs": "6"}, 6), ({"fvs": "40"}, 40), ({"fvs": "1"}, 2), ({"fvs": "100000"}, FVS_NH_MAX),
           ({"exact": 1}, FVS_NH_MAX | 1 << 31), ({"fvs": "40", "exact": 1}, 40 | 1 << 31)]
    assert [p["fvs_max"] for p in planner.parse([s for s, _ in fvs])] == [w for _, w in fvs]
    per_cu = [({}, 2), ({"one": 1}, 1), ({"percu": "1"}, 1), ({"percu": "2", "one": 1}, 2), ({"percu": "9"}, 2),
              ({"percu": "0"}, 1), ({"percu": "-4"}, 1)]
    assert [p["per_cu"] for p in planner.parse([s for s, _ in per_cu])] == [w for _, w in per_cu]


def test_recorded_builds(planner):
    """C1 (1e6 keys), C2 (1e8 keys, 66 667 buckets, the mid class) and the second of C4's six passes (keys, counts
    known, index slots), on 256 CUs: the values gov_build_impl's own expressions gave before the plan existed."""
    c4_n, c4_m = 13_193_787_549, 8_795_859
    c1, c2, c4 = planner([
        case(1_000_000, 0, 667, n_global=1_000_000, st3=0),
        case(100_000_000, 0, 66_667, n_global=100_000_000, st1=0, st3=3),
        case(c4_n, c4_m // 6, 2 * c4_m // 6, 1, 1, n_global=c4_n, n_local=2_198_961_000, want_pos=1)])
    assert c1 == PINNED_C1
    assert c2 == PINNED_C2
    assert c4 == PINNED_C4


PINNED_C1 = {'cls': 'small', 'm': 667, 'nb': 667, 'mult': 1334, 'mid_g': 15, 'cw_bytes': 0, 'mid_bytes': 0, 'count_grid': 245,
    'col_grid': 3, 'base_grid': 3, 'counts_bytes': 2672, 'cursor_bytes': 5336, 'status_bytes': 16, 'values_bytes':
    274416, 'sorted_bytes': 16000000, 'need_pay': 0, 'pay_bytes': 8000000, 'big_cap': 601, 'big_bytes': 2404,
    'per_cu': 2, 'lds_pad': 0, 'solve_grid': 512, 'scratch_bytes': 368050176, 'cursor_grid': 3, 'scatter_grid': 245,
    'sort_grid': 667, 'list_grid': 3, 'verify_grid': 3907, 'led_fail': 0, 'led_claim': 21344, 'led_won': 24012,
    'led_done': 26680, 'led_active': 29348, 'led_zero': 29348, 'led_ones': 2048, 'led_bytes': 31460,
    'sigbits_bytes': 500008, 'nbig': 0, 'nhuge': 0, 'big_sort_grid': 0, 'mid_grid': 0, 'big_grid': 0, 'slabs_bytes':
    0, 'midscr_bytes': 0}
PINNED_C2 = {'cls': 'mid', 'm': 66667, 'nb': 66667, 'mult': 133334, 'mid_g': 256, 'cw_bytes': 34133504, 'mid_bytes': 102400512,
    'count_grid': 256, 'col_grid': 261, 'base_grid': 261, 'counts_bytes': 266672, 'cursor_bytes': 533336,
    'status_bytes': 16, 'values_bytes': 27441408, 'sorted_bytes': 1600000000, 'need_pay': 0, 'pay_bytes': 800000000,
    'big_cap': 60061, 'big_bytes': 240244, 'per_cu': 2, 'lds_pad': 0, 'solve_grid': 512, 'scratch_bytes': 368050176,
    'cursor_grid': 261, 'scatter_grid': 256, 'sort_grid': 2048, 'list_grid': 261, 'verify_grid': 4096, 'led_fail':
    0, 'led_claim': 2133344, 'led_won': 2400012, 'led_done': 2666680, 'led_active': 2933348, 'led_zero': 2933348,
    'led_ones': 2048, 'led_bytes': 2935460, 'sigbits_bytes': 50000008, 'nbig': 3, 'nhuge': 0, 'big_sort_grid': 3,
    'mid_grid': 3, 'big_grid': 0, 'slabs_bytes': 1179648, 'midscr_bytes': 3244032}
PINNED_C4 = {'cls': 'copy_counts', 'm': 8795859, 'nb': 1465977, 'mult': 17591718, 'mid_g': 256, 'cw_bytes': 0, 'mid_bytes': 0,
    'count_grid': 0, 'col_grid': 5727, 'base_grid': 4096, 'counts_bytes': 5863912, 'cursor_bytes': 11727816,
    'status_bytes': 16, 'values_bytes': 3620560848, 'sorted_bytes': 35183376000, 'need_pay': 1, 'pay_bytes':
    17591688000, 'big_cap': 1320698, 'big_bytes': 5282792, 'per_cu': 2, 'lds_pad': 0, 'solve_grid': 512,
    'scratch_bytes': 368050176, 'cursor_grid': 4096, 'scatter_grid': 4096, 'sort_grid': 2048, 'list_grid': 4096,
    'verify_grid': 4096, 'led_fail': 0, 'led_claim': 46911264, 'led_won': 52775172, 'led_done': 58639080,
    'led_active': 64502988, 'led_zero': 64502988, 'led_ones': 2048, 'led_bytes': 64505100, 'sigbits_bytes':
    6596893784, 'nbig': 0, 'nhuge': 0, 'big_sort_grid': 0, 'mid_grid': 0, 'big_grid': 0, 'slabs_bytes': 0,
    'midscr_bytes': 0}
