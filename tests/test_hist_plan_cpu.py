"""The histogram's launch planner (bsdb_amd/csrc/hist_plan.hpp) without a GPU:
tests/hist_plan_check.cpp is built with the system C++ compiler under
ASan + UBSan and run as a program of its own; it prints one JSON line per case
(the plan, and sums over every launch the plan enumerates).  Asserted here: the
invariants every plan must keep, over a grid of key sets and knobs, and the
values the project has recorded for C4 and for the 16-launch test shape."""
import itertools
import json
import math
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hist_plan_check.cpp")

P1_TILE = 8192
D13E_TILE = 16384
PART_SHIFT = 15
C4_N, C4_M = 13_193_787_549, 8_795_859
AMPLE = 256 * 10**9
ENUM_MAX = 2_000    # launches enumerated per case; a case with more is checked on its plan alone
DETAIL = 64         # launches listed one by one


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler on this machine")
    exe = str(tmp_path_factory.mktemp("hist_plan") / "hist_plan_check")
    # The sanitizer runtimes are linked into the program (g++ needs the two flags, clang does so by itself and
    # does not know them), so it starts whatever else the environment preloads; the environment is passed on as it is.
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-o", exe, SRC]
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True)
    probe = subprocess.run([exe], input="", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the sanitized program does not start in this environment: " + probe.stderr.strip()[-300:])

    def run(cases):
        text = "".join(" ".join(f"{k}={int(v)}" for k, v in c.items()) + "\n" for c in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        out = [json.loads(line) for line in r.stdout.splitlines()]
        assert len(out) == len(cases)
        return out

    return run


def case(key_len, n, m, **kw):
    """key_len None: variable-length keys (20 bytes a key on average)."""
    var = key_len is None
    c = dict(var=var, key_len=0 if var else key_len, n=n, m=m, blob_bytes=n * (20 if var else key_len), seed0=1,
             num_cus=256, wg_per_cu=1 if key_len in (8, 12, 13, 16) else 4, free_bytes=AMPLE, ids_bytes=0,
             detail=DETAIL)
    c.update(kw)
    return c


def expected_launches(c):
    return -(-c["n"] // max(P1_TILE, c.get("chunk_keys") or 1 << 32))


def check(c, p):
    """The invariants of one plan; c: the case, p: the program's line for it."""
    ctx = (c, p)
    nparts = -(-c["m"] // (1 << PART_SHIFT))
    if p["atomic"]:
        assert c.get("hist_mode") == 2 or nparts > 512, ctx
        return
    has_kernel = p["kind"] != "none"
    # the kernel choice
    if has_kernel:
        assert p["nparts"] == -(-c["m"] // (1 << p["bin_shift"])) and p["bin_shift"] <= PART_SHIFT, ctx
        assert p["nparts"] <= {"d13e": 288, "vare": 144, "d13": 1024}[p["kind"]], ctx
        assert p["tile"] == {"d13e": D13E_TILE, "vare": 8192, "d13": 8192}[p["kind"]], ctx
    else:
        assert (p["nparts"], p["bin_shift"], p["tile"]) == (nparts, PART_SHIFT, 0), ctx
    if p["binned"]:
        assert p["capb"] % 8 == 0 and p["nparts"] * p["capb"] <= {"d13e": 36864, "vare": 18432}[p["kind"]], ctx
    # the buffers: [nmain][P][cap] + [ntail][P][cap_tail]; cursors, scratch and prefix as the workspace grows them
    assert p["nmain"] == (c.get("d13_copies", 8) if p["binned"] else 8), ctx
    assert p["ntail"] == (8 if has_kernel else 0), ctx
    assert p["set_elems"] == p["nmain"] * p["nparts"] * p["cap"], ctx
    assert p["tail_elems"] == p["ntail"] * p["nparts"] * p["cap_tail"], ctx
    assert p["ids_per_buf"] == p["set_elems"] + p["tail_elems"], ctx
    assert p["cur_per_buf"] == p["nparts"] * (p["nmain"] + p["ntail"]), ctx
    assert p["nbuf"] == (2 if p["pipe"] else 1), ctx
    assert p["ids_bytes"] == p["nbuf"] * p["ids_per_buf"] * 2, ctx
    assert p["cursor_bytes"] == (p["nbuf"] * p["cur_per_buf"] + 10240 + 2048 * 1024) * 4, ctx
    assert p["prefix_bytes"] == p["nbuf"] * (p["cur_per_buf"] + 1) * 8, ctx
    assert p["cap"] % 64 == 0 and p["cap_tail"] % 64 == 0, ctx
    if has_kernel:
        assert p["cap_tail"] >= max(P1_TILE, p["tile"]), ctx  # a tail region holds a whole tile of one bin
    # the rules of the halving
    pipe_pl = bool(c.get("pipe")) and p["windowed"] and p["binned"]
    budget = (c["free_bytes"] + c["ids_bytes"]) // 2 // (2 if pipe_pl else 1)
    rules = p["nparts"] * p["cap"] < 1 << 32 and p["keys_per_copy"] < 1 << 32 and p["ids_per_buf"] * 2 <= budget
    if p["bottomed_out"]:
        assert not rules and p["launch"] <= 2 * P1_TILE and p["per_span"] == 1, ctx
    else:
        assert rules, ctx
    assert p["launch"] >= 1 and p["per_span"] >= 1, ctx
    assert p["pipe"] == (pipe_pl and c["n"] > p["launch"]), ctx
    if p["pipe"]:
        assert p["per_span"] == 1 and 1 <= p["p2_cus"] <= c["num_cus"] // 2, ctx
    if "launches" not in p:
        return
    # the launches tile [0, n) in order; persistent part + tail = the launch
    for k in ("bad_cover", "bad_split", "bad_blob", "bad_window", "bad_grid", "bad_pipe_grid", "bad_buf"):
        assert p[k] == 0, (k, ctx)
    assert p["spans"] >= 1 and p["launches"] >= p["spans"], ctx
    assert p["max_span_launches"] <= p["per_span"], ctx
    if has_kernel and p["launch"] % p["tile"] == 0:
        assert p["nonlast_tails"] == 0, ctx  # only a span's last launch leaves a tail
    if not has_kernel:
        assert p["tails"] == 0, ctx
    # capacity, from the tiles as dealt
    assert p["keys_per_copy"] >= p["max_copy_keys"], ctx
    share = p["max_copy_keys"] * min(1.0, (1 << p["bin_shift"]) / c["m"])
    pads = 0
    if p["kind"] == "d13e":
        pads = 7 * (p["grid_d13"] // p["nmain"] + 1) * p["max_span_launches"]
    elif p["kind"] == "vare":
        pads = 7 * p["max_copy_tiles"]
    assert p["cap"] >= share * 1.02 + 8 * math.sqrt(share) + pads, ctx
    if "launch_list" in p:
        check_launches(c, p)


def check_launches(c, p):
    """The listed launches again, from the list alone (and tile by tile for small sets)."""
    ctx = (c, p)
    L = 0 if c["var"] else c["key_len"]
    tile = p["tile"] or P1_TILE
    nxt = 0
    per_span = {}
    for span, k0, nk, blob, grid, tiles, t0, tn, tblob, ttiles in p["launch_list"]:
        assert k0 == nxt and nk > 0, ctx
        nxt = k0 + nk
        fast = tiles * tile if p["kind"] != "none" else nk
        if tn:
            assert (t0, tn) == (k0 + fast, nk - fast) and ttiles == -(-tn // P1_TILE), ctx
            assert c["var"] or tblob == tn * L, ctx
        else:
            assert fast == nk, ctx
        if not c["var"]:
            assert nk * L <= blob <= c["blob_bytes"] - k0 * L, ctx
        if p["windowed"] and tiles:
            assert tiles * tile * L + (16 - L) <= blob, ctx
        if p["kind"] != "none" and tiles:
            assert 1 <= grid <= min(tiles, p["grid_d13"]), ctx
        per_span.setdefault(span, []).append(nk)
    assert nxt == c["n"], ctx
    spans = p["span_list"]
    assert [s[3] for s in spans] == [len(per_span[i]) for i in range(len(spans))], ctx
    assert [s[1] for s in spans] == [sum(per_span[i]) for i in range(len(spans))], ctx
    for i, (s0, ns, blob, nl, buf, p2_grid) in enumerate(spans):
        assert buf == (i & 1 if p["pipe"] else 0), ctx
        assert p2_grid == (p["p2_cus"] if p["pipe"] and s0 + ns < c["n"] else c["num_cus"]), ctx
        assert c["var"] or ns * L <= blob <= c["blob_bytes"] - s0 * L, ctx
    if c["n"] <= 1 << 20:
        worst = 0
        for nks in per_span.values():
            copies = [0] * p["nmain"]
            for nk in nks:
                for t in range(-(-nk // tile)):
                    copies[t % p["nmain"]] += min(tile, nk - t * tile)
            worst = max(worst, max(copies))
        assert worst == p["max_copy_keys"] <= p["keys_per_copy"], ctx


KEY_LENS = (8, 12, 13, 16, 20, None)
MS = (1, 667, C4_M, 9_437_184, 144 * 32768, 288 * 32768 + 1)
NS = (1, 777, D13E_TILE - 1, D13E_TILE, D13E_TILE + 1, 15 * D13E_TILE + 777, 9 * D13E_TILE, 5 * 17 * D13E_TILE + 3,
      (1 << 32) - 1, (1 << 32) + 1, C4_N, 4_000_000_000)
LAUNCHES = (P1_TILE, D13E_TILE, 3 * D13E_TILE, 9 * D13E_TILE, 17 * D13E_TILE) + tuple(1 << k for k in range(27, 34)) + (0,)


def grid_cases():
    out = []

    def add(c):
        out.append(dict(c, enum_max=ENUM_MAX))

    # launch length x span limit, every key kind and size
    for L, m, n, ch, sm in itertools.product(KEY_LENS, MS, NS, LAUNCHES, (0, 1, 2)):
        if sm and expected_launches(dict(n=n, chunk_keys=ch)) == 1 and n > 777:
            continue  # (a span limit changes nothing in a call of one launch)
        add(case(L, n, m, chunk_keys=ch, span_max=sm))
    some_n = (777, 15 * D13E_TILE + 777, 5 * 17 * D13E_TILE + 3, (1 << 32) + 1, C4_N)
    some_ch = (0, D13E_TILE, 9 * D13E_TILE, 1 << 28)
    # the pipelined mode
    for L, m, n, ch, nch, cus in itertools.product(KEY_LENS, MS, some_n, some_ch, (4, 8), (0, 200)):
        add(case(L, n, m, chunk_keys=ch, pipe=1, pipe_chunks=nch, pipe_cus=cus))
    # region copies and the grid knob
    for L, m, n, ch, cp, g in itertools.product(KEY_LENS, MS, some_n, some_ch, (8, 16, 32), (None, 2)):
        if cp == 8 and g is None:
            continue
        c = case(L, n, m, chunk_keys=ch, d13_copies=cp)
        if g is not None:
            c["d13_grid"] = g
        add(c)
    # budgets, from ample down to a few MB (some already held by the context)
    for L, m, n, ch, (free, held), pipe in itertools.product(
            KEY_LENS, MS, some_n, (0, 1 << 28),
            ((64 * 10**9, 0), (8 * 10**9, 10**9), (512 * 10**6, 0), (48 * 10**6, 16 * 10**6), (4 * 10**6, 0)), (0, 1)):
        add(case(L, n, m, chunk_keys=ch, free_bytes=free, ids_bytes=held, pipe=pipe))
    # the other kernels and modes
    for L, m, n in itertools.product(KEY_LENS, MS, some_n):
        for kw in (dict(frontend=1), dict(hist_mode=2), dict(d13_variant=2), dict(d13_variant=0, no_seed0=1),
                   dict(no_fixed_window=1), dict(wg_per_cu=0)):
            add(case(L, n, m, **kw))
    # long sets in launches of one tile, enumerated in full
    out.append(case(13, (1 << 32) + 1, C4_M, chunk_keys=D13E_TILE))
    out.append(case(None, 4_000_000_000, 667, chunk_keys=P1_TILE, span_max=2))
    return out


def test_invariants_over_the_grid(planner):
    cases = grid_cases()
    plans = planner(cases)
    enumerated = 0
    for c, p in zip(cases, plans):
        check(c, p)
        enumerated += "launches" in p
    assert enumerated > 0.8 * len(cases)
    # the grid reaches every kernel, both modes, the pipelined mode and both ends of the halving
    assert {p["kind"] for p in plans} == {"none", "d13", "d13e", "vare"}
    assert any(p["atomic"] for p in plans) and any(p.get("pipe") for p in plans)
    assert any(p.get("bottomed_out") for p in plans)
    assert any(not p["atomic"] and not p["bottomed_out"] and c["free_bytes"] < AMPLE and p["launch"] < (c.get("chunk_keys") or 1 << 32)
               and p["launch"] < c["n"] for c, p in zip(cases, plans))


def test_kernel_choice(planner):
    """pass1_select's rules, one key set each: (kernel, its key length, VARIANT, seed folded)."""
    small, big = 667, 288 * 32768
    want = [
        (case(13, 10**6, C4_M), ("d13e", 13, 13, 1)),
        (case(13, 10**6, C4_M, d13_variant=0), ("d13e", 13, 0, 1)),
        (case(13, 10**6, C4_M, d13_variant=7, no_seed0=1), ("d13e", 13, 0, 0)),
        (case(13, 10**6, C4_M, seed0=0), ("d13e", 13, 13, 0)),
        (case(13, 10**6, C4_M, d13_variant=2), ("d13", 13, 0, 0)),
        (case(13, 10**6, big), ("d13e", 13, 13, 1)),
        (case(13, 10**6, big + 1), ("d13", 13, 0, 0)),
        (case(13, 10**6, small, frontend=1), ("none", 0, 0, 0)),
        (case(20, 10**6, small), ("vare", 20, 0, 1)),
        (case(32, 10**6, small), ("vare", 32, 0, 1)),
        (case(33, 10**6, small), ("none", 0, 0, 0)),
        (case(None, 10**6, small), ("vare", 0, 0, 1)),
        (case(None, 10**6, small, seed0=0), ("vare", 0, 0, 0)),
        (case(None, 10**6, 144 * 32768), ("vare", 0, 0, 1)),
        (case(None, 10**6, 144 * 32768 + 1), ("none", 0, 0, 0)),
        (case(None, 10**6, small, frontend=2), ("none", 0, 0, 0)),
    ]
    for L in (8, 12, 16):
        want += [(case(L, 10**6, big), ("d13e", L, 0, 1)), (case(L, 10**6, big + 1), ("none", 0, 0, 0)),
                 (case(L, 10**6, small, no_fixed_window=1), ("vare", L, 0, 1)),
                 (case(L, 10**6, 144 * 32768 + 1, no_fixed_window=1), ("none", 0, 0, 0))]
    for (c, w), p in zip(want, planner([c for c, _ in want])):
        assert (p["kind"], p["k_key_len"], p["variant"], p["k_seed0"]) == w, c
    atomic = planner([case(13, 10**6, 512 * 32768 + 1), case(13, 10**6, 512 * 32768), case(13, 10**6, small, hist_mode=2)])
    assert [p["atomic"] for p in atomic] == [1, 0, 1]


def test_c4_plans_as_recorded(planner):
    """C4 on 256 CUs, one workgroup per CU, 8 copies, ample memory: the launches per
    step of profiles/launch_length/README.md, one span, a tail in the last launch only."""
    chunks = {32: 4, 31: 7, 30: 13, 29: 25, 28: 50, 27: 99}
    plans = planner([case(13, C4_N, C4_M, chunk_keys=1 << k) for k in chunks] + [case(13, C4_N, C4_M)])
    for (k, want), p in zip(chunks.items(), plans):
        assert (p["kind"], p["bin_shift"], p["nparts"], p["nmain"]) == ("d13e", 15, 269, 8)
        assert (p["launch"], p["spans"], p["launches"], p["per_span"]) == (1 << k, 1, want, want)
        assert (p["tails"], p["nonlast_tails"], p["tail_only"]) == (1, 0, 0)
        assert p["grid_d13"] == 256 and not p["pipe"] and not p["bottomed_out"]
    assert plans[0]["cap"] == 6_304_128  # the 6.31 M ids of DESIGN §4.1
    assert plans[-1] == plans[0]  # 2^32 is the default
    # the full build's histogram: launches of 2^30, a pass 2 each
    p = planner([case(13, C4_N, C4_M, chunk_keys=1 << 30, span_max=1)])[0]
    assert (p["spans"], p["launches"], p["per_span"], p["max_span_launches"]) == (13, 13, 1, 1)


def test_sixteen_launches_as_the_device_test_sees_them(planner):
    """N = 15 x 16384 + 777 in launches of one tile: 16 launches, the last tail-only;
    16 / 8 / 1 spans for a span limit of 1 / 2 / none (test_span_regions_gpu.py).  A span's
    last launch reads no byte past its own keys, so a last launch of one whole tile goes
    to the bounds-checked kernel as well: a tail per span."""
    n = 15 * D13E_TILE + 777
    plans = planner([case(13, n, C4_M, chunk_keys=D13E_TILE, span_max=sm) for sm in (1, 2, 0)])
    assert [p["spans"] for p in plans] == [16, 8, 1]
    for p in plans:
        assert (p["launches"], p["nonlast_tails"]) == (16, 0) and p["tails"] == p["tail_only"] == p["spans"]
        last = p["launch_list"][-1]
        assert last[1:3] == [15 * D13E_TILE, 777] and last[5] == 0 and last[6:8] == [15 * D13E_TILE, 777]
