"""The plans of the enumeration of a resident database by slot
(bsdb_amd/csrc/dump_plan.hpp) without a GPU: tests/dump_plan_check.cpp is
built with the system C++ compiler under ASan + UBSan and run as a program of
its own, as tests/test_get_plan_cpu.py does for the batched reader's plans; it
prints one JSON line per case.  Asserted here, against the same expressions in
Python's integers: dump_cut (the records of a chunk whose text fits the cap,
at least one), a record's line length and the length part of the text test at
the edges of the header's and the text front end's limits, the grids (every
one in [1, 2^32), nothing wrapped) and the text-chunk cap's rule."""
import itertools
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "dump_plan_check.cpp")
U32 = 1 << 32
OK, BAD_ADDR, NOT_TEXT = 0, 1, 2
MAX_LINE = 255 + 65535 + 2


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler on this machine")
    exe = str(tmp_path_factory.mktemp("dump_plan") / "dump_plan_check")
    # (the sanitizer runtimes are linked into the program: see tests/test_get_plan_cpu.py)
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-o", exe, SRC]
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True)
    probe = subprocess.run([exe], input="", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the sanitized program does not start in this environment: " + probe.stderr.strip()[-300:])

    def tok(v):
        return ",".join(str(int(x)) for x in v) if isinstance(v, (list, tuple)) else str(int(v))

    def plans(cases):
        lines = [" ".join(f"{k}={tok(v)}" for k, v in c.items() if not (isinstance(v, (list, tuple)) and not v)) for c in cases]
        r = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        out = [json.loads(line) for line in r.stdout.splitlines()]
        assert len(out) == len(cases)
        return out

    return plans


def cut_of(llen, cap):
    """The largest k >= 1 whose first k lines fit cap bytes (k = 1 whatever the first line's length); 0 of none."""
    if not llen:
        return 0
    k, total = 0, 0
    while k < len(llen) and total + llen[k] <= cap:
        total += llen[k]
        k += 1
    return max(k, 1)


def test_dump_cut(planner):
    lines = [10, 20, 30, 5, 5, 100, 1]
    zeros = [0, 0, 7, 0, 0, 0, 9, 0, 3, 0, 0]                 # BAD_ADDR slots: entries of length 0
    cases = []
    for llen in (lines, zeros, [MAX_LINE], [MAX_LINE, 4, MAX_LINE], [0], [0, 0, 0], [4] * 300, []):
        total = sum(llen)
        caps = {0, 1, total - 1, total, total + 1, 1 << 62, (1 << 64) - 1} | {c for l in itertools.accumulate(llen)
                                                                              for c in (l - 1, l, l + 1)}
        for cap in sorted(c for c in caps if c >= 0):
            for loff0 in (0, 12345):                          # (a scan that starts anywhere: the cut is relative)
                cases.append(dict(llen=llen, cap=cap, loff0=loff0))
    for c, p in zip(cases, planner(cases)):
        want = cut_of(c["llen"], c["cap"])
        assert p["cut"] == want, (c, p)
        if c["llen"]:
            assert 1 <= p["cut"] <= len(c["llen"])            # the host form always advances
            assert sum(c["llen"][: p["cut"]]) <= c["cap"] or p["cut"] == 1
    by = {(tuple(c["llen"]), c["cap"], c["loff0"]): p["cut"] for c, p in zip(cases, planner(cases))}
    L = tuple(lines)
    assert by[(L, 9, 0)] == 1          # a cap below one line: the first line alone over the cap still returns 1
    assert by[(L, 10, 0)] == 1         # at one line
    assert by[(L, 11, 0)] == 1         # above one line, below two
    assert by[(L, 30, 0)] == 2
    assert by[(L, 171, 0)] == by[(L, 1 << 62, 0)] == 7       # a chunk that fits whole
    assert by[(L, 170, 0)] == 6
    Z = tuple(zeros)
    assert by[(Z, 0, 0)] == 2          # the empty entries before the first line that has bytes
    assert by[(Z, 7, 0)] == 6 and by[(Z, 16, 0)] == 8 and by[(Z, 19, 0)] == 11
    assert by[((MAX_LINE,), 0, 0)] == 1 and by[((), 1, 0)] == 0


def test_line_length_and_length_status(planner):
    cases = [dict(status=s, klen=k, vlen=v) for s in (OK, BAD_ADDR, NOT_TEXT, 3, 255) for k in (0, 1, 255)
             for v in (0, 1, 32510, 32511, 65535)]
    hostile = [dict(status=OK, klen=k, vlen=v) for k, v in ((256, 5), (U32 - 1, 5), (5, 65536), (5, U32 - 1), (U32 - 1, U32 - 1))]
    for c, p in zip(cases + hostile, planner(cases + hostile)):
        s, k, v = c["status"], c["klen"], c["vlen"]
        assert p["status_in"] == (s if s in (OK, NOT_TEXT) else BAD_ADDR)
        if s == BAD_ADDR:
            assert p["line_len"] == 0 and p["length_status"] == BAD_ADDR, (c, p)
            continue
        assert p["line_len"] == min(k, 255) + 1 + min(v, 65535) + 1 <= MAX_LINE, (c, p)
        if s == OK:
            text = 1 <= k <= 255 and 1 <= v <= 32510          # TEXT_MAX_KEY, TEXT_MAX_VALUE
            assert p["length_status"] == (OK if text else NOT_TEXT), (c, p)
    assert planner([dict(count=0)])[0]["max_line"] == MAX_LINE


def test_grids(planner):
    cases = [dict(count=n, text_bytes=tb, mis=mis, num_cus=cus)
             for n, tb, mis, cus in itertools.product([0, 1, 255, 256, 257, 1 << 40], [0, 1, 15, 16, 17, 65792, 1 << 40, (1 << 64) - 1],
                                                      [0, 5, 15], [1, 256, 304])]
    for c, p in zip(cases, planner(cases)):
        assert 1 <= p["lane_grid"] < U32 and 1 <= p["text_grid"] < U32, (c, p)
        assert p["lane_grid"] == max(1, min(-(-c["count"] // 256), c["num_cus"] * 16))       # get_locate_grid's rule
        pieces = -(-(c["text_bytes"] + c["mis"]) // 16) if c["text_bytes"] else 0
        assert p["text_grid"] == max(1, min(-(-pieces // 256), c["num_cus"] * 32, U32 - 1))  # piece_grid
    # the record kernels' cap on 256 CUs: 1 048 576 lanes, so 1 100 000 records enter the second trip
    p = planner([dict(count=1_100_000, num_cus=256)])[0]
    assert p["lane_grid"] * 256 == 1_048_576 < 1_100_000


def test_text_chunk_cap(planner):
    cases = [dict(chunk=c) for c in (0, 1, MAX_LINE - 1, MAX_LINE, MAX_LINE + 1, 256 << 20, 1 << 40)]
    for c, p in zip(cases, planner(cases)):
        assert p["bad_chunk"] == int(0 < c["chunk"] < MAX_LINE), (c, p)
        assert p["chunk_bytes"] == (c["chunk"] or 256 << 20)
