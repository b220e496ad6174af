"""The duplicate finder's plans (bsdb_amd/csrc/dup_plan.hpp) without a GPU:
tests/dup_plan_check.cpp is built with the system C++ compiler under
ASan + UBSan and run as a program of its own, as tests/test_gov_plan_cpu.py
does for the build's plans; it prints one JSON line per case.  Asserted here,
over key counts from 0 to README size, list capacities and bucket counts
around the sort's limit: every grid lies in [1, 2^32), every size equals the
same expression in Python's integers (nothing wrapped), an oversize bucket is
cut into ceil(count / 16 384) chunks, and 1 <= passes <= m."""
import itertools
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "dup_plan_check.cpp")

GB_CMAX, BUCKET_SIZE = 16384, 1500
U32 = 1 << 32
N = [0, 1, 65_535, 65_536, 100_000_000, 13_193_787_549]
CAP = [0, 1, 1 << 20]
COUNT = [16_384, 16_385, 1_000_000]
GRIDS = ("collect_grid", "big_sort_grid", "over_grid", "over_sort_grid", "over_collect_grid", "classify_grid")


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler on this machine")
    exe = str(tmp_path_factory.mktemp("dup_plan") / "dup_plan_check")
    # The sanitizer runtimes are linked into the program (g++ needs the two flags, clang does so by itself and
    # does not know them), so it starts whatever else the environment preloads; the environment is passed on as it is.
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-o", exe, SRC]
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True)
    probe = subprocess.run([exe], input="", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the sanitized program does not start in this environment: " + probe.stderr.strip()[-300:])

    def plans(cases):
        lines = [" ".join(f"{k}={int(v)}" for k, v in c.items()) for c in cases]
        r = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        out = [json.loads(line) for line in r.stdout.splitlines()]
        assert len(out) == len(cases)
        return out

    return plans


def grid_checks(p):
    for g in GRIDS:
        assert 1 <= p[g] < U32, (g, p)


def test_passes(planner):
    cases = [dict(n=n, passes=ps, free=fr, source_bpk=sb)
             for n, ps, fr, sb in itertools.product(N, [0, 1, 3, 7, 64, 4096], [0, 1 << 30, 280 << 30], [0, 56])]
    for c, p in zip(cases, planner(cases)):
        m = c["n"] // BUCKET_SIZE + 1
        assert p["m"] == m and 1 <= p["passes"] <= m, (c, p)
        assert p["bytes_per_key"] == 24 + c["source_bpk"]
        if c["passes"]:
            assert p["passes"] == min(c["passes"], m)
        else:
            assert p["passes"] <= 64
            room = 0.85 * c["free"] - 1e9
            if room > 0 and p["passes"] < min(64, m):  # the chosen passes' working set fits the room
                assert 1.05 * c["n"] * p["bytes_per_key"] <= p["passes"] * room * (1 + 1e-9), (c, p)
    # README size on a device with 280 GB free: 13.19e9 keys x 24 B in two passes
    assert planner([dict(n=N[-1], free=280 * 10**9)])[0]["passes"] == 2
    assert planner([dict(n=N[-2], free=280 * 10**9)])[0]["passes"] == 1


def test_one_pass_collect_and_chunks(planner):
    cases = [dict(nb=nb, n_local=n, nbig=nbig, num_cus=cus, count=count, listed=listed)
             for n, nbig, cus, count in itertools.product(N, [0, 1, 300, U32 - 1], [1, 256, 304], COUNT)
             for nb in {1, n // BUCKET_SIZE + 1, max(1, (n // BUCKET_SIZE + 1) // 7)}
             for listed in {0, 1, -(-count // GB_CMAX), n // GB_CMAX + 5, U32 - 1}]
    for c, p in zip(cases, planner(cases)):
        grid_checks(p)
        n, cus = c["n_local"], c["num_cus"]
        assert p["collect_grid"] == max(1, min(c["nb"], cus * 8))
        assert p["big_sort_grid"] == max(1, min(c["nbig"], cus))
        assert p["slabs_bytes"] == p["big_sort_grid"] * GB_CMAX * 24
        # every oversize bucket holds more than GB_CMAX of the pass's keys; its chunks are full but the last
        assert p["over_cap"] == n // (GB_CMAX + 1) + 1 and p["chunk_cap"] == n // GB_CMAX + p["over_cap"]
        most_over = n // (GB_CMAX + 1)
        assert most_over <= p["over_cap"] and n // GB_CMAX + most_over <= p["chunk_cap"]
        assert p["over_bytes"] == (p["chunk_cap"] + p["over_cap"]) * 8 + p["chunk_cap"] * 4 + 64
        assert p["bucket_chunks"] == -(-c["count"] // GB_CMAX)  # ceil
        assert (p["bucket_chunks"] - 1) * GB_CMAX < c["count"] <= p["bucket_chunks"] * GB_CMAX
        assert p["chunks"] == min(c["listed"], p["chunk_cap"])
        assert p["over_sort_grid"] == max(1, min(p["chunks"], cus))
        assert p["over_collect_grid"] == max(1, min(p["chunks"], cus * 8))
        assert p["over_slabs_bytes"] == p["over_sort_grid"] * GB_CMAX * 24


def test_issue_bucket_counts(planner):
    got = [p["bucket_chunks"] for p in planner([dict(count=c) for c in COUNT])]
    assert got == [1, 2, 62]


def test_list(planner):
    cases = [dict(found=f, cap=cap, num_cus=cus)
             for cap, cus in itertools.product(CAP, [1, 256])
             for f in {0, 1, cap, cap + 1, 39_999, N[-1]}]
    for c, p in zip(cases, planner(cases)):
        grid_checks(p)
        assert p["listed"] == min(c["found"], c["cap"]) and p["list_full"] == int(c["found"] > c["cap"])
        assert p["pairs_bytes"] == 16 * c["cap"] and p["kinds_bytes"] == c["cap"]
        assert p["classify_grid"] == max(1, min(-(-p["listed"] // 256), c["num_cus"] * 16))
