"""The plans of the diff of two resident databases (bsdb_amd/csrc/diff_plan.hpp)
without a GPU: tests/diff_plan_check.cpp is built with the system C++ compiler
under ASan + UBSan and run as a program of its own, as
tests/test_check_plan_cpu.py does for the check's plans.  Asserted here: the
codes and the report's words are the header's, a selection's mask may name
statuses 0 .. 5 only, and every grid lies in [1, 2^32): a record per lane capped
at 16 workgroups a CU, a thread per 16 bytes of the most `count` records can
hold capped at 32 workgroups a CU, with no product that wraps."""
import itertools
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "diff_plan_check.cpp")
HDR = os.path.join(ROOT, "include", "bsdb_mi355x.h")
U32 = 1 << 32
MAX_COUNT, MAX_VALUE = 1 << 40, 65535


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler on this machine")
    exe = str(tmp_path_factory.mktemp("diff_plan") / "diff_plan_check")
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


def test_constants_are_the_headers(planner):
    p = planner([dict(count=0)])[0]
    hdr = open(HDR).read()
    define = {k: int(v) for k, v in re.findall(r"#define\s+(BSDB_\w+)\s+(\d+)\s", hdr)}
    assert (p["words"], p["same"], p["bad_slot"]) == (define["BSDB_DIFF_WORDS"], define["BSDB_DIFF_SAME"], define["BSDB_DIFF_BAD_SLOT"]) \
        == (10, 0, 6)
    assert (p["first_diff"], p["compared_bytes"]) == (8, 9)
    assert p["selectable"] == 0x3F
    get, chk = [define[f"BSDB_GET_{k}"] for k in ("REJECTED", "KEY_MISMATCH")], [define[f"BSDB_CHECK_{k}"] for k in ("VALUE_LEN", "VALUE_BYTES")]
    assert p["mask_absent"] == sum(1 << s for s in get) == 0b000110
    assert p["mask_upsert"] == sum(1 << s for s in get + chk) == 0b110110
    assert p["max_count"] == MAX_COUNT and MAX_COUNT * MAX_VALUE < 1 << 64
    import bsdb_amd.native as N
    assert (N.DIFF_WORDS, N.DIFF_SAME, N.DIFF_BAD_SLOT, N.DIFF_MASK_ABSENT, N.DIFF_MASK_UPSERT) == (10, 0, 6, 6, 0x36)
    assert len(N.DIFF_FIELDS) == N.DIFF_WORDS and N.DIFF_FIELDS.index("first_diff") == 8


def test_masks(planner):
    masks = [0, 1, 2, 0x36, 0x3F, 0x40, 0x41, 0x7F, 0x80, 1 << 31, U32 - 1]
    for m, p in zip(masks, planner([dict(mask=m) for m in masks])):
        assert p["bad_mask"] == int(m >> 6 != 0), m


def test_grids(planner):
    cases = [dict(count=n, num_cus=cus)
             for n, cus in itertools.product([0, 1, 63, 64, 65, 255, 256, 257, 4096, 10**7, 1 << 30, MAX_COUNT, MAX_COUNT + 1, (1 << 64) - 1],
                                             [0, 1, 256, 304])]
    for c, p in zip(cases, planner(cases)):
        cus = max(1, c["num_cus"])
        assert 1 <= p["lane_grid"] < U32 and 1 <= p["values_grid"] < U32
        assert p["lane_grid"] == max(1, min(-(-c["count"] // 256), cus * 16)), c
        pieces = -(-min(c["count"], MAX_COUNT) * MAX_VALUE // 16)
        assert p["values_grid"] == max(1, min(-(-pieces // 256), cus * 32)), c
    by = {(c["count"], c["num_cus"]): p for c, p in zip(cases, planner(cases))}
    # count 0: one workgroup that finds nothing; one wave of records: one workgroup of lanes, and a workgroup of
    # compare threads per 4 096 bytes they may hold; many records: the caps by CU count
    assert (by[(0, 256)]["lane_grid"], by[(0, 256)]["values_grid"]) == (1, 1)
    assert (by[(64, 256)]["lane_grid"], by[(64, 256)]["values_grid"]) == (1, -(-64 * MAX_VALUE // 4096))
    assert (by[(10**7, 256)]["lane_grid"], by[(10**7, 256)]["values_grid"]) == (256 * 16, 256 * 32)
    assert (by[(10**7, 1)]["lane_grid"], by[(10**7, 1)]["values_grid"]) == (16, 32)
