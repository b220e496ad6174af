"""The plans of the merge of resident databases (bsdb_amd/csrc/merge_plan.hpp)
without a GPU: tests/merge_plan_check.cpp is built with the system C++ compiler
under ASan + UBSan and run as a program of its own, as
tests/test_diff_plan_cpu.py does for the diff's plans.  Asserted here: the
codes and the report's words are the header's; the status rule for every
combination of three status bytes; the grids; the chunk cut (the largest
prefix whose image stays under the cap, a single record above it alone) against
a restatement; the image bound of either layout against a byte-level placement
of random records; and the smallest output at which a workgroup of the pack
takes a second trip of its piece loop."""
import itertools
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "merge_plan_check.cpp")
HDR = os.path.join(ROOT, "include", "bsdb_mi355x.h")
U32 = 1 << 32
MAX_RECORD = 3 + 255 + 32510
KEPT, REPLACED, REMOVED, BAD_SLOT, BAD_ADDR = range(5)


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler on this machine")
    exe = str(tmp_path_factory.mktemp("merge_plan") / "merge_plan_check")
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-o", exe, SRC]
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True)
    probe = subprocess.run([exe], input="", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the sanitized program does not start in this environment: " + probe.stderr.strip()[-300:])

    def plans(cases):
        lines = [" ".join(f"{k}={v if k == 'sizes' else int(v)}" for k, v in c.items()) for c in cases]
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
    assert p["words"] == define["BSDB_MERGE_WORDS"] == 12
    assert [p[k] for k in ("kept", "replaced", "removed", "bad_slot", "bad_addr")] == \
        [define[f"BSDB_MERGE_{k}"] for k in ("KEPT", "REPLACED", "REMOVED", "BAD_SLOT", "BAD_ADDR")] == [0, 1, 2, 3, 4]
    assert p["mask_kept"] == 1 and p["out_records"] == 9 and p["max_record"] == MAX_RECORD == 32768 and p["max_count"] == 1 << 40
    import bsdb_amd.native as N
    assert N.MERGE_WORDS == len(N.MERGE_FIELDS) == 12 and N.MERGE_FIELDS.index("out_records") == 9
    assert (N.MERGE_KEPT, N.MERGE_REPLACED, N.MERGE_REMOVED, N.MERGE_BAD_SLOT, N.MERGE_BAD_ADDR) == (0, 1, 2, 3, 4)


def test_status_rule(planner):
    """Every combination of a scan status and two locate statuses, bytes that are no code included."""
    codes = [0, 1, 2, 3, 4, 7, 255]
    cases = [dict(scan=s, delta=d, removed=r) for s, d, r in itertools.product(codes, codes, codes)]
    for c, p in zip(cases, planner(cases)):
        s, d, r = c["scan"], min(c["delta"], 3), min(c["removed"], 3)
        if s not in (0, 2):                 # OK and NOT_TEXT are records; everything else names none
            want = BAD_SLOT
        elif 3 in (d, r):
            want = BAD_ADDR
        elif d == 0:
            want = REPLACED                 # delta wins when removed holds the key too
        else:
            want = REMOVED if r == 0 else KEPT
        assert p["status"] == want, c
        assert p["locate_in"] == d


def test_grids_and_second_trip(planner):
    cases = [dict(count=n, num_cus=cus, out_bytes=b, mis=mis)
             for n, cus, b, mis in itertools.product([0, 1, 64, 257, 10**7, 1 << 40], [0, 1, 256, 304], [0, 1, 16, 4097, 1 << 34], [0, 1, 15])]
    for c, p in zip(cases, planner(cases)):
        cus = max(1, c["num_cus"])
        assert p["lane_grid"] == max(1, min(-(-c["count"] // 256), cus * 16)), c
        pieces = -(-(c["out_bytes"] + c["mis"]) // 16) if c["out_bytes"] else 0
        assert p["pack_grid"] == max(1, min(-(-pieces // 256), cus * 32)), c
        # one piece more than the largest grid holds threads: the first output with a second trip, and not a byte sooner
        assert p["pieces_at"] == cus * 32 * 256 + 1 and p["grid_at_second_trip"] == p["grid_before"] == cus * 32
        assert p["second_trip"] == cus * 32 * 256 * 16 - c["mis"] + 1
    assert planner([dict(num_cus=256)])[0]["second_trip"] == (32 << 20) + 1


def place(sizes, parts, B):
    """The image's bytes of one pack: run p by the writers' rules (compact: back to back; blocked: text_place_blocked)."""
    k, total = len(sizes), 0
    for p in range(parts):
        run = sizes[p * k // parts: (p + 1) * k // parts]
        if not B:
            total += sum(run)
            continue
        fill, opened = 0, False
        for s in run:
            if s > B:
                total += -(-s // 4096) * 4096
                continue
            if opened and B - fill < s:
                total += B
                opened = False
            if not opened:
                opened, fill = True, 0
            fill += s
        total += B if opened else 0
    return total


def test_cut_and_image_bound(planner):
    rng = np.random.default_rng(11)
    cases = []
    for trial in range(120):
        n = int(rng.integers(1, 60))
        kind = trial % 4
        sizes = [int(x) for x in (rng.integers(4, 40, n) if kind == 0 else rng.integers(4, MAX_RECORD + 1, n) if kind == 1 else
                                  rng.choice([4, 4095, 4096, 4097, 8192, 8193, MAX_RECORD], n) if kind == 2 else rng.integers(2000, 5000, n))]
        B = (0, 4096, 8192, 65536)[trial % 4 if trial % 3 else 0]
        parts = int(rng.integers(1, 6))
        cap = int(rng.choice([0, 100, 65792, 200_000, 1 << 20, 256 << 20]))
        cases.append(dict(sizes=",".join(map(str, sizes)), cap=cap, parts=parts, B=B, count=n, num_cus=256, _sizes=sizes))
    outs = planner([{k: v for k, v in c.items() if k != "_sizes"} for c in cases])
    seen_alone = seen_all = seen_cut = 0
    for c, p in zip(cases, outs):
        sizes, B, parts, cap = c["_sizes"], c["B"], c["parts"], c["cap"]
        fixed = parts * B + 16
        rc = (max(cap - 16, 0) if not B else (cap - fixed) // 2 if cap > fixed else 0)
        assert p["record_cap"] == rc, c
        scan = np.concatenate([[0], np.cumsum(sizes)])
        want = max(1, int(np.searchsorted(scan, rc, side="right")) - 1)          # the largest k with scan[k] <= rc, at least 1
        assert p["cut"] == want and p["cut_bytes"] == scan[want], (c, p)
        seen_alone += want == 1 and scan[1] > rc
        seen_all += want == len(sizes)
        seen_cut += 1 < want < len(sizes)
        # the bound holds for the records that were cut, and a cut of more than one record stays under the cap
        image = place(sizes[:want], parts, B)
        assert image <= p["image_of_cut"], (c, image)
        if scan[want] <= rc:
            assert p["image_of_cut"] <= max(cap, 16), c
        # the plan's buffers hold any pack of the chunk
        assert p["image_max"] >= p["image_of_cut"] and p["blob_max"] >= min(255 * want, scan[want])
        assert p["workspace"] > p["image_max"] + p["blob_max"]
    assert seen_alone > 5 and seen_all > 5 and seen_cut > 5


def test_plan_sizes_do_not_wrap(planner):
    cases = [dict(count=n, cap=cap, parts=parts, B=B, approx=a, num_cus=256)
             for n, cap, parts, B, a in itertools.product([0, 1, 1 << 20, 1 << 40, (1 << 64) - 1], [0, 65792, 256 << 20, (1 << 64) - 1],
                                                          [1, 128], [0, 4096, 65536], [0, 1])]
    for c, p in zip(cases, planner(cases)):
        assert 1 <= p["plan_pack_grid"] <= 256 * 32 and 1 <= p["lane_grid"] <= 256 * 16
        assert p["image_max"] < 1 << 62 and p["workspace"] < 1 << 63, c
        nk = min(c["count"], 1 << 40)
        assert p["image_max"] >= min(nk, 1) * MAX_RECORD                              # one record always fits
