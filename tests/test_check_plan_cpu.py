"""The plans of the check of a database against text input
(bsdb_amd/csrc/check_plan.hpp) without a GPU: tests/check_plan_check.cpp is
built with the system C++ compiler under ASan + UBSan and run as a program of
its own, as tests/test_get_plan_cpu.py does for the reader's plans.  Asserted
here: a chunk's footprint equals a restatement in Python's integers (the text
and the split's workspace at the worst case, the descriptors, the key blob with
its offsets and the pack's size arrays, 25 bytes a record for src, dbvlen,
status, cmp_len and coff), nothing wraps, the chunk size is the largest halving
that fits half of the free memory, and every grid lies in [1, 2^32)."""
import itertools
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "check_plan_check.cpp")
U32 = 1 << 32
MIN_CHUNK, DEFAULT_CHUNK, MAX_CHUNK = 64 << 10, 256 << 20, (U32 - 1) & ~15


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler on this machine")
    exe = str(tmp_path_factory.mktemp("check_plan") / "check_plan_check")
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


def footprint(b):
    """The restatement: device bytes of a chunk of b text bytes."""
    r = b // 4 + 1                                   # the most records
    nb = max(1, -(-b // 4096))                       # workgroups of the count kernel
    lines = seps = b                                 # the worst case: every byte a line and a separator
    split_ws = 2 * 4 * nb + 2 * 8 * (nb + 1) + 4 * lines + 4 * (seps + 1) + 4 * lines + 8 * (lines + 1)
    split = b + 16 + split_ws + 4 * 4 * r            # the text, the workspace, four u32 descriptors a record
    blob = (b + 16) + 8 * (r + 1) + 2 * 4 * r + 8 * (r + 1)   # keys, offsets, two size arrays, the size scan
    check = 25 * r + 8                               # src 8 + dbvlen 4 + status 1 + cmp_len 4 + coff 8; coff's last entry
    return split, blob, check, split + blob + check


def chunk(requested, free):
    c = min(max(requested or DEFAULT_CHUNK, MIN_CHUNK), MAX_CHUNK)
    while c > MIN_CHUNK and footprint(c)[3] > free // 2:
        c = max(MIN_CHUNK, c // 2)
    return c


def test_constants(planner):
    p = planner([dict(bytes=0)])[0]
    assert (p["words"], p["value_len"], p["value_bytes"], p["record_bytes"], p["max_value"]) == (8, 4, 5, 25, 65535)


def test_footprint(planner):
    sizes = [0, 1, 3, 4, 15, 16, 4095, 4096, 4097, MIN_CHUNK, 10**6 + 7, DEFAULT_CHUNK, MAX_CHUNK, U32 - 1]
    for b, p in zip(sizes, planner([dict(bytes=b) for b in sizes])):
        assert (p["split"], p["blob"], p["check"], p["total"]) == footprint(b), (b, p)
        assert p["total"] < 1 << 40
    # the largest chunk: about 38 bytes of device memory a text byte (20 of them the split's worst case)
    assert 35 * MAX_CHUNK < footprint(MAX_CHUNK)[3] < 42 * MAX_CHUNK


def test_chunk_size(planner):
    image = 5 * 10**9                                # a resident image: the free figures below lie on either side of it
    frees = [0, 1, MIN_CHUNK, 1 << 20, 100 << 20, image - 1, image, 2 * footprint(DEFAULT_CHUNK)[3] - 1,
             2 * footprint(DEFAULT_CHUNK)[3], 280 * 10**9, (1 << 64) - 1]
    reqs = [0, 1, MIN_CHUNK - 1, MIN_CHUNK, MIN_CHUNK + 1, 1 << 20, DEFAULT_CHUNK, MAX_CHUNK, U32, 1 << 40]
    cases = [dict(requested=r, free=f) for r, f in itertools.product(reqs, frees)]
    for c, p in zip(cases, planner(cases)):
        want = chunk(c["requested"], c["free"])
        assert p["chunk"] == want, (c, p)
        assert MIN_CHUNK <= p["chunk"] <= MAX_CHUNK
        assert p["chunk"] == MIN_CHUNK or footprint(p["chunk"])[3] <= c["free"] // 2
    # a free-memory figure smaller than the image (and smaller than any chunk's footprint): the smallest chunk
    assert planner([dict(requested=0, free=1 << 20)])[0]["chunk"] == MIN_CHUNK
    # the default chunk fits an MI355X beside a 5 GB image; 64 KiB asked for stays 64 KiB
    assert planner([dict(requested=0, free=288 * 10**9 - image)])[0]["chunk"] == DEFAULT_CHUNK
    assert planner([dict(requested=MIN_CHUNK, free=280 * 10**9)])[0]["chunk"] == MIN_CHUNK


def test_grids(planner):
    cases = [dict(bytes=b, count=n, num_cus=cus)
             for b, n, cus in itertools.product([0, 1, 15, 16, 17, 4096, 10**6, MAX_CHUNK, U32 - 1],
                                                [0, 1, 255, 256, 257, 10**7, 1 << 30], [1, 256, 304])]
    for c, p in zip(cases, planner(cases)):
        assert 1 <= p["lane_grid"] < U32 and 1 <= p["values_grid"] < U32
        assert p["lane_grid"] == max(1, min(-(-c["count"] // 256), c["num_cus"] * 16))
        pieces = -(-c["bytes"] // 16)
        assert p["values_grid"] == max(1, min(-(-pieces // 256), c["num_cus"] * 32))
