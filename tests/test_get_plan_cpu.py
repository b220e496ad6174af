"""The batched reader's plans (bsdb_amd/csrc/get_plan.hpp) without a GPU:
tests/get_plan_check.cpp is built with the system C++ compiler under
ASan + UBSan and run as a program of its own, as tests/test_dup_plan_cpu.py
does for the duplicate finder's plans; it prints one JSON line per case.
Asserted here: the image layout (16-byte aligned bases, file sizes up to 2^56,
128 partitions) and every grid equal the same expressions in Python's integers
(nothing wrapped, every grid in [1, 2^32)), and get_decode -- the function the
locate kernel calls -- agrees with a restatement of the reference's bit fields
(read/SyncReader.java:52, read/kv/PartitionedKVReader.java:78-82,
read/kv/BlockedKVReader.java:42-52) on valid and on out-of-range addresses."""
import itertools
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "get_plan_check.cpp")

U32 = 1 << 32
FILE_MAX = 1 << 56
PAGE = 4096
RESERVE = 256 << 20


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler on this machine")
    exe = str(tmp_path_factory.mktemp("get_plan") / "get_plan_check")
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


def with_sizes(sizes, **kw):
    c = dict(parts=len(sizes), **kw)
    c.update({f"size{p}": s for p, s in enumerate(sizes)})
    return c


def test_layout(planner):
    sets = [[0], [1], [16], [17, 0, 31], [100_003, 100_019, 99_991], [FILE_MAX], [FILE_MAX] * 128,
            [FILE_MAX - 1] * 128, list(range(1, 129)), [5_000_000_000] * 8]
    for sizes, p in zip(sets, planner([with_sizes(s) for s in sets])):
        assert p["layout_ok"] == 1
        end, base = 0, []
        for s in sizes:
            base.append(end)
            end = (end + s + 15) // 16 * 16
        assert p["base"] == base and p["total"] == end, (sizes, p)
        assert all(b % 16 == 0 for b in p["base"]) and end < 1 << 64
        assert all(b + s <= nb for b, s, nb in zip(base, sizes, base[1:] + [end]))  # partitions do not overlap
    # out of range: no partition, 129 partitions, a file over 2^56
    bad = planner([dict(parts=0), dict(parts=129), with_sizes([FILE_MAX + 1]), with_sizes([4, FILE_MAX + 1])])
    assert [p["layout_ok"] for p in bad] == [0, 0, 0, 0]


def test_open_footprint_and_chunks(planner):
    cases = [with_sizes([size] * parts, n=n, approx=a, free=fr)
             for size, parts, n, a, fr in itertools.product([0, 100_000, 5_000_000_000], [1, 8], [0, 20_000, 10**8],
                                                            [0, 1], [0, RESERVE, 1 << 30, 280 * 10**9])]
    for c, p in zip(cases, planner(cases)):
        need = (0 if c["approx"] else p["total"]) + 8 * c["n"] + 2 * 8 * 128 + 64
        assert p["open_bytes"] == need
        assert p["fits"] == int(c["free"] >= RESERVE and need <= c["free"] - RESERVE), (c, p)
    # the C2 shape (1e8 records, 8 partitions of ~0.65 GB) fits an MI355X; 128 files of 2^56 bytes do not
    assert planner([with_sizes([650_000_000] * 8, n=10**8, free=280 * 10**9)])[0]["fits"] == 1
    assert planner([with_sizes([FILE_MAX] * 128, n=10**8, free=280 * 10**9)])[0]["fits"] == 0
    chunks = [dict(batch=b, key_len=k) for b in (0, 1, 1000, 1 << 22, 1 << 40) for k in (0, 1, 13, 255)]
    for c, p in zip(chunks, planner(chunks)):
        want = c["batch"] or 1 << 22
        if c["key_len"]:
            want = min(want, max(1, (256 << 20) // c["key_len"]))
        assert p["chunk"] == max(1, want), (c, p)


def test_grids(planner):
    cases = [dict(nq=nq, value_bytes=vb, mis=mis, num_cus=cus)
             for nq, vb, mis, cus in itertools.product([0, 1, 255, 256, 257, 2_500_000, 10**12, (1 << 64) - 1],
                                                       [0, 1, 15, 16, 17, 125_535, 10**13, (1 << 64) - 1],
                                                       [0, 5, 15], [1, 256, 304])]
    for c, p in zip(cases, planner(cases)):
        assert 1 <= p["locate_grid"] < U32 and 1 <= p["gather_grid"] < U32, (c, p)
        assert p["locate_grid"] == max(1, min(-(-c["nq"] // 256), c["num_cus"] * 16))
        pieces = -(-(c["value_bytes"] + c["mis"]) // 16) if c["value_bytes"] else 0
        assert p["pieces"] == pieces, (c, p)
        assert p["gather_grid"] == max(1, min(-(-pieces // 256), c["num_cus"] * 32))


def decode(addr, fmt, sizes, parts):
    """The reference's bit fields, and the header's bounds rule for the 3-byte record header."""
    if addr >> 63:                                   # SyncReader.java:52: addr < 0 is null
        return None
    part = addr >> 56                                # PartitionedKVReader.java:79
    if part >= parts:
        return None
    if fmt == 0:
        pos, limit = addr & (FILE_MAX - 1), sizes[part]  # PartitionedKVReader.java:80
    else:
        block = ((addr >> 16) & 0xFFFFFFFF) * PAGE   # BlockedKVReader.java:42-44
        bsize = ((addr >> 48) & 0xFF) * PAGE         # :46-48
        rec = addr & 0xFFFF                          # :50-52
        if bsize == 0 or block + bsize > sizes[part] or rec >= bsize:
            return None
        pos, limit = block + rec, block + bsize
    return (part, pos, limit) if pos + 3 <= limit else None


def check_decode(planner, cases):
    """cases: (addr, fmt, sizes, partitions the decode sees)."""
    out = planner([with_sizes(s, addr=a, format=f, dparts=dp) for a, f, s, dp in cases])
    for (a, f, s, dp), p in zip(cases, out):
        want = decode(a, f, s, dp)
        assert p["ok"] == int(want is not None), (hex(a), f, s, dp, p)
        if want:
            assert (p["part"], p["pos"], p["limit"]) == want, (hex(a), f, s, dp, p)
            assert p["pos"] + 3 <= p["limit"] <= s[p["part"]]
    return out


def test_decode_compact(planner):
    sizes = [1000, 100_003, 5, 2, 0, FILE_MAX]
    cases = []
    for part, size in enumerate(sizes):
        for off in {0, 1, 2, 3, size // 2, max(size - 4, 0), max(size - 3, 0), max(size - 2, 0), max(size - 1, 0), size,
                    size + 1, FILE_MAX - 4, FILE_MAX - 3, FILE_MAX - 2, FILE_MAX - 1}:
            if off < FILE_MAX:
                cases.append((part << 56 | off, 0, sizes, len(sizes)))
    out = check_decode(planner, cases)
    assert sum(p["ok"] for p in out) > 10 and sum(1 - p["ok"] for p in out) > 10
    # the named edges: a whole header at size - 3; the header crosses the end at size - 2, size - 1; offset = size
    edge = check_decode(planner, [(o, 0, [1000], 1) for o in (997, 998, 999, 1000)])
    assert [p["ok"] for p in edge] == [1, 0, 0, 0]
    # top bit set; partition = partitions; partition = 127 (seen by a 3-partition and by a 128-partition database)
    big = [1000] * 128
    cases = [(1 << 63 | 10, 0, big, 128), ((1 << 64) - 1, 0, big, 128), (3 << 56 | 10, 0, big, 3), (2 << 56 | 10, 0, big, 3),
             (127 << 56 | 10, 0, big, 3), (127 << 56 | 10, 0, big, 128), (127 << 56 | 998, 0, big, 128)]
    assert [p["ok"] for p in check_decode(planner, cases)] == [0, 0, 0, 1, 0, 1, 0]
    # an offset near 2^56 - 1 against a small file and against a full-size one
    near = [(FILE_MAX - 1, 0, [1000], 1), (FILE_MAX - 3, 0, [FILE_MAX], 1), (FILE_MAX - 2, 0, [FILE_MAX], 1)]
    assert [p["ok"] for p in check_decode(planner, near)] == [0, 1, 0]


def test_decode_blocked(planner):
    def addr(part, pages, page_pos, rec):
        return part << 56 | pages << 48 | page_pos << 16 | rec

    sizes = [10 * PAGE, 3 * PAGE + 100, 0, 255 * PAGE]
    cases = [(addr(p, pages, pos, rec), 1, sizes, len(sizes))
             for p, pages, pos, rec in itertools.product(range(4), [0, 1, 2, 17, 255], [0, 1, 2, 8, 9, 10, 0xFFFFFFFF],
                                                         [0, 1, 4092, 4093, 4094, 4095, 4096, 8189, 8190, 0xFFFF])]
    out = check_decode(planner, cases)
    assert sum(p["ok"] for p in out) > 20 and sum(1 - p["ok"] for p in out) > 20
    one = [10 * PAGE]
    named = [
        (addr(0, 1, 3, 100), 1),          # a valid record in a one-page block
        (addr(0, 0, 3, 100), 0),          # block count 0
        (addr(0, 2, 8, 0), 1),            # block end = file size
        (addr(0, 2, 9, 0), 0),            # block end > file size
        (addr(0, 1, 10, 0), 0),           # block starts at the file's end
        (addr(0, 1, 3, 4096), 0),         # record offset = block size
        (addr(0, 1, 3, 0xFFFF), 0),       # record offset > block size
        (addr(0, 1, 3, 4093), 1),         # the header ends at the block's end
        (addr(0, 1, 3, 4094), 0),         # the header crosses the block's end
        (addr(0, 255, 0xFFFFFFFF, 0), 0),  # the largest block at the largest position: nothing wraps
        (1 << 63 | addr(0, 1, 3, 100), 0),  # top bit set
        (addr(1, 1, 3, 100), 0),          # partition = partitions
    ]
    got = check_decode(planner, [(a, 1, one, 1) for a, _ in named])
    assert [p["ok"] for p in got] == [w for _, w in named]
    # the largest position inside a file that holds it (2^32 - 1 pages and one block more: below 2^56)
    huge = [(0xFFFFFFFF + 255) * PAGE]
    assert [p["ok"] for p in check_decode(planner, [(addr(0, 255, 0xFFFFFFFF, 5), 1, huge, 1)])] == [1]
