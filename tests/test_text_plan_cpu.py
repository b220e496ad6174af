"""The text front end's plans (bsdb_amd/csrc/text_plan.hpp) without a GPU:
tests/text_plan_check.cpp is built with the system C++ compiler under
ASan + UBSan and run as a program of its own, exactly as
tests/test_get_plan_cpu.py builds its checker; it prints one JSON line per
case.  Asserted here: the record bound, every grid and the footprint equal the
same expressions in Python's integers (nothing wrapped, every grid in
[1, 2^32)), the run bounds of the partition rule, the cut of a file buffer on
each way a buffer can end, and text_verdict -- the function the records kernel
calls -- against the byte-walking restatement of the rule (tests/text_rule.py:
split at the separator, drop trailing empty fields) on the issue's table and on
seeded random lines over the alphabet {a, separator}."""
import itertools
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import text_rule as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "text_plan_check.cpp")

U32 = 1 << 32
SIZES = [0, 1, 15, 16, 17, U32 - 1]
VERDICTS = {0: "records", 1: "not_two_fields", 2: "empty_key", 3: "too_large"}


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler on this machine")
    exe = str(tmp_path_factory.mktemp("text_plan") / "text_plan_check")
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
        lines = [" ".join(f"{k}={v if isinstance(v, str) else int(v)}" for k, v in c.items()) for c in cases]
        r = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        out = [json.loads(line) for line in r.stdout.splitlines()]
        assert len(out) == len(cases)
        return out

    return plans


def footprint(b, lines, seps, approx):
    nb = max(1, -(-b // 4096))
    r = b // 4 + 1
    split = 2 * 4 * nb + 2 * 8 * (nb + 1) + 4 * lines + 4 * (seps + 1) + 4 * lines + 8 * (lines + 1)
    pack = (4 * 4 * r + 2 * 4 * r + 2 * 8 * (r + 1) + (b + b // 2 + 16) + (b + 16) + 8 * (r + 1) + 8 * r
            + (9 * r if approx else 0))
    return split, pack, b + 16 + split + pack


def test_grids_and_footprints(planner):
    cases = [dict(bytes=b, lines=min(b, l), seps=min(b, s), approx=a, items=it, out_bytes=ob, mis=mis, num_cus=cus)
             for b, (l, s), a, (it, ob, mis), cus in itertools.product(
                 SIZES, [(0, 0), (1, 1), (U32, U32), (1000, 5)], [0, 1],
                 [(0, 0, 0), (1, 1, 15), (255, 15, 1), (256, 16, 0), (257, 17, 15), (U32 - 1, U32 - 1, 5),
                  (1 << 30, 3 * (U32 - 1) // 2 + 16, 15)], [1, 256, 304])]
    for c, p in zip(cases, planner(cases)):
        b = c["bytes"]
        assert p["max_records"] == b // 4 + 1
        assert p["blocks"] == -(-b // 4096)
        assert p["count_grid"] == max(1, -(-b // 4096)) and 1 <= p["count_grid"] < U32
        assert p["lane_grid"] == max(1, min(-(-c["items"] // 256), c["num_cus"] * 16)) and 1 <= p["lane_grid"] < U32
        pieces = -(-(c["out_bytes"] + c["mis"]) // 16) if c["out_bytes"] else 0
        assert p["pieces"] == pieces, (c, p)
        assert p["pack_grid"] == max(1, min(-(-pieces // 256), c["num_cus"] * 32)) and 1 <= p["pack_grid"] < U32
        assert p["image_max"] == b + b // 2 + 16 and p["blob_max"] == b + 16
        assert (p["fp_split"], p["fp_pack"], p["fp_total"]) == footprint(b, c["lines"], c["seps"], c["approx"]), (c, p)
        assert p["fp_total"] < 1 << 40
        # the bounds the footprint rests on: a record is its text plus one byte (two without a terminator)
        assert p["image_max"] >= b + p["max_records"] + 1 or b < 4
        assert p["image_max"] <= 3 * b // 2 + 16


def test_image_bound_on_the_densest_records():
    """"a b\\n" repeated is the text with the most records per byte: the image bound and the record bound hold."""
    for n, tail in itertools.product([1, 2, 7], [b"\n", b""]):
        text = b"a b\n" * (n - 1) + b"a b" + tail
        recs, rep = R.restate(text, b" ")
        assert rep["records"] == n <= len(text) // 4 + 1
        assert len(R.image_of(recs)[0]) == 5 * n <= len(text) + len(text) // 2 + 16


def test_chunk_size(planner):
    MIN, DEF = 64 << 10, 256 << 20
    cases = [dict(requested=r, free=f) for r in (0, 1, MIN - 1, MIN, MIN + 1, 1 << 20, DEF, 1 << 31, U32, 1 << 40)
             for f in (0, 1 << 20, 1 << 30, 64 << 30, 280 * 10**9)]
    for c, p in zip(cases, planner(cases)):
        want = c["requested"] or DEF
        want = min(max(want, MIN), (U32 - 1) & ~15)
        while want > MIN and footprint(want, want, want, 1)[2] > c["free"] // 2:
            want = max(MIN, want // 2)
        assert p["chunk"] == want, (c, p)
        assert MIN <= p["chunk"] < U32
    # the default chunk fits an MI355X as it is
    assert planner([dict(requested=0, free=280 * 10**9)])[0]["chunk"] == DEF


def test_run_bounds(planner):
    cases = [dict(k=k, parts=P) for P in (1, 3, 8, 128) for k in (0, 1, 5, P - 1, P, P + 1, 20_000, 1 << 30)]
    for c, p in zip(cases, planner(cases)):
        k, P = c["k"], c["parts"]
        assert p["bound"] == R.run_bounds(k, P), (c, p)
        assert p["bound"][0] == 0 and p["bound"][-1] == k
        sizes = np.diff(p["bound"])
        assert sizes.min() >= 0 and sizes.max() - sizes.min() <= 1      # contiguous, balanced
    named = planner([dict(k=5, parts=8), dict(k=8, parts=8), dict(k=0, parts=8)])
    assert named[0]["bound"] == [0, 0, 1, 1, 2, 3, 3, 4, 5]               # k < P: some runs are empty
    assert named[1]["bound"] == list(range(9))                            # k = P: one record each
    assert named[2]["bound"] == [0] * 9                                   # k = 0


def cut_restated(buf: bytes, eof: bool) -> int:
    """The largest prefix that is whole lines by splitlines: a prefix ends a line iff
    appending a byte starts a new line (or the file ends with it)."""
    if eof:
        return len(buf)
    for i in range(len(buf), 0, -1):
        head = buf[:i]
        if head[-1:] == b"\n":
            return i
        # a '\r' ends its line only when the next byte is known and is no '\n'
        if head[-1:] == b"\r" and i < len(buf) and buf[i:i + 1] != b"\n":
            return i
    return 0


def test_cut(planner):
    named = [
        (b"ab c\nde f\n", 0, 10),          # ends in \n
        (b"ab c\nde f\r", 0, 5),           # ends in \r: it may be half of \r\n -> never a cut point
        (b"ab c\nde f\r", 1, 10),          # \r + EOF
        (b"ab c\rde f\r\n", 0, 11),        # \r then \n as the next byte: cut after the \n
        (b"ab c\r\nde f\r", 0, 6),         #   ... and with the \n of a pair before a last bare \r
        (b"ab c\nde f", 0, 5),             # no terminator at the end
        (b"ab c\nde f", 1, 9),             # no terminator + EOF
        (b"ab c de f", 0, 0),              # a full buffer without a line end
        (b"ab c\rde f", 0, 5),             # a \r whose next byte is present and no \n
        (b"\r", 0, 0), (b"\r", 1, 1), (b"\n", 0, 1), (b"", 0, 0), (b"", 1, 0), (b"\r\r", 0, 1), (b"\r\n", 0, 2),
    ]
    got = planner([dict(buf=b.hex() or "", eof=e) for b, e, _ in named])
    assert [p["cut"] for p in got] == [w for _, _, w in named]
    rng = np.random.default_rng(5)
    rand = [(bytes(rng.choice(list(b"a \r\n"), int(rng.integers(0, 12)), p=[0.4, 0.2, 0.2, 0.2]).astype(np.uint8)),
             int(rng.integers(0, 2))) for _ in range(2000)]
    got = planner([dict(buf=b.hex(), eof=e) for b, e in rand])
    for (b, e), p in zip(rand, got):
        assert p["cut"] == cut_restated(b, bool(e)), (b, e, p)
        # what is cut off is whole lines: the lines of the two parts are the lines of the whole
        if not e and p["cut"]:
            assert b[:p["cut"]].splitlines() + b[p["cut"]:].splitlines() == b.splitlines()


TABLE = [("a b", "records"), ("a b ", "records"), ("a b  ", "records"), ("a  b", "not_two_fields"),
         (" a b", "not_two_fields"), ("a b c", "not_two_fields"), ("a ", "not_two_fields"), ("a", "not_two_fields"),
         ("", "not_two_fields"), (" ", "not_two_fields"), (" b", "empty_key")]


def check_verdicts(planner, lines, sep: bytes):
    out = planner([dict(line=l.hex(), sep=sep[0]) for l in lines])
    for l, p in zip(lines, out):
        cls, k, v = R.verdict(l, sep)
        assert VERDICTS[p["verdict"]] == cls, (l, p)
        if cls == "records":
            assert l[p["kpos"]:p["kpos"] + p["klen"]] == k and l[p["vpos"]:p["vpos"] + p["vlen"]] == v, (l, p)
    return out


def test_verdict_table(planner):
    for sep in (b" ", b"\t", b","):
        lines = [t.replace(" ", sep.decode()).encode() for t, _ in TABLE]
        out = check_verdicts(planner, lines, sep)
        assert [VERDICTS[p["verdict"]] for p in out] == [w for _, w in TABLE]
    # the value after trailing separators are dropped
    p = planner([dict(line=b"a b  ".hex(), sep=32)])[0]
    assert (p["kpos"], p["klen"], p["vpos"], p["vlen"]) == (0, 1, 2, 1)


def test_verdict_sizes(planner):
    lines = [b"k" * kl + b" " + b"v" * vl + tail for kl in (1, 254, 255, 256, 300) for vl in (1, 32509, 32510, 32511)
             for tail in (b"", b"  ")]
    out = check_verdicts(planner, lines, b" ")
    assert {VERDICTS[p["verdict"]] for p in out} == {"records", "too_large"}


def test_verdict_random(planner):
    rng = np.random.default_rng(17)
    lines = [bytes(rng.choice([97, 32], int(rng.integers(0, 10)), p=[0.6, 0.4]).astype(np.uint8)) for _ in range(4000)]
    out = check_verdicts(planner, lines, b" ")
    seen = {VERDICTS[p["verdict"]] for p in out}
    assert seen == {"records", "not_two_fields", "empty_key"}


def test_separator_rule(planner):
    out = planner([dict(sep=s) for s in (32, 9, 44, 0, 1, 127, 128, 255, 10, 13)])
    assert [p["bad_sep"] for p in out] == [0, 0, 0, 0, 0, 0, 1, 1, 1, 1]
