"""The kernels of the check of a database against text input
(bsdb_amd/csrc/check_kernels.hip), run on the host under ASan + UBSan without
a GPU, as tests/test_piece_host_cpu.py runs the piece-copy kernels.

tests/check_host_check.cpp includes the kernel file unchanged; the header
tests/hostwave/hip/hip_runtime.h stands in for HIP's.  The text, the image and
every descriptor array sit in an allocation of exactly their length, the status
array and the report between guard bytes.

Ground truth is Python's: the records of a text are tests/text_rule.py's, a
record's status is restated in `expected` from slices of the text and of the
image.  Valid cases are compared status by status and word by word.  Hostile
cases (a source past the image, a value past the text, lengths of 2^32 - 1,
offsets that are no scan) run only here, never on a GPU: they must leave no
sanitizer report and no dead guard byte, and a report whose sum still holds.

test_mutation: one-line edits of check_kernels.hip, each built against a copy
of the sources and each required to fail a valid case."""
import concurrent.futures
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import text_rule as R  # noqa: E402
from test_piece_host_cpu import CSRC, FLAGS, SHIM, encode, find_compiler  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "check_host_check.cpp")
U32, U64 = (1 << 32) - 1, (1 << 64) - 1
OK, REJECTED, KEY_MISMATCH, BAD_ADDR, VALUE_LEN, VALUE_BYTES = range(6)


def build(cxx, exe, csrc=CSRC):
    return subprocess.run([cxx] + FLAGS + ["-I", SHIM, "-I", csrc, "-o", exe, SRC], capture_output=True, text=True)


def run(exe, cases):
    import json
    r = subprocess.run([exe], input="".join(encode(c) + "\n" for c in cases), capture_output=True, text=True, timeout=600)
    return r.returncode, [json.loads(line) for line in r.stdout.splitlines() if line.endswith("}")], r.stderr[-3000:]


@pytest.fixture(scope="module")
def cxx():
    c = find_compiler()
    if c is None:
        pytest.skip("no clang++ on this machine (the kernel files need clang's extensions)")
    return c


@pytest.fixture(scope="module")
def exe(cxx, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("check_host") / "check_host_check")
    r = build(cxx, path)
    assert r.returncode == 0, r.stderr[-3000:]
    rc, _, err = run(path, [])
    if rc != 0:
        pytest.skip("the sanitized program does not start in this environment: " + err.strip()[-300:])
    return path


# ---- the restatement ----------------------------------------------------------------------------------------------

def expected(c):
    """(statuses, report) of a VALID case: every slice lies inside its buffer."""
    text, image, out = c["text"], c["image"], []
    for vp, vl, s, dl, st in zip(c["vpos"], c["vlen"], c["src"], c["dbvlen"], c["status"]):
        if st == OK and c.get("approx"):
            head = text[vp: vp + min(vl, 8)].ljust(8, b"\0")
            st = OK if image[8 * s: 8 * s + 8] == head else VALUE_BYTES
        elif st == OK:
            if vl != dl:
                st = VALUE_LEN
            else:
                assert vp + vl <= len(text) and s + dl <= len(image)
                st = OK if text[vp: vp + vl] == image[s: s + dl] else VALUE_BYTES
        out.append(st)
    bad = [i for i, s in enumerate(out) if s]
    rep = [len(out)] + [out.count(s) for s in range(6)] + [c.get("record_base", 0) + bad[0] if bad else U64]
    return out, rep


def case_of(records, db, sep=b" ", approx=False, tail=b"", **kw):
    """records: [(key, value)] written as text lines; db: per record (status, value the database holds).  The image
    is the database's values in a shuffled order with other bytes between them, ending with a value's last byte."""
    text = b"".join(k + sep + v + b"\n" for k, v in records) + tail
    recs, _ = R.restate(text, sep)
    assert [(k, v) for _, k, _, v in recs] == [(k, v) for k, v in records if v]
    rng = np.random.default_rng(len(records) * 7 + len(text))
    c = dict(text=text, vpos=[vp for _, _, vp, _ in recs], vlen=[len(v) for _, _, _, v in recs], status=[s for s, _ in db],
             approx=int(approx), **kw)
    if approx:
        slots = rng.permutation(len(db) + 3)[: len(db)]
        image = bytearray(rng.integers(1, 256, 8 * (len(db) + 3), dtype=np.uint8).tobytes())
        for s, (_, v) in zip(slots, db):
            image[8 * s: 8 * s + 8] = v[:8].ljust(8, b"\0")
        c.update(image=bytes(image), src=[int(s) for s in slots], dbvlen=[8] * len(db))
        return c
    image, src = bytearray(), [0] * len(db)
    for i in rng.permutation(len(db)):
        image += rng.integers(0, 256, int(rng.integers(0, 5)), dtype=np.uint8).tobytes()
        src[i] = len(image)
        image += db[i][1]
    c.update(image=bytes(image), src=src, dbvlen=[len(v) if s == OK else 0 for s, v in db])
    return c


def flip(v, j):
    return v[:j] + bytes([v[j] ^ 0x40]) + v[j + 1:]


def val(rng, n):
    """n value bytes that are neither a separator nor a line terminator."""
    return bytes(int(x) for x in rng.choice(np.array([b for b in range(33, 256)], np.uint8), n))


def valid_cases():
    rng = np.random.default_rng(2024)
    cases = []
    # every length around the 8-byte step and the 16-byte piece, the longest value; equal, then one mutation each
    lens = [1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 100, 255, 4096, 32510]
    recs = [(b"k%d" % i, val(rng, l)) for i, l in enumerate(lens * 2)]
    cases.append(dict(case_of(recs, [(OK, v) for _, v in recs]), _name="all_equal"))
    db = []
    for i, (_, v) in enumerate(recs):
        kind = i % 7
        db.append([(OK, v), (OK, flip(v, 0)), (OK, flip(v, len(v) - 1)), (OK, v[:-1]), (OK, v + b"x"), (REJECTED, b""),
                   (KEY_MISMATCH, b"")][kind] if i % 11 else (BAD_ADDR, b""))
    cases.append(dict(case_of(recs, db, record_base=1000), _name="every_class"))
    # 33-byte values, record j differs in byte j only; between every two an equal one-byte value
    recs, db = [], []
    for j in range(33):
        v = val(rng, 33)
        recs += [(b"a%d" % j, v), (b"b%d" % j, val(rng, 1))]
        db += [(OK, flip(v, j)), (OK, recs[-1][1])]
    c = case_of(recs, db)
    assert expected(c)[0] == [VALUE_BYTES, OK] * 33
    cases.append(dict(c, _name="byte_j"))
    # the longest value differing only in its last / its first byte, between equal neighbours
    big = [val(rng, 32510) for _ in range(2)]
    recs = [(b"n0", val(rng, 5)), (b"big0", big[0]), (b"n1", val(rng, 16)), (b"big1", big[1]), (b"n2", val(rng, 3))]
    db = [(OK, recs[0][1]), (OK, flip(big[0], 32509)), (OK, recs[2][1]), (OK, flip(big[1], 0)), (OK, recs[4][1])]
    cases.append(dict(case_of(recs, db), _name="longest"))
    # 40 one-byte values in a row, the 17th differing
    recs = [(b"o%d" % i, val(rng, 1)) for i in range(40)]
    cases.append(dict(case_of(recs, [(OK, flip(v, 0) if i == 16 else v) for i, (_, v) in enumerate(recs)]), _name="one_byte_run"))
    # record counts around a wave and over a workgroup; no terminator after the last line: its value ends the text
    for n in (1, 63, 64, 65, 300):
        recs = [(b"c%d" % i, val(rng, int(rng.integers(1, 40)))) for i in range(n)]
        db = [(OK, flip(v, len(v) // 2) if i % 13 == 5 else v) for i, (_, v) in enumerate(recs)]
        c = case_of(recs, db, cus=1 if n == 300 else 256)
        c["text"] = c["text"][:-1]
        cases.append(dict(c, _name=f"count_{n}"))
    cases.append(dict(text=b"", image=b"", vpos=[], vlen=[], src=[], dbvlen=[], status=[], _name="count_0"))
    # empty database values against empty descriptors, in runs and between values
    recs = [(b"e%d" % i, val(rng, 4)) for i in range(30)]
    c = case_of(recs, [(OK, flip(v, 1) if i == 17 else v) for i, (_, v) in enumerate(recs)])
    for i in range(30):
        if i % 5 != 2:                        # records 0, 1 and 29 among them: the bytes to compare start and end with none
            c["vlen"][i] = c["dbvlen"][i] = 0
    assert expected(c)[0] == [VALUE_BYTES if i == 17 else OK for i in range(30)]
    cases.append(dict(c, _name="empty_values"))
    # approximate mode: the slot against the value head
    recs = [(b"p%d" % i, val(rng, l)) for i, l in enumerate([1, 3, 7, 8, 9, 20, 8, 12, 2, 40])]
    db = [(OK, v) for _, v in recs]
    db[1], db[4], db[5], db[7], db[8] = (OK, flip(db[1][1], 2)), (OK, flip(db[4][1], 7)), (OK, flip(db[5][1], 8)), \
        (REJECTED, b""), (OK, db[8][1] + b"\x01")
    c = case_of(recs, db, approx=True, record_base=7)
    assert expected(c)[0] == [OK, VALUE_BYTES, OK, OK, VALUE_BYTES, OK, OK, REJECTED, VALUE_BYTES, OK]
    cases.append(dict(c, _name="approximate"))
    return cases


def hostile_cases():
    rng = np.random.default_rng(7)
    recs = [(b"h%d" % i, val(rng, int(l))) for i, l in enumerate(rng.integers(1, 50, 40))]
    base = case_of(recs, [(OK, v) for _, v in recs])
    n, T, I = len(recs), len(base["text"]), len(base["image"])
    out = []

    def variant(name, **kw):
        c = {k: (list(v) if isinstance(v, list) else v) for k, v in base.items()}
        for k, f in kw.items():
            c[k] = f(c[k]) if callable(f) else f
        out.append(dict(c, _name=name))

    def at(idx, vals):
        def f(lst):
            for i, v in zip(idx, vals):
                lst[i] = v
            return lst
        return f

    some = [0, 5, 17, 39]
    variant("src_past_the_image", src=at(some, [I - 1, I, I + 1, U64]))
    variant("src_wraps", src=at(some, [U64 - 3, U64 - 20, 1 << 63, I - 3]))
    variant("value_past_the_text", vpos=at(some, [T - 1, T, T + 5, U32]))
    variant("length_all_ones", vlen=at(some, [U32] * 4))
    variant("both_lengths_all_ones", vlen=at(some, [U32] * 4), dbvlen=at(some, [U32] * 4))
    variant("both_lengths_65535", vlen=at(some, [65535] * 4), dbvlen=at(some, [65535] * 4))
    variant("status_bytes_no_code", status=at(some, [4, 5, 6, 255]))
    true_coff = np.concatenate([[0], np.cumsum(base["vlen"])]).tolist()
    variant("coff_random", coff=sorted(int(x) for x in rng.integers(0, 900, n + 1)))
    variant("coff_unsorted", coff=[int(x) for x in rng.integers(0, 900, n + 1)])
    variant("coff_decreasing", coff=true_coff[::-1])
    variant("coff_total_larger", coff=true_coff[:-1] + [true_coff[-1] + 3000])
    variant("coff_all_equal", coff=[0] * n + [700])
    variant("coff_first_not_zero", coff=[x + 100 for x in true_coff])
    variant("approx_slot_past_the_image", approx=1, src=at(some, [I // 8, I // 8 + 1, U64, (1 << 61) + 1]))
    return out


# ---- the cases on the library as it is ---------------------------------------------------------------------------

def check_valid(cases, outs):
    for c, o in zip(cases, outs):
        st, rep = expected(c)
        assert o["guard"] == 1, ("guard", c["_name"])
        if o["status"] != st:
            bad = next(i for i in range(len(st)) if o["status"][i] != st[i])
            raise AssertionError((c["_name"], "record", bad, "got", o["status"][bad], "want", st[bad], c["vlen"][bad]))
        assert o["report"] == rep, (c["_name"], o["report"], rep)


def test_valid_cases(exe):
    cases = valid_cases()
    names = {c["_name"] for c in cases}
    assert {"byte_j", "longest", "one_byte_run", "empty_values", "approximate", "count_0", "count_65"} <= names
    rc, outs, err = run(exe, cases)
    assert rc == 0, err
    assert len(outs) == len(cases)
    check_valid(cases, outs)
    # every class occurs in the table
    seen = {s for c in cases for s in expected(c)[0]}
    assert seen == set(range(6))


def test_hostile_cases_leave_no_report_and_no_dead_guard(exe):
    cases = hostile_cases()
    rc, outs, err = run(exe, cases)
    assert rc == 0, err                       # no sanitizer report
    assert len(outs) == len(cases)
    for c, o in zip(cases, outs):
        assert o["guard"] == 1, ("guard", c["_name"])
        assert all(0 <= s <= 5 for s in o["status"]), c["_name"]
        rep = o["report"]
        assert rep[0] == len(c["status"]) == sum(rep[1:7]), (c["_name"], rep)
        assert rep[1:7] == [o["status"].count(s) for s in range(6)], (c["_name"], rep)
        bad = [i for i, s in enumerate(o["status"]) if s]
        assert rep[7] == (bad[0] if bad else U64), c["_name"]
    by = {c["_name"]: o for c, o in zip(cases, outs)}
    some = [0, 5, 17, 39]
    # what the header promises of such input: a length no record has is VALUE_LEN, a byte that is no code BAD_ADDR,
    # and the records the edit did not touch keep their verdict
    for name in ("length_all_ones", "both_lengths_all_ones"):
        assert [by[name]["status"][i] for i in some] == [VALUE_LEN] * 4
    assert [by["status_bytes_no_code"]["status"][i] for i in some] == [BAD_ADDR] * 4
    for name in ("src_past_the_image", "src_wraps", "value_past_the_text", "length_all_ones", "status_bytes_no_code"):
        assert all(s == OK for i, s in enumerate(by[name]["status"]) if i not in some), name
    assert all(by["approx_slot_past_the_image"]["status"][i] == VALUE_BYTES for i in some)


# ---- mutations: the harness notices a subtly wrong kernel -------------------------------------------------------

MUTATIONS = [
    ("last_step_not_masked", "low_bytes_mask(n - x < 8 ? n - x : 8)", "low_bytes_mask(8)"),
    ("run_offset_dropped", "const uint64_t at = o - start;", "const uint64_t at = 0;"),
    ("length_test_dropped", "a.vlen[r] != a.dbvlen[r] || ", ""),
    ("second_step_skipped", "for (uint32_t x = 0; x < n; x += 8) {", "for (uint32_t x = 0; x < n; x += 16) {"),
]


@pytest.fixture(scope="module")
def mutants(cxx, exe, tmp_path_factory):
    top = tmp_path_factory.mktemp("check_mutants")

    def make(m):
        name, old, new = m
        d = str(top / name)
        shutil.copytree(CSRC, d, ignore=shutil.ignore_patterns("*.o", "*.so", "*.so.*", "*.a"))
        path = os.path.join(d, "check_kernels.hip")
        text = open(path).read()
        if text.count(old) != 1:              # a refactor moved the line: the entry must follow it
            return name, None, f"check_kernels.hip: {old!r} occurs {text.count(old)} times, not once"
        with open(path, "w") as f:
            f.write(text.replace(old, new))
        r = build(cxx, os.path.join(d, "check_host_check"), d)
        return name, os.path.join(d, "check_host_check"), r.stderr[-3000:] if r.returncode else None

    with concurrent.futures.ThreadPoolExecutor(max(1, min(4, os.cpu_count() or 1))) as pool:
        return {name: (path, err) for name, path, err in pool.map(make, MUTATIONS)}


@pytest.mark.parametrize("name", [m[0] for m in MUTATIONS])
def test_mutation(mutants, name):
    """The one substitution makes a valid case fail: a wrong status, or a sanitizer report."""
    path, err = mutants[name]
    assert err is None, err
    cases = valid_cases()
    rc, outs, stderr = run(path, cases)
    if rc != 0:
        assert "Sanitizer" in stderr or "runtime error" in stderr, stderr
        return
    assert len(outs) == len(cases)
    with pytest.raises(AssertionError):
        check_valid(cases, outs)
