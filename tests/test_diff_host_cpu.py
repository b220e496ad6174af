"""The kernels of the diff of two resident databases
(bsdb_amd/csrc/diff_kernels.hip), run on the host under ASan + UBSan without a
GPU, as tests/test_check_host_cpu.py runs the check's.

tests/diff_host_check.cpp includes the kernel file unchanged; the header
tests/hostwave/hip/hip_runtime.h stands in for HIP's.  Both images and every
descriptor array sit in an allocation of exactly their length, the status
array, the report and the selection's outputs between guard bytes.  The
program is started as a child process: nothing sanitized is loaded into Python.

Ground truth is Python's: a record's status is restated in `expected` from
slices of the two images, a selection in `selected` as a filter.  Valid cases
are compared status by status and word by word.  Hostile cases (positions past
either image, positions that wrap, lengths of 2^32 - 1, status bytes that are no
code, offsets that are no scan) run only here, never on a GPU: they must leave
no sanitizer report and no dead guard byte, and a report whose sum still holds.

test_mutation: one-line edits of diff_kernels.hip, each built against a copy
of the sources and each required to fail a valid case."""
import concurrent.futures
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_piece_host_cpu import CSRC, FLAGS, SHIM, encode, find_compiler  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "diff_host_check.cpp")
U32, U64 = (1 << 32) - 1, (1 << 64) - 1
SAME, REJECTED, KEY_MISMATCH, BAD_ADDR, VALUE_LEN, VALUE_BYTES, BAD_SLOT = range(7)
SCAN_OK, SCAN_BAD_ADDR, SCAN_NOT_TEXT = 0, 1, 2
LENS = [1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 100, 255, 4096, 65535]


def build(cxx, exe, csrc=CSRC):
    return subprocess.run([cxx] + FLAGS + ["-I", SHIM, "-I", csrc, "-o", exe, SRC], capture_output=True, text=True)


def run(exe, cases):
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
    path = str(tmp_path_factory.mktemp("diff_host") / "diff_host_check")
    r = build(cxx, path)
    assert r.returncode == 0, r.stderr[-3000:]
    rc, _, err = run(path, [])
    if rc != 0:
        pytest.skip("the sanitized program does not start in this environment: " + err.strip()[-300:])
    return path


# ---- the restatement ----------------------------------------------------------------------------------------------

def expected(c):
    """(statuses, report) of a VALID diff case: every slice lies inside its image."""
    ia, ib, out, compared = c["image_a"], c["image_b"], [], 0
    for sa, va, la, sb, lb, st in zip(c["status_a"], c["vsrc_a"], c["vlen_a"], c["src_b"], c["vlen_b"], c["status"]):
        if sa == SCAN_BAD_ADDR:
            st = BAD_SLOT
        elif st == SAME:
            if la != lb:
                st = VALUE_LEN
            else:
                assert va + la <= len(ia) and sb + lb <= len(ib)
                compared += la
                st = SAME if ia[va: va + la] == ib[sb: sb + lb] else VALUE_BYTES
        out.append(st)
    diff = [i for i, s in enumerate(out) if s]
    rep = [len(out)] + [out.count(s) for s in range(7)] + [c.get("slot_base", 0) + diff[0] if diff else U64, compared]
    return out, rep


def selected(c):
    return [i for i, s in enumerate(c["status"]) if s < BAD_SLOT and c["mask"] >> s & 1]


def case_of(recs, pad_a=0, pad_b=0, **kw):
    """recs: per slot of A a dict: a = the value A holds (None: the slot names no record), st = locate's status in B,
    b = the value B holds (FOUND only), oa / ob = where the value starts, mod 16 (None: wherever it falls).  Each
    image is its side's values in a shuffled order of its own with other bytes between them, after pad_* bytes."""
    rng = np.random.default_rng(len(recs) * 11 + pad_a + 3 * pad_b)
    n = len(recs)

    def image(vals, offs, pad, seed):
        r = np.random.default_rng(seed)
        img, pos = bytearray(r.integers(0, 256, pad, dtype=np.uint8).tobytes()), [0] * n
        for i in r.permutation(n):
            img += r.integers(0, 256, int(r.integers(0, 5)), dtype=np.uint8).tobytes()
            if offs[i] is not None:
                img += r.integers(0, 256, (offs[i] - len(img)) % 16, dtype=np.uint8).tobytes()
            pos[i] = len(img)
            img += vals[i]
        return bytes(img), pos

    va = [r["a"] if r["a"] is not None else b"" for r in recs]
    vb = [r.get("b", b"") if r["st"] == SAME else b"" for r in recs]
    image_a, vsrc_a = image(va, [r.get("oa") for r in recs], pad_a, int(rng.integers(1 << 30)))
    image_b, src_b = image(vb, [r.get("ob") for r in recs], pad_b, int(rng.integers(1 << 30)))
    return dict(image_a=image_a, image_b=image_b, status_a=[SCAN_BAD_ADDR if r["a"] is None else SCAN_OK for r in recs],
                vsrc_a=[0 if r["a"] is None else p for r, p in zip(recs, vsrc_a)], vlen_a=[len(v) for v in va],
                src_b=[p if r["st"] == SAME else 0 for r, p in zip(recs, src_b)], vlen_b=[len(v) for v in vb],
                status=[r["st"] for r in recs], **kw)


def flip(v, j):
    return v[:j] + bytes([v[j] ^ 0x40]) + v[j + 1:]


def val(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def same(v):
    return dict(a=v, st=SAME, b=v)


def valid_cases():
    rng = np.random.default_rng(2025)
    cases = []
    # every length around the 8-byte step and the 16-byte piece, the longest value a header holds; equal on both sides
    vals = [val(rng, l) for l in LENS * 2]
    cases.append(dict(case_of([same(v) for v in vals]), _name="all_equal"))
    # the same lengths with one flip each at the first and at the last byte, and the lengths +-1
    recs = []
    for v in vals[: len(LENS)]:
        recs += [dict(a=v, st=SAME, b=flip(v, 0)), same(v), dict(a=v, st=SAME, b=flip(v, len(v) - 1)),
                 dict(a=v, st=SAME, b=v[:-1]), dict(a=v, st=SAME, b=v + b"x")]
    c = case_of(recs)
    assert expected(c)[0] == [VALUE_BYTES, SAME, VALUE_BYTES, VALUE_LEN, VALUE_LEN] * len(LENS)
    cases.append(dict(c, _name="flips_and_lengths"))
    # 33-byte values, record j differs in byte j only; between every two an equal one-byte value
    recs = []
    for j in range(33):
        v = val(rng, 33)
        recs += [dict(a=v, st=SAME, b=flip(v, j)), same(val(rng, 1))]
    c = case_of(recs)
    assert expected(c)[0] == [VALUE_BYTES, SAME] * 33
    cases.append(dict(c, _name="byte_j"))
    # 40 one-byte values in a row, the 17th differing
    vals1 = [val(rng, 1) for _ in range(40)]
    cases.append(dict(case_of([dict(a=v, st=SAME, b=flip(v, 0) if i == 16 else v) for i, v in enumerate(vals1)]), _name="one_byte_run"))
    # empty values on both sides: at the start, at the end and in runs
    recs = [same(val(rng, 4)) if i % 5 == 2 else same(b"") for i in range(30)]
    recs[17] = dict(a=recs[17]["a"], st=SAME, b=flip(recs[17]["a"], 1))
    c = case_of(recs)
    assert expected(c)[0] == [VALUE_BYTES if i == 17 else SAME for i in range(30)] and c["vlen_a"][0] == c["vlen_a"][29] == 0
    cases.append(dict(c, _name="empty_values"))
    cases.append(dict(case_of([same(b"")] * 5), _name="only_empty_values"))
    # record counts around a wave and over a workgroup, on one CU
    for n in (1, 63, 64, 65, 300):
        vs = [val(rng, int(rng.integers(1, 40))) for _ in range(n)]
        recs = [dict(a=v, st=SAME, b=flip(v, len(v) // 2) if i % 13 == 5 else v) for i, v in enumerate(vs)]
        cases.append(dict(case_of(recs, cus=1), _name=f"count_{n}"))
    cases.append(dict(image_a=b"", image_b=b"", status_a=[], vsrc_a=[], vlen_a=[], src_b=[], vlen_b=[], status=[], _name="count_0"))
    # every status class, with a slot base
    recs = []
    for i in range(90):
        v = val(rng, int(rng.integers(1, 60)))
        recs.append([same(v), dict(a=v, st=SAME, b=flip(v, len(v) - 1)), dict(a=v, st=SAME, b=v + v[:1]), dict(a=v, st=REJECTED),
                     dict(a=v, st=KEY_MISMATCH), dict(a=v, st=BAD_ADDR), dict(a=None, st=(SAME, REJECTED, KEY_MISMATCH)[i % 3]),
                     same(v), same(v)][i % 9])
    c = case_of(recs, slot_base=5_000_000_000)
    assert set(expected(c)[0]) == set(range(7)) and expected(c)[1][8] == 5_000_000_001
    cases.append(dict(c, _name="every_class"))
    # the same value at every misalignment on either side, the images of different lengths: A the longer, then B
    v33 = [val(rng, 33) for _ in range(256)]
    recs = [dict(a=v, st=SAME, b=flip(v, 32) if i % 17 == 3 else v, oa=i // 16, ob=i % 16) for i, v in enumerate(v33)]
    for name, pa, pb in (("misaligned_a_longer", 20_011, 0), ("misaligned_b_longer", 5, 30_002)):
        c = case_of(recs, pad_a=pa, pad_b=pb)
        assert {(a % 16, b % 16) for a, b in zip(c["vsrc_a"], c["src_b"])} == {(i, j) for i in range(16) for j in range(16)}
        assert min(c["vsrc_a"]) > len(c["image_b"]) if pa > pb else min(c["src_b"]) > len(c["image_a"])
        cases.append(dict(c, _name=name))
    return cases


def select_cases():
    rng = np.random.default_rng(99)
    cases = []
    for n in (0, 1, 64, 65, 300):
        status = [int(s) for s in rng.integers(0, 7, n)]
        desc = dict(ksrc=[int(x) for x in rng.integers(0, 1 << 62, n)], klen=[int(x) for x in rng.integers(0, 256, n)],
                    vsrc=[int(x) for x in rng.integers(0, 1 << 62, n)], vlen=[int(x) for x in rng.integers(0, 65536, n)])
        for name, mask, st in [("none", 0, status), ("all", 0x3F, status), ("upsert", 0x36, status)] + \
                [(f"class_{k}", 1 << k, status) for k in range(6)] + [("alternating", 2, [i % 2 for i in range(n)])]:
            cases.append(dict(op="select", status=st, mask=mask, cus=1 if n == 300 else 256, **desc, _name=f"{name}_{n}"))
    return cases


def hostile_cases():
    rng = np.random.default_rng(7)
    base = case_of([same(val(rng, int(l))) for l in rng.integers(1, 50, 40)])
    n, A, B = 40, len(base["image_a"]), len(base["image_b"])
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
    variant("a_past_its_image", vsrc_a=at(some, [A - 1, A, A + 1, U64]))
    variant("b_past_its_image", src_b=at(some, [B - 1, B, B + 1, U64]))
    variant("a_wraps", vsrc_a=at(some, [U64 - 3, U64 - 20, 1 << 63, A - 3]))
    variant("b_wraps", src_b=at(some, [U64 - 3, U64 - 20, 1 << 63, B - 3]))
    variant("a_length_all_ones", vlen_a=at(some, [U32] * 4))
    variant("b_length_all_ones", vlen_b=at(some, [U32] * 4))
    variant("both_lengths_all_ones", vlen_a=at(some, [U32] * 4), vlen_b=at(some, [U32] * 4))
    variant("both_lengths_65535", vlen_a=at(some, [65535] * 4), vlen_b=at(some, [65535] * 4))
    variant("status_bytes_no_code", status=at(some, [4, 5, 6, 255]))
    variant("scan_status_bytes_no_code", status_a=at(some, [3, 7, 255, SCAN_NOT_TEXT]))
    true_coff = np.concatenate([[0], np.cumsum(base["vlen_a"])]).tolist()
    mixed = at(range(0, n, 3), [REJECTED, KEY_MISMATCH, BAD_ADDR] * n)   # offsets that are no scan over records that are not FOUND
    variant("coff_random", coff=sorted(int(x) for x in rng.integers(0, 900, n + 1)), status=mixed)
    variant("coff_unsorted", coff=[int(x) for x in rng.integers(0, 900, n + 1)], status=mixed)
    variant("coff_decreasing", coff=true_coff[::-1])
    variant("coff_total_larger", coff=true_coff[:-1] + [true_coff[-1] + 3000])
    variant("coff_all_equal", coff=[0] * n + [700], status=mixed)
    variant("coff_first_not_zero", coff=[x + 100 for x in true_coff])
    return out


# ---- the cases on the library as it is ---------------------------------------------------------------------------

def check_valid(cases, outs):
    for c, o in zip(cases, outs):
        st, rep = expected(c)
        assert o["guard"] == 1, ("guard", c["_name"])
        if o["status"] != st:
            bad = next(i for i in range(len(st)) if o["status"][i] != st[i])
            raise AssertionError((c["_name"], "record", bad, "got", o["status"][bad], "want", st[bad], c["vlen_a"][bad]))
        assert o["report"] == rep, (c["_name"], o["report"], rep)


def test_valid_cases(exe):
    cases = valid_cases()
    names = {c["_name"] for c in cases}
    assert {"byte_j", "one_byte_run", "empty_values", "count_0", "count_65", "count_300", "misaligned_a_longer"} <= names
    rc, outs, err = run(exe, cases)
    assert rc == 0, err
    assert len(outs) == len(cases)
    check_valid(cases, outs)
    assert {s for c in cases for s in expected(c)[0]} == set(range(7))   # every class occurs in the table


def test_select_cases(exe):
    cases = select_cases()
    rc, outs, err = run(exe, cases)
    assert rc == 0, err
    assert len(outs) == len(cases)
    for c, o in zip(cases, outs):
        want = selected(c)
        assert o["guard"] == 1, ("guard", c["_name"])
        assert o["nsel"] == len(want) and o["sel"] == want, c["_name"]          # order and nsel exact
        for k in ("ksrc", "klen", "vsrc", "vlen"):
            assert o[k] == [c[k][i] for i in want], (c["_name"], k)
    by = {c["_name"]: o for c, o in zip(cases, outs)}
    assert by["none_300"]["nsel"] == 0 and by["alternating_300"]["sel"] == list(range(1, 300, 2))
    assert by["all_300"]["nsel"] == sum(s < BAD_SLOT for s in cases[[c["_name"] for c in cases].index("all_300")]["status"]) > 200


def test_hostile_cases_leave_no_report_and_no_dead_guard(exe):
    cases = hostile_cases()
    rc, outs, err = run(exe, cases)
    assert rc == 0, err                       # no sanitizer report
    assert len(outs) == len(cases)
    for c, o in zip(cases, outs):
        assert o["guard"] == 1, ("guard", c["_name"])
        assert all(0 <= s <= 6 for s in o["status"]), c["_name"]
        rep = o["report"]
        assert rep[0] == len(c["status"]) == sum(rep[1:8]), (c["_name"], rep)      # the sum identity
        assert rep[1:8] == [o["status"].count(s) for s in range(7)], (c["_name"], rep)
        diff = [i for i, s in enumerate(o["status"]) if s]
        assert rep[8] == (diff[0] if diff else U64), c["_name"]
    by = {c["_name"]: o for c, o in zip(cases, outs)}
    some = [0, 5, 17, 39]
    # what the header promises of such input: a length no record has is VALUE_LEN, a byte that is no code BAD_ADDR (a
    # scan status that is none BAD_SLOT, NOT_TEXT a record like any other), and untouched records keep their verdict
    for name in ("a_length_all_ones", "b_length_all_ones", "both_lengths_all_ones"):
        assert [by[name]["status"][i] for i in some] == [VALUE_LEN] * 4
    assert [by["status_bytes_no_code"]["status"][i] for i in some] == [BAD_ADDR] * 4
    assert [by["scan_status_bytes_no_code"]["status"][i] for i in some] == [BAD_SLOT] * 3 + [SAME]
    for name in ("a_past_its_image", "b_past_its_image", "a_wraps", "b_wraps", "a_length_all_ones", "status_bytes_no_code"):
        assert all(s == SAME for i, s in enumerate(by[name]["status"]) if i not in some), name
    for name in ("coff_random", "coff_unsorted", "coff_all_equal"):      # a record that was not FOUND stays what it was
        assert by[name]["status"][0::3] == ([REJECTED, KEY_MISMATCH, BAD_ADDR] * 14)[: len(range(0, 40, 3))], name


# ---- mutations: the harness notices a subtly wrong kernel -------------------------------------------------------

MUTATIONS = [
    ("last_step_not_masked", "low_bytes_mask(n - x < 8 ? n - x : 8)", "low_bytes_mask(8)"),
    ("run_offset_dropped", "const uint64_t at = o - start;", "const uint64_t at = 0;"),
    ("length_test_dropped", "a.vlen_a[r] != a.vlen_b[r] || ", ""),
    ("b_bound_for_a_read", "ap < a.bytes_a ? sel_gload64(a.image_a, a.bytes_a, ap)", "ap < a.bytes_b ? sel_gload64(a.image_a, a.bytes_b, ap)"),
    ("second_step_skipped", "for (uint32_t x = 0; x < n; x += 8) {", "for (uint32_t x = 0; x < n; x += 16) {"),
    ("bad_slot_looked_up", "if (dump_status_in(a.status_a[r]) == DUMP_BAD_ADDR) {", "if (false) {"),
]


@pytest.fixture(scope="module")
def mutants(cxx, exe, tmp_path_factory):
    top = tmp_path_factory.mktemp("diff_mutants")

    def make(m):
        name, old, new = m
        d = str(top / name)
        shutil.copytree(CSRC, d, ignore=shutil.ignore_patterns("*.o", "*.so", "*.so.*", "*.a"))
        path = os.path.join(d, "diff_kernels.hip")
        text = open(path).read()
        if text.count(old) != 1:              # a refactor moved the line: the entry must follow it
            return name, None, f"diff_kernels.hip: {old!r} occurs {text.count(old)} times, not once"
        with open(path, "w") as f:
            f.write(text.replace(old, new))
        r = build(cxx, os.path.join(d, "diff_host_check"), d)
        return name, os.path.join(d, "diff_host_check"), r.stderr[-3000:] if r.returncode else None

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
