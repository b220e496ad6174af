"""The kernels of the merge of resident databases
(bsdb_amd/csrc/merge_kernels.hip), run on the host under ASan + UBSan without a
GPU, as tests/test_diff_host_cpu.py runs the diff's.

tests/merge_host_check.cpp includes the kernel file unchanged; the header
tests/hostwave/hip/hip_runtime.h stands in for HIP's.  The image and every
descriptor array sit in an allocation of exactly their length, every output
between guard bytes at misalignments 0 .. 15.  The program is started as a
child process: nothing sanitized is loaded into Python.

Ground truth is Python's.  `expected_pack` restates what the header promises of
bsdb_dev_db_pack for ANY descriptors: a length is cut to 255 / 32 510, a source
byte at or past the image's end is 0 (a position that wraps is past the end),
the compact image is the records back to back per run, the blocked one what
kvfiles.write_blocked writes per run.  So the hostile position and length
cases (which run only here, never on a GPU) are compared byte for byte too; a
size scan that is no scan and status bytes that are no code must leave no
sanitizer report, no dead guard byte, and both identities of the report.

test_mutation: one-line edits of the sources, each built against a copy and
each required to fail a valid case."""
import concurrent.futures
import itertools
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
sys.path.insert(0, ROOT)
from bsdb_amd import kvfiles  # noqa: E402

SRC = os.path.join(ROOT, "tests", "merge_host_check.cpp")
U32, U64 = (1 << 32) - 1, (1 << 64) - 1
KEPT, REPLACED, REMOVED, BAD_SLOT, BAD_ADDR = range(5)
MAX_KEY, MAX_VALUE = 255, 32510


def build(cxx, exe, csrc=CSRC):
    return subprocess.run([cxx] + FLAGS + ["-I", SHIM, "-I", csrc, "-o", exe, SRC], capture_output=True, text=True)


def run(exe, cases):
    r = subprocess.run([exe], input="".join(encode(c) + "\n" for c in cases), capture_output=True, text=True, timeout=900)
    return r.returncode, [json.loads(line) for line in r.stdout.splitlines() if line.endswith("}")], r.stderr[-3000:]


@pytest.fixture(scope="module")
def cxx():
    c = find_compiler()
    if c is None:
        pytest.skip("no clang++ on this machine (the kernel files need clang's extensions)")
    return c


@pytest.fixture(scope="module")
def exe(cxx, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("merge_host") / "merge_host_check")
    r = build(cxx, path)
    assert r.returncode == 0, r.stderr[-3000:]
    rc, _, err = run(path, [])
    if rc != 0:
        pytest.skip("the sanitized program does not start in this environment: " + err.strip()[-300:])
    return path


# ---- the restatement ----------------------------------------------------------------------------------------------

def status_of(b, d, r):
    """b: the scan status; d / r: locate's status, None when that database is not there."""
    if b not in (0, 2):
        return BAD_SLOT
    if (d is not None and d >= 3) or (r is not None and r >= 3):
        return BAD_ADDR
    return REPLACED if d == 0 else REMOVED if r == 0 else KEPT


def expected_status(c):
    n = len(c["base"])
    d, r = c.get("delta", [None] * n), c.get("removed", [None] * n)
    if c.get("delta_side"):
        st = [status_of(b, None, None) for b in c["base"]]
        rep = [0] * 6 + [n, st.count(KEPT), st.count(BAD_SLOT), 0, 0, 0]
    else:
        st = [status_of(*t) for t in zip(c["base"], d, r)]
        rep = [n] + [st.count(s) for s in range(5)] + [0] * 6
    return st, rep, [i for i, s in enumerate(st) if s == KEPT]


def source(image, pos, n):
    """n bytes at pos of the image as the pack reads them: nothing at or past the end, or through a position that wraps."""
    if pos >= len(image):
        return bytes(n)
    return (image[pos: pos + n] + bytes(n))[:n]


def records_of(c):
    img = c["image"]
    return [(source(img, ks, min(kl, MAX_KEY)), source(img, vs, min(vl, MAX_VALUE)))
            for ks, kl, vs, vl in zip(c["ksrc"], c["klen"], c["vsrc"], c["vlen"])]


def expected_pack(c, tmp):
    recs, parts, B = records_of(c), c.get("parts", 1), c.get("B", 0)
    before = (c.get("before", []) + [0] * parts)[:parts]
    n = len(recs)
    files, addr = [], []
    for p in range(parts):
        run = recs[p * n // parts: (p + 1) * n // parts]
        if not B:
            pos = before[p]
            for k, v in run:
                addr.append(p << 56 | pos)
                pos += 3 + len(k) + len(v)
            files.append(b"".join(bytes([len(k), len(v) >> 8, len(v) & 255]) + k + v for k, v in run))
            continue
        base = os.path.join(tmp, f"want.{p}")
        kb, ko = kvfiles.pack_values([k for k, _ in run])
        vb, vo = kvfiles.pack_values([v for _, v in run])
        a = kvfiles.write_blocked(base, 1, kb, ko, vb, vo, B)
        files.append(open(base + ".0", "rb").read())
        addr += [int(x) + (p << 56) + ((before[p] // 4096) << 16) for x in a]
    return dict(image=b"".join(files).hex(), run_bytes=[len(f) for f in files], addr=addr, blob=b"".join(k for k, _ in recs).hex(),
                off=np.concatenate([[0], np.cumsum([len(k) for k, _ in recs], dtype=np.int64)]).tolist(),
                value8=[int.from_bytes((v[:8] + bytes(8))[:8], "little") for _, v in recs], value_len=[min(len(v), 8) for _, v in recs],
                report=[0] * 9 + [n, sum(len(k) for k, _ in recs), sum(len(v) for _, v in recs)])


def case_of(records, seed=0, **kw):
    """A resident image holding `records` as whole records in a shuffled order with other bytes between them; the
    descriptors are k_db_records': key at +3, value behind the key."""
    rng = np.random.default_rng(seed + 7 * len(records))
    img, ksrc = bytearray(rng.integers(0, 256, int(rng.integers(0, 40)), dtype=np.uint8).tobytes()), [0] * len(records)
    for i in rng.permutation(len(records)):
        k, v = records[i]
        img += rng.integers(1, 256, int(rng.integers(0, 9)), dtype=np.uint8).tobytes()
        ksrc[i] = len(img) + 3
        img += bytes([len(k), len(v) >> 8, len(v) & 255]) + k + v
    return dict(image=bytes(img), ksrc=ksrc, klen=[len(k) for k, _ in records], vsrc=[p + len(k) for p, (k, _) in zip(ksrc, records)],
                vlen=[len(v) for _, v in records], **kw)


def rb(rng, n):
    return rng.integers(0, 256, int(n), dtype=np.uint8).tobytes()


def valid_cases():
    rng = np.random.default_rng(2028)
    cases = []
    # every key length 1 .. 255, values around the 8-byte step and the 16-byte piece; every misalignment of both outputs
    vl = [0, 1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33]
    recs = [(rb(rng, k), rb(rng, vl[k % len(vl)])) for k in range(1, 256)]
    for mis in range(16):
        cases.append(dict(case_of(recs[mis * 16: mis * 16 + 40] if mis else recs, mis), mis=mis, bmis=(mis * 5 + 3) % 16, parts=1 + mis % 3,
                          _name=f"key_lengths_mis_{mis}"))
    # values around the block sizes and up to what a header holds (cut to 32 510), both block sizes and compact
    big = [1, 4000, 4092, 4093, 4094, 8180, 8188, 8189, 8190, 32510, 32511, 40000, 65535, 100, 0, 5]
    recs = [(rb(rng, 1 + i % 7), rb(rng, l)) for i, l in enumerate(big)]
    for B, parts in ((0, 1), (0, 3), (4096, 1), (4096, 2), (8192, 1), (8192, 3)):
        cases.append(dict(case_of(recs, B + parts), B=B, parts=parts, mis=(B // 4096 + parts) % 16, before=[4096 * 5 * p for p in range(parts)],
                          _name=f"value_lengths_B{B}_p{parts}"))
    # empty values, runs of 3-byte records (an empty value and a one-byte key is 4 bytes; 3-byte records have neither,
    # which only hostile descriptors give: klen 0) and counts around a wave
    cases.append(dict(case_of([(bytes([65 + i % 26]), b"") for i in range(70)], 3), mis=9, _name="empty_values"))
    tiny = case_of([(bytes([65 + i % 26]), b"") for i in range(130)], 4)
    tiny["klen"] = [0 if i % 4 else 1 for i in range(130)]
    cases.append(dict(tiny, mis=1, _name="three_byte_records"))
    for B in (4096, 8192):
        cases.append(dict(case_of([(rb(rng, 1 + i % 3), rb(rng, i % 5)) for i in range(1500)], B), B=B, parts=2, mis=7, _name=f"small_records_B{B}"))
    for n in (1, 63, 64, 65, 300):
        cases.append(dict(case_of([(rb(rng, rng.integers(1, 30)), rb(rng, rng.integers(0, 90))) for _ in range(n)], n), cus=1, mis=n % 16,
                          B=4096 if n % 2 else 0, parts=min(n, 2), _name=f"count_{n}"))
    return cases


def hostile_cases():
    rng = np.random.default_rng(17)
    base = case_of([(rb(rng, rng.integers(1, 20)), rb(rng, rng.integers(0, 60))) for _ in range(40)], 5)
    n, L = 40, len(base["image"])
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
    for B in (0, 4096):
        t = f"_B{B}"
        variant("key_at_and_past_the_end" + t, ksrc=at(some, [L - 1, L, L + 1, L + (1 << 40)]), B=B, mis=3)
        variant("value_at_and_past_the_end" + t, vsrc=at(some, [L - 1, L, L + 1, L - 9]), B=B, mis=5)
        variant("positions_wrap" + t, ksrc=at(some, [U64, U64 - 3, U64 - 254, 1 << 63]), vsrc=at(some, [U64 - 7, U64 - 32509, U64, (1 << 63) + 5]), B=B, mis=11)
        variant("lengths_all_ones" + t, klen=at(some, [U32] * 4), vlen=at(some[:2], [U32] * 2), B=B, parts=2, mis=13)
        variant("value_lengths_all_ones_at_the_end" + t, vlen=at(some, [U32, 65535, 32511, U32]), vsrc=at(some, [L - 2, 0, L - 100, L]), B=B, mis=15)
    true_roff = np.concatenate([[0], np.cumsum([3 + min(k, 255) + min(v, 32510) for k, v in zip(base["klen"], base["vlen"])])]).tolist()
    variant("roff_random", roff=sorted(int(x) for x in rng.integers(0, true_roff[-1], n + 1)), _noscan=1)
    variant("roff_unsorted", roff=[int(x) for x in rng.integers(0, 3000, n + 1)], _noscan=1)
    variant("roff_decreasing", roff=true_roff[::-1], _noscan=1)
    variant("roff_huge", roff=[U64 - i for i in range(n + 1)], _noscan=1)
    variant("roff_all_equal", roff=[0] * n + [true_roff[-1]], _noscan=1)
    variant("roff_first_not_zero", roff=[x + 100 for x in true_roff], _noscan=1)
    return out


def status_cases():
    codes = [0, 1, 2, 3, 4, 7, 255]
    combos = list(itertools.product(codes, codes, codes)) * 2
    b, d, r = ([t[i] for t in combos] for i in range(3))
    cases = [dict(op="status", base=b, delta=d, removed=r, mis=1, _name="all"), dict(op="status", base=b, delta=d, mis=2, _name="no_removed"),
             dict(op="status", base=b, removed=r, mis=3, _name="no_delta"), dict(op="status", base=b, mis=4, _name="rebuild"),
             dict(op="status", base=b, delta=d, removed=r, delta_side=1, mis=5, _name="delta_side")]
    rng = np.random.default_rng(3)
    for n in (1, 63, 64, 65, 300):
        cases.append(dict(op="status", base=[int(x) for x in rng.choice([0, 0, 0, 2, 1], n)], delta=[int(x) for x in rng.integers(0, 4, n)],
                          removed=[int(x) for x in rng.integers(0, 4, n)], cus=1, mis=n % 16, _name=f"count_{n}"))
    return cases


# ---- the cases on the library as it is ---------------------------------------------------------------------------

def check_pack(cases, outs, tmp):
    for c, o in zip(cases, outs):
        assert o["guard"] == 1, ("guard", c["_name"])
        if c.get("_noscan"):
            continue
        want = expected_pack(c, tmp)
        for k, v in want.items():
            if o[k] != v:
                where = next(i for i in range(min(len(v), len(o[k]))) if o[k][i] != v[i]) if len(v) == len(o[k]) else ("len", len(o[k]), len(v))
                raise AssertionError((c["_name"], k, where))


def check_status(cases, outs):
    for c, o in zip(cases, outs):
        st, rep, sel = expected_status(c)
        assert o["guard"] == 1, ("guard", c["_name"])
        assert o["status"] == st and o["report"] == rep, (c["_name"], o["report"], rep)
        assert o["nsel"] == len(sel) and o["sel"] == sel and o["ksrc"] == [1000 + i for i in sel] and o["vlen"] == [7 * i for i in sel], c["_name"]
        assert rep[0] == sum(rep[1:6])


def test_valid_cases(exe, tmp_path):
    cases = valid_cases()
    rc, outs, err = run(exe, cases)
    assert rc == 0, err
    assert len(outs) == len(cases)
    check_pack(cases, outs, str(tmp_path))
    by = {c["_name"]: (c, o) for c, o in zip(cases, outs)}
    c, o = by["value_lengths_B0_p1"]
    assert max(c["vlen"]) == 65535 and o["report"][11] == sum(min(v, MAX_VALUE) for v in c["vlen"])      # the cut is counted as written
    assert len(by["three_byte_records"][1]["image"]) // 2 == 130 * 3 + 33                                  # 33 of them have a key


def test_status_cases(exe):
    cases = status_cases()
    rc, outs, err = run(exe, cases)
    assert rc == 0, err
    assert len(outs) == len(cases)
    check_status(cases, outs)
    assert {s for c in cases for s in expected_status(c)[0]} == set(range(5))
    # bytes that are no code: a scan status that is none names no record, a locate status that is none is BAD_ADDR
    st = dict(zip(zip(cases[0]["base"], cases[0]["delta"], cases[0]["removed"]), outs[0]["status"]))
    assert st[(7, 0, 0)] == st[(255, 1, 1)] == st[(1, 0, 0)] == BAD_SLOT and st[(0, 255, 0)] == st[(2, 0, 4)] == st[(0, 1, 7)] == BAD_ADDR
    assert st[(0, 0, 0)] == REPLACED and st[(2, 1, 0)] == st[(0, 2, 0)] == REMOVED and st[(2, 1, 2)] == KEPT


def test_hostile_cases_leave_no_report_and_no_dead_guard(exe, tmp_path):
    cases = hostile_cases()
    rc, outs, err = run(exe, cases)
    assert rc == 0, err                       # no sanitizer report
    assert len(outs) == len(cases)
    check_pack(cases, outs, str(tmp_path))    # (positions and lengths: byte for byte what the header promises)
    for c, o in zip(cases, outs):
        rep = o["report"]
        assert rep[9] == len(c["ksrc"]) and rep[10] == sum(min(k, MAX_KEY) for k in c["klen"]), c["_name"]
        assert rep[11] == sum(min(v, MAX_VALUE) for v in c["vlen"]) and rep[:9] == [0] * 9, c["_name"]
        assert len(o["image"]) // 2 == sum(o["run_bytes"])
    by = {c["_name"]: o for c, o in zip(cases, outs)}
    assert set(by["roff_huge"]["image"]) == {"0"} and set(by["roff_first_not_zero"]["image"][:200]) == {"0"}    # no owner: zeros


# ---- mutations: the harness notices a subtly wrong kernel -------------------------------------------------------

MUTATIONS = [
    ("header_bytes_swapped", "merge_kernels.hip", "(uint64_t)(vl >> 8) << 8 | (uint64_t)(vl & 0xFF) << 16",
     "(uint64_t)(vl & 0xFF) << 8 | (uint64_t)(vl >> 8) << 16", "pack"),
    ("key_value_boundary_off_by_one", "merge_kernels.hip", "const uint32_t s0 = seg ? hdr + kl : hdr,", "const uint32_t s0 = seg ? hdr + kl + 1 : hdr,", "pack"),
    ("head_not_masked", "merge_kernels.hip", "(vsrc < bytes ? sel_gload64(image, bytes, vsrc) : 0) & low_bytes_mask(l);",
     "(vsrc < bytes ? sel_gload64(image, bytes, vsrc) : 0);", "pack"),
    ("last_step_not_masked", "piece_copy.hpp", "j + x, n - x < 8 ? n - x : 8);", "j + x, 8);", "pack"),
    ("value_length_uncut_in_the_sizes", "merge_kernels.hip", "const uint32_t kl = text_klen(klen[r]), vl = text_vlen(vlen[r]), sz = 3 + kl + vl;",
     "const uint32_t kl = text_klen(klen[r]), vl = vlen[r], sz = 3 + kl + vl;", "pack"),
    ("delta_ignored_when_removed_holds_the_key", "merge_plan.hpp", "if (d == GET_FOUND) return MERGE_REPLACED;",
     "if (d == GET_FOUND && r != GET_FOUND) return MERGE_REPLACED;", "status"),
    ("bad_slot_selected", "merge_plan.hpp", "if (dump_status_in(scan) == DUMP_BAD_ADDR) return MERGE_BAD_SLOT;",
     "if (dump_status_in(scan) == DUMP_BAD_ADDR) return MERGE_KEPT;", "status"),
]


@pytest.fixture(scope="module")
def mutants(cxx, exe, tmp_path_factory):
    top = tmp_path_factory.mktemp("merge_mutants")

    def make(m):
        name, fname, old, new, _ = m
        d = str(top / name)
        shutil.copytree(CSRC, d, ignore=shutil.ignore_patterns("*.o", "*.so", "*.so.*", "*.a"))
        path = os.path.join(d, fname)
        text = open(path).read()
        if text.count(old) != 1:              # a refactor moved the line: the entry must follow it
            return name, None, f"{fname}: {old!r} occurs {text.count(old)} times, not once"
        with open(path, "w") as f:
            f.write(text.replace(old, new))
        r = build(cxx, os.path.join(d, "merge_host_check"), d)
        return name, os.path.join(d, "merge_host_check"), r.stderr[-3000:] if r.returncode else None

    with concurrent.futures.ThreadPoolExecutor(max(1, min(4, os.cpu_count() or 1))) as pool:
        return {name: (path, err) for name, path, err in pool.map(make, MUTATIONS)}


@pytest.mark.parametrize("name", [m[0] for m in MUTATIONS])
def test_mutation(mutants, name, tmp_path):
    """The one substitution makes a valid case fail: wrong bytes, a wrong status, or a sanitizer report."""
    path, err = mutants[name]
    assert err is None, err
    kind = next(m[4] for m in MUTATIONS if m[0] == name)
    cases = valid_cases() if kind == "pack" else status_cases()
    rc, outs, stderr = run(path, cases)
    if rc != 0:
        assert "Sanitizer" in stderr or "runtime error" in stderr, stderr
        return
    assert len(outs) == len(cases)
    with pytest.raises(AssertionError):
        check_pack(cases, outs, str(tmp_path)) if kind == "pack" else check_status(cases, outs)
