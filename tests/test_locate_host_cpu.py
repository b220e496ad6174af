"""The kernels that decide whether an address is safe to touch -- k_get_locate
(get_kernels.hip), k_verify_structure / k_verify_fixed / k_verify_var
(verify_kernels.hip), k_lookup / k_sign / k_index_scatter (mph_kernels.hip) and
their device functions get_slot, get_decode, sel_gload64, mph_lookup_wide,
count_nonzero_pairs_wide, bitlist_get, sig_to_equation -- run on the host under
ASan + UBSan without a GPU, as tests/test_piece_host_cpu.py runs the piece-copy
kernels.

tests/locate_host_check.cpp includes the kernel files unchanged; the header
tests/hostwave/hip/hip_runtime.h stands in for HIP's.  The program is started
as a program of its own (nothing is loaded into Python).  E, values, the
checksum bits, the index, the image and the keys sit in allocations of exactly
their documented lengths, every output between guard bytes: a read one word
past values[], sigbits[], E[m] or the image, which on a GPU is slack of a larger
allocation, is a report here.

Ground truth is Python's (tests/locate_cases.py): the address rule, the image
layout, the oracle's MPHF and lookup.  Valid cases are compared exactly.  The
hostile cases run only here, never on a GPU, and have a truth too:
  1  index words against a fixed image (random, sign bit, partition out of
     range, addresses next to valid ones, the ends of partitions and blocks,
     headers planted in value bytes): status, src, vlen and the report are the
     rule's;
  2  containment: the same queries grouped by the container (partition or block)
     their slot names, against an image whose every byte outside that container
     is inverted: nothing may change.  ASan cannot see a read of the neighbour's
     bytes (they are in the same allocation); this does;
  3  offset arrays the structure check accepts but no build made, over random
     values and checksum words: equal to the oracle's lookup on the same arrays;
  4  offset arrays the check must refuse: flag bit 0, and then the record kernels
     write nothing and read no word of values[] (a zero-length allocation).

test_mutation: one-line edits of the library's sources, each built against a
copy and each required to fail at least one case.  One of the edits cannot
fail any: see EQUIVALENT.

What this emulation proves: addressing, arithmetic, uniform control flow.  What
it does not (the shim's opening comment): the memory model, races between
lanes, code generation, speed.  The GPU suite stays the judge of the real
kernels; tests/test_locate_cases_gpu.py runs the valid cases there."""
import collections
import concurrent.futures
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import locate_cases as L  # noqa: E402
from test_piece_host_cpu import CSRC, FLAGS, SHIM, encode, find_compiler  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "locate_host_check.cpp")
LAYOUTS = [l[0] for l in L.HOSTILE_LAYOUTS]


def build(cxx, exe, csrc=CSRC):
    return subprocess.run([cxx] + FLAGS + ["-I", SHIM, "-I", csrc, "-o", exe, SRC], capture_output=True, text=True)


def run(exe, cases):
    """(exit status, one dict per case that ran, the end of stderr)."""
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
    path = str(tmp_path_factory.mktemp("locate_host") / "locate_host_check")
    r = build(cxx, path)
    assert r.returncode == 0, r.stderr[-3000:]
    rc, _, err = run(path, [])
    if rc != 0:
        pytest.skip("the sanitized program does not start in this environment: " + err.strip()[-300:])
    return path


# ---- the check: raises AssertionError on the first case that is wrong -------------------------------------------

def first_difference(got, want):
    return next((i for i, (g, w) in enumerate(zip(got, want)) if g != w), min(len(got), len(want)))


def check(cases, outs):
    assert len(outs) == len(cases)
    for c, o in zip(cases, outs):
        name, mode = c["_name"], c["mode"]
        assert o.get("intact", 1) == 1, ("guard", name)
        if mode == "locate":
            st, src, vl, rep = L.locate_expected(c)
            for what, got, want in (("status", o["status"], st), ("src", o["src"], src), ("vlen", o["vlen"], vl), ("report", o["report"], rep)):
                if got != want:
                    i = first_difference(got, want)
                    raise AssertionError((name, what, "query", i, "got", got[i: i + 1], "want", want[i: i + 1]))
        elif mode == "verify":
            assert o["report"] == L.verify_expected(c), (name, o["report"], L.verify_expected(c))
        elif mode == "lookup":
            want = L.lookup_expected(c)
            assert o["out"] == want, (name, first_difference(o["out"], want))
        elif mode == "sign":
            want = L.sign_expected(c)
            assert o["out"] == want, (name, first_difference(o["out"], want))
        elif mode == "scatter":
            index, index_a = L.scatter_expected(c)
            assert o["index"] == index, (name, first_difference(o["index"], index))
            assert bytes.fromhex(o["index_a"]) == index_a, name
        elif mode == "count":
            want = L.count_expected(c)
            assert o["wide"] == want, (name, "wide", c["_spans"][first_difference(o["wide"], want)])
            assert o["narrow"] == want, (name, "narrow", c["_spans"][first_difference(o["narrow"], want)])
        elif mode == "structure":
            assert o["report"] == [0] * 6 + [int(c["_refuse"]), 0], (name, o["report"])
        elif mode == "decode":
            want = L.decode_expected(c)
            for what, w in zip(("ok", "part", "pos", "limit"), want):
                assert o[what] == w, (name, what, hex(c["words"][first_difference(o[what], w)]))
        else:
            raise AssertionError(mode)


def run_ok(exe, cases):
    rc, outs, err = run(exe, cases)
    assert rc == 0, err                       # no sanitizer report
    check(cases, outs)
    return outs


# ---- the valid cases ---------------------------------------------------------------------------------------------

def test_locate_valid(exe):
    cases = L.locate_valid()
    names = {c["_name"] for c in cases}
    assert {f"n{n}" for n in L.NS} | {f"width{w}" for w in L.WIDTHS} | {f"fixed{k}" for k in L.FIXED_LENS} <= names
    assert {f"nq{q}" for q in L.NQS} | {"nq4101", "k13_nq4_kmis0", "k13_nq5_kmis12", "values_compact", "values_blocked"} <= names
    seen = collections.Counter(s for c in cases for s in L.locate_expected(c)[0])
    assert all(seen[s] > 50 for s in (L.FOUND, L.REJECTED, L.KEY_MISMATCH))
    # the twins: a slot that names a record whose key differs in its last byte only is a mismatch at every tail length
    c = next(c for c in cases if c["_name"] == "width13")
    st = dict(zip(c["_keys"], L.locate_expected(c)[0]))
    db = L.db_by_width(13)
    assert sorted(len(db.keys[i]) for i in db.victims) == sorted(L.TAIL_LENS)
    assert all(st[db.keys[i]] == L.KEY_MISMATCH for i in db.victims)
    # the value lengths, and a record that ends its partition / fills its block
    for c in cases[-2:]:
        assert {0, 1, 255, 256, 65535} <= set(L.locate_expected(c)[2])
    run_ok(exe, cases)


def test_lookup_and_sign_valid(exe):
    cases = L.mph_valid()
    assert {(c["mode"], c["width"]) for c in cases} >= {(m, w) for m in ("lookup", "sign") for w in L.WIDTHS if w or m == "lookup"}
    assert {c["n"] for c in cases} == set(L.NS)
    run_ok(exe, cases)


def test_index_scatter_valid(exe):
    cases = L.scatter_valid()
    assert any(c["approx"] for c in cases) and any(not c["approx"] for c in cases)
    assert {0, 7, 8, 9, 255} <= {v for c in cases if c["approx"] for v in c["value_len"]}
    run_ok(exe, cases)


def test_count_nonzero_pairs(exe):
    cases = L.count_valid()
    assert {c["vmis"] for c in cases} == {0, 8}
    spans = {(s & 31, e & 31, (e >> 5) - (s >> 5), (s >> 5) & 1) for c in cases for s, e in c["_spans"]}
    assert {(so, eo, words, par) for so in (0, 1, 31) for eo in (0, 1, 31) for words in range(1, 5) for par in (0, 1)} <= spans
    run_ok(exe, cases)


def test_verify_valid(exe):
    cases = L.verify_valid()
    kinds = {(("off" in c) * 2 or int(c.get("key_len") != 13), "addr" in c, "index_a" in c) for c in cases}
    assert {(k, a, False) for k in (0, 1, 2) for a in (True, False)} | {(k, True, True) for k in (0, 1, 2)} <= kinds
    exp = [L.verify_expected(c) for c in cases]
    assert any(e[3] == 1 for e in exp) and any(e[4] == 1 for e in exp) and any(e[1] for e in exp)
    assert any(0 < e[2] < e[0] - e[1] for e in exp) and any(e[2] == 0 and e[0] for e in exp)        # a window that cuts; an empty one
    run_ok(exe, cases)


def test_layout_restated(cxx, tmp_path):
    """locate_cases.layout against get_layout itself, through tests/get_plan_check.cpp (which pins it)."""
    prog = str(tmp_path / "get_plan_check")
    r = subprocess.run([cxx] + FLAGS + ["-o", prog, os.path.join(ROOT, "tests", "get_plan_check.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    sets = [L.hostile_db(l).image.sizes for l in LAYOUTS] + [db.image.sizes for db in L.db_values()] + [L.db_by_width(4).image.sizes]
    lines = [" ".join([f"parts={len(s)}"] + [f"size{p}={x}" for p, x in enumerate(s)]) for s in sets]
    r = subprocess.run([prog], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    for s, line in zip(sets, r.stdout.splitlines()):
        p = json.loads(line)
        assert (p["base"][: len(s)], p["total"]) == L.layout(s), s


# ---- the hostile cases: here only ---------------------------------------------------------------------------------

def hostile_classes(layout):
    """Per class of hostile word, how often each status is the truth (the full rounds, not the containment runs)."""
    db = L.hostile_db(layout)
    table = collections.defaultdict(collections.Counter)
    for idx, recs in L.hostile_rounds(layout):
        for i, cls in recs:
            table[cls][db.image.slot(idx[db.rank[i]], db.keys[i])[0]] += 1
    return table


@pytest.mark.parametrize("layout", LAYOUTS)
def test_hostile_index_words_and_containment(exe, layout):
    # a condition of the case set, on the Python truth alone: every status occurs at least 20 times
    table = hostile_classes(layout)
    total = sum(table.values(), collections.Counter())
    print(layout, {cls: dict(t) for cls, t in table.items()}, dict(total))
    assert all(total[s] >= 20 for s in (L.FOUND, L.KEY_MISMATCH, L.BAD_ADDR)), total
    want = {"random", "sign_bit", "partition", "near", "planted_record", "planted_prefix", "planted_at_the_end"}
    want |= {"compact_end", "tiny_partition"} if layout == "compact" else \
        {"bytes_0", "header_at_the_block_end", "block_past_the_file", "block_ends_the_file", "wider_block"}
    assert want <= set(table)
    assert dict(table["planted_at_the_end"]) == {L.FOUND: 1, L.KEY_MISMATCH: 1, L.BAD_ADDR: 1}
    assert set(table["planted_record"]) == {L.FOUND} and set(table["planted_prefix"]) == {L.KEY_MISMATCH}
    cases = L.hostile_index_cases(layout)
    # containment: every query of a round is asked once more against an image inverted outside its container
    assert sum("_span" not in c for c in cases) * L.N_HOSTILE == sum(c["nq"] for c in cases if "_span" in c)
    assert all(c["image"] != L.hostile_db(layout).image.bytes for c in cases if "_span" in c)
    run_ok(exe, cases + [L.decode_case(layout)])


def test_offset_arrays_the_structure_check_accepts(exe):
    """None of the shapes is left out of the comparison: the oracle's C lookup takes them all (it ran on them when
    locate_expected / lookup_expected were computed, in this process)."""
    cases = L.accepted_offset_cases()
    assert all(L.structure_valid(c["_mph"]["E"], c["n"]) for c in cases)
    structure = [dict(L.structure_case(c["_name"], c["E"], c["n"]), _refuse=False) for c in cases if c["mode"] == "lookup"]
    run_ok(exe, cases + structure)


def refused_cases():
    rng = np.random.default_rng(23)
    keys = L.distinct_keys(rng, 70, list(range(1, 20)))
    cases = []
    for name, E, n, refuse in L.refused_offset_arrays():
        for cus in (1, 2):
            cases.append(dict(L.structure_case(name, E, n, cus), _refuse=refuse))
        if refuse:                            # the record kernels then write nothing and read no word of values[]
            mph = dict(n=n, width=0, E=np.array(E, np.uint64), values=np.zeros(0, np.uint64), sigbits=None)
            cases.append(L.verify_case("verify_" + name, mph, keys, 2, list(range(n)), 0, n, addr=list(range(70)), no_values=True))
            cases.append(L.verify_case("verify13_" + name, mph, [k.ljust(13, b".")[:13] for k in keys], 0, list(range(n)), 0, n,
                                       addr_base=1, addr_stride=1))
            cases[-1]["no_values"] = 1
    return cases


def test_offset_arrays_the_structure_check_refuses(exe):
    cases = refused_cases()
    assert sum(c["mode"] == "structure" and c["_refuse"] for c in cases) > 60
    for c in cases:
        if c["mode"] == "verify":
            assert L.verify_expected(c) == [0, 0, 0, 0, 0, L.U64, 1, 0] and c["no_values"] == 1
    run_ok(exe, cases)
    # every valid array of the other cases leaves the flag clear
    valid = [dict(L.structure_case(c["_name"], c["E"], c["n"], 2), _refuse=False) for c in L.locate_valid() + L.mph_valid()]
    run_ok(exe, valid)


# ---- mutations: the harness notices a subtly wrong kernel -------------------------------------------------------

def hostile_all():
    return [c for l in LAYOUTS for c in L.hostile_index_cases(l)]


CASES = {
    "locate": L.locate_valid,
    "hostile": hostile_all,
    "hostile_compact": lambda: L.hostile_index_cases("compact"),
    "decode": lambda: [L.decode_case(l) for l in LAYOUTS],
    "mph": L.mph_valid,
    "count": L.count_valid,
    "scatter": L.scatter_valid,
    "verify": L.verify_valid,
    "structure": lambda: [c for c in refused_cases() if c["mode"] == "structure"],
}

MUTATIONS = [
    # (id, file, what is there, what replaces it, the case sets of which at least one case must notice)
    ("whole_record_test_strict", "get_kernels.hip", "s.ok = s.p + 3 + s.kl + s.vb <= s.lim;", "s.ok = s.p + 3 + s.kl + s.vb < s.lim;",
     ["locate"]),
    ("header_read_under_the_image", "get_kernels.hip", "sel_gload64(db.image, s.lim, s.p)", "sel_gload64(db.image, db.image_bytes, s.p)",
     ["hostile", "decode"]),
    ("compact_header_may_cross", "get_plan.hpp", "r.pos <= size - 3", "r.pos <= size - 2", ["decode"]),
    ("block_end_strict", "get_plan.hpp", "r.limit <= size", "r.limit < size", ["locate"]),
    ("blocked_header_may_cross", "get_plan.hpp", "rec + 3 <= bytes", "rec <= bytes", ["decode"]),
    ("key_length_not_compared", "get_kernels.hip", "bool same = kl == klen;", "bool same = true;", ["hostile_compact"]),
    ("compare_tail_not_masked", "get_kernels.hip", "^ rdk(o)) & low_bytes_mask(k)) == 0", "^ rdk(o)) & ~0ULL) == 0", ["locate"]),
    ("wide_count_no_step_to_16", "verify_kernels.hip",
     "    if (blk < end_blk && ((uintptr_t)(a + blk) & 8)) pairs += nz_pairs(a[blk++]);  // up to a 16-byte boundary\n", "", ["count"]),
    ("rank_n_accepted", "verify_kernels.hip", "if (r >= v.n) return -1;", "if (r > v.n) return -1;", ["locate"]),
    ("bitlist_second_word_at_64", "mph_kernels.hip", "if (off + width > 64) x |=", "if (off + width >= 64) x |=", ["mph"]),
    ("structure_reads_past_E", "verify_kernels.hip", "if (b == m ? e != n : e > (E[b + 1] & OFFSET_MASK)) bad = true;",
     "if (e > (E[b + 1] & OFFSET_MASK)) bad = true;", ["structure"]),
    ("scatter_window_end", "mph_kernels.hip", "if ((uint64_t)r < start || idx >= len) continue;",
     "if ((uint64_t)r < start || idx > len) continue;", ["scatter"]),
    ("sign_drops_the_second_word", "mph_kernels.hip",
     "        if (off + v.width > 64) atomicOr((unsigned long long *)(out + word + 1), (unsigned long long)(val >> (64 - off)));\n", "",
     ["mph"]),
]

# The one edit no case can notice, and why.  get_decode returns ok only with pos + 3 <= limit, so the three header
# bytes get_slot reads always lie below s.lim: whether the bounded reader is given s.lim or the image's length, it
# returns the same three bytes (the bytes above them, which do differ, are shifted out of kl and vb), and both
# limits lie inside the image's allocation, so ASan sees nothing either.  The reader's limit there is a second
# guard behind get_decode's; the first is pinned by compact_header_may_cross and blocked_header_may_cross.  The
# test states what does hold: the edit changes no output of any hostile case, the containment runs included.
EQUIVALENT = {"header_read_under_the_image"}


@pytest.fixture(scope="module")
def mutants(cxx, exe, tmp_path_factory):
    """Every mutation's program, built against a copy of the sources with the one substitution; built together."""
    top = tmp_path_factory.mktemp("locate_mutants")

    def make(m):
        name, fname, old, new = m[:4]
        d = str(top / name)
        shutil.copytree(CSRC, d, ignore=shutil.ignore_patterns("*.o", "*.so", "*.so.*", "*.a"))
        path = os.path.join(d, fname)
        text = open(path).read()
        if text.count(old) != 1:              # a refactor moved the line: the entry must follow it
            return name, None, f"{fname}: {old!r} occurs {text.count(old)} times, not once"
        with open(path, "w") as f:
            f.write(text.replace(old, new))
        r = build(cxx, os.path.join(d, "locate_host_check"), d)
        return name, os.path.join(d, "locate_host_check"), r.stderr[-3000:] if r.returncode else None

    with concurrent.futures.ThreadPoolExecutor(max(1, min(8, os.cpu_count() or 1))) as pool:
        return {name: (path, err) for name, path, err in pool.map(make, MUTATIONS)}


@pytest.mark.parametrize("name", [m[0] for m in MUTATIONS])
def test_mutation(mutants, name):
    """The one substitution makes at least one case of the named sets fail: a wrong output, a dead guard byte or a
    sanitizer report."""
    path, err = mutants[name]
    assert err is None, err
    noticed = False
    for which in next(m[4] for m in MUTATIONS if m[0] == name):
        cases = CASES[which]()
        rc, outs, stderr = run(path, cases)
        if rc != 0:
            assert "Sanitizer" in stderr or "runtime error" in stderr, stderr   # a report, not a program that does not start
            noticed = True
        else:
            try:
                check(cases, outs)
            except AssertionError:
                noticed = True
    assert noticed == (name not in EQUIVALENT), name
