"""The kernels of the enumeration of a resident database by slot
(bsdb_amd/csrc/dump_kernels.hip), run on the host under ASan + UBSan without a
GPU, as tests/test_piece_host_cpu.py runs the piece-copy kernels.

tests/dump_host_check.cpp includes the kernel file unchanged; the header
tests/hostwave/hip/hip_runtime.h stands in for HIP's.  The image, index.db and
the partition table sit in an allocation of exactly their length, every output
is a view between 0xA5 guard bytes at misalignments 0 - 15.

Ground truth is Python's.  The images are written here (compact) or by
bsdb_amd/kvfiles.py (blocked); a slot's status is the restatement of the
reference's bit fields in tests/test_get_plan_cpu.py (decode) and the header's
rule over the image's bytes; the text is the records' lines in slot order; a
record is text exactly when tests/text_rule.py reads its line back as that one
record.  Valid cases are compared word for word and byte for byte.  Hostile
cases (positions at and past the image's end, lengths no header can hold,
offsets that are no scan, slots that decode to every BAD_ADDR clause) must
leave no sanitizer report and no dead guard byte, and a report whose sum holds.

test_mutation: one-line edits of the kernel sources, each built against a copy
and each required to fail a valid case."""
import concurrent.futures
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import piece_cases as P  # noqa: E402
import text_rule as R  # noqa: E402
from test_get_plan_cpu import decode  # noqa: E402
from test_piece_host_cpu import CSRC, FLAGS, SHIM, encode, find_compiler  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bsdb_amd import kvfiles  # noqa: E402

SRC = os.path.join(ROOT, "tests", "dump_host_check.cpp")
U32, U64 = (1 << 32) - 1, (1 << 64) - 1
OK, BAD_ADDR, NOT_TEXT = 0, 1, 2
PAGE = 4096
LENS = (0, 1, 7, 8, 9, 15, 16, 17)


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
    path = str(tmp_path_factory.mktemp("dump_host") / "dump_host_check")
    r = build(cxx, path)
    assert r.returncode == 0, r.stderr[-3000:]
    rc, _, err = run(path, [])
    if rc != 0:
        pytest.skip("the sanitized program does not start in this environment: " + err.strip()[-300:])
    return path


# ---- databases and their restatement ------------------------------------------------------------------------------

def record_bytes(k, v):
    return bytes([len(k), len(v) >> 8, len(v) & 0xFF]) + k + v


def image_of(files):
    """The resident image of the partition files: each at a 16-byte aligned base, nothing after the last."""
    image, base = bytearray(), []
    for f in files:
        image += bytes(-len(image) % 16)
        base.append(len(image))
        image += f
    return bytes(image), base, [len(f) for f in files]


def compact_db(records, parts=1):
    """records -> (case fields, address per record); record i in partition i % parts (keys of any length, 0 too)."""
    files, addr = [bytearray() for _ in range(parts)], []
    for i, (k, v) in enumerate(records):
        addr.append((i % parts) << 56 | len(files[i % parts]))
        files[i % parts] += record_bytes(k, v)
    image, base, size = image_of(files)
    return dict(image=image, base=base, size=size, format=0), addr


def blocked_db(records, parts, B, tmp):
    kb, ko = kvfiles.pack_values([k for k, _ in records])
    vb, vo = kvfiles.pack_values([v for _, v in records])
    stem = os.path.join(str(tmp), f"kv{len(records)}_{parts}_{B}")
    addr = kvfiles.write_blocked(stem, parts, kb, ko, vb, vo, B)
    image, base, size = image_of([open(f"{stem}.{p}", "rb").read() for p in range(parts)])
    return dict(image=image, base=base, size=size, format=1), [int(a) for a in addr]


def is_text(k, v, sep):
    recs, _ = R.restate(k + sep + v + b"\n", sep)
    return [(rk, rv) for _, rk, _, rv in recs] == [(k, v)]


def slot_record(c, a):
    """(key position, kLen, value position, vLen) of the record address `a` names, or None: BAD_ADDR."""
    d = decode(a, c["format"], c["size"], c.get("dparts", len(c["size"])))
    if d is None:
        return None
    part, pos, limit = d
    image, b = c["image"], c["base"][part]
    kl, vl = image[b + pos], image[b + pos + 1] << 8 | image[b + pos + 2]
    if pos + 3 + kl + vl > limit:
        return None
    return b + pos + 3, kl, b + pos + 3 + kl, vl


def expected(c):
    """What both stages owe for a case whose index holds any addresses and whose image holds whole records."""
    first, count = c.get("first", 0), c.get("count", len(c["index"]) - c.get("first", 0))
    sep = bytes([c["sep"]])
    image = c["image"]
    w = dict(r_ksrc=[], r_klen=[], r_vsrc=[], r_vlen=[], r_status=[], llen=[], status=[], text=bytearray())
    for a in c["index"][first: first + count]:
        rec = slot_record(c, a)
        ks, kl, vs, vl = rec or (0, 0, 0, 0)
        k, v = image[ks: ks + kl], image[vs: vs + vl]
        w["r_ksrc"].append(ks), w["r_klen"].append(kl), w["r_vsrc"].append(vs), w["r_vlen"].append(vl)
        w["r_status"].append(OK if rec else BAD_ADDR)
        w["llen"].append(kl + vl + 2 if rec else 0)
        w["status"].append(BAD_ADDR if not rec else OK if is_text(k, v, sep) else NOT_TEXT)
        if rec:
            w["text"] += k + sep + v + b"\n"

    def report(st, text_bytes):
        bad = [i for i, s in enumerate(st) if s]
        return [count, st.count(OK), st.count(BAD_ADDR), st.count(NOT_TEXT), sum(w["r_klen"]), sum(w["r_vlen"]), text_bytes,
                first + bad[0] if bad else U64]

    w["r_report"] = report(w["r_status"], 0)
    w["report"] = report(w["status"], len(w["text"]))
    w["text"] = bytes(w["text"])
    return w


CLEAN = np.array([b for b in range(1, 256) if b not in (9, 10, 13, 32, 44)], np.uint8)


def clean(rng, n):
    """n bytes that are no separator of these tests and no line terminator."""
    return bytes(int(x) for x in rng.choice(CLEAN, n))


BAD = [1 << 63 | 5, U64, 9 << 56 | 1, 0 << 56 | (1 << 40)]     # top bit set (twice), partition >= partitions, past the file


def with_bad(addr, where):
    """Runs of BAD_ADDR slots put into the index before the positions `where` (len(addr): at the end)."""
    out = []
    for i in range(len(addr) + 1):
        if i in where:
            out += BAD[: where[i]]
        if i < len(addr):
            out.append(addr[i])
    return out


def valid_cases(tmp):
    rng = np.random.default_rng(2025)
    cases = []

    def add(name, db, index, sep=b" ", **kw):
        cases.append(dict(db, index=index, sep=sep[0], _name=name, **kw))

    # every pair of lengths around the 8-byte step and the 16-byte piece, at every misalignment; alone at three
    pairs = [(kl, vl) for kl in LENS for vl in LENS]
    for mis in range(16):
        order = rng.permutation(len(pairs))
        recs = [(clean(rng, pairs[i][0]), clean(rng, pairs[i][1])) for i in order]
        db, addr = compact_db(recs, parts=1 + mis % 3)
        add("enumeration", db, addr, mis=mis)
    for mis in (0, 5, 15):
        for kl, vl in pairs:
            db, addr = compact_db([(clean(rng, kl), clean(rng, vl))])
            add("one_record", db, addr, mis=mis)
    # 40 one-byte values in a row
    db, addr = compact_db([(clean(rng, 1 + i % 2), clean(rng, 1)) for i in range(40)], parts=2)
    add("one_byte_run", db, addr, mis=3)
    # a 65 535-byte value beside a 60 000-byte one; the longest value the text carries, and one byte more
    big = [(b"n0", clean(rng, 5)), (b"big0", clean(rng, 65535)), (b"big1", clean(rng, 60000)), (b"n1", clean(rng, 16)),
           (b"t0", clean(rng, 32510)), (b"t1", clean(rng, 32511)), (b"K" * 255, clean(rng, 3))]
    db, addr = compact_db(big)
    add("longest", db, addr, mis=7)
    assert expected(cases[-1])["status"] == [OK, NOT_TEXT, NOT_TEXT, OK, OK, NOT_TEXT, OK]
    # BAD_ADDR runs at the start, in the middle and at the end; windows of it
    recs = [(b"k%d" % i, clean(rng, int(rng.integers(1, 40)))) for i in range(30)]
    db, addr = compact_db(recs, parts=3)
    index = with_bad(addr, {0: 3, 11: 1, 17: 4, 30: 2})
    add("bad_runs", db, index, mis=9)
    st = expected(cases[-1])["status"]
    assert st[:3] == [BAD_ADDR] * 3 and st[-2:] == [BAD_ADDR] * 2 and st.count(BAD_ADDR) == 10 and st.count(OK) == 30
    for first, count in ((0, 0), (0, 1), (1, 2), (3, 20), (14, 26), (39, 1), (40, 0)):
        add("window", db, index, mis=first % 16, first=first, count=count)
    add("all_bad", db, BAD * 20, mis=1)
    # the blocked layout: blocks of one and two pages, a record larger than a block, one that ends at a block's end
    for B in (PAGE, 2 * PAGE):
        recs = [(b"b%d" % i, clean(rng, int(rng.integers(1, 300)))) for i in range(60)]
        recs[7] = (b"large", clean(rng, B + 100))
        recs[20] = (b"exact", clean(rng, B - 3 - 5))          # a block of its own, filled to its last byte
        db, addr = blocked_db(recs, 2, B, tmp)
        add(f"blocked_{B}", db, with_bad(addr, {0: 1, 30: 2, 60: 1}), sep=b"\t", mis=B // PAGE)
        assert expected(cases[-1])["status"].count(OK) == 60
    # record counts around a wave and a workgroup
    for n in (1, 63, 64, 65, 257):
        db, addr = compact_db([(b"c%d" % i, clean(rng, int(rng.integers(1, 20)))) for i in range(n)])
        add(f"count_{n}", db, addr, mis=n % 16)
    # one CU: 4 096 lanes and 8 192 pieces a trip; 4 200 records of ~40 bytes enter the second trip of both loops
    db, addr = compact_db([(b"s%d" % i, clean(rng, 20 + i % 31)) for i in range(4200)], parts=2)
    add("second_trip", db, addr, mis=5, cus=1)
    # the bytes' part of the text test: the separator, 0x0A and 0x0D at every byte of a key and of a 33-byte value,
    # an honest one-byte record between every two; a separator byte that is not this dump's is an ordinary byte
    for sep, other in ((b" ", b"\t"), (b"\t", b" "), (b",", b" ")):
        recs = []
        for j in range(33):
            for byte in (sep, b"\n", b"\r", other):
                v = clean(rng, 33)
                recs += [(b"v%d" % j, v[:j] + byte + v[j + 1:]), (b"h", clean(rng, 1))]
        for j in range(17):
            k = clean(rng, 17)
            recs += [(k[:j] + sep + k[j + 1:], b"x"), (k[:j] + b"\n" + k[j + 1:], b"y"), (k[:j] + other + k[j + 1:], b"z")]
        recs += [(b"last", b"ab" + sep), (b"only", sep), (b"e", b""), (b"", b"v"), (b"", b"")]
        db, addr = compact_db(recs, parts=2)
        add("not_text", db, addr, sep=sep, mis=sep[0] % 16)
        st = expected(cases[-1])["status"]
        assert st[: 33 * 8] == [NOT_TEXT, OK, NOT_TEXT, OK, NOT_TEXT, OK, OK, OK] * 33
        assert st[33 * 8: 33 * 8 + 51] == [NOT_TEXT, NOT_TEXT, OK] * 17 and st[-5:] == [NOT_TEXT] * 5
    # any bytes at all: the oracle decides
    recs = [(bytes(rng.integers(0, 256, int(rng.integers(1, 20)), dtype=np.uint8)),
             bytes(rng.integers(0, 256, int(rng.integers(0, 60)), dtype=np.uint8))) for _ in range(200)]
    db, addr = compact_db(recs, parts=3)
    add("random_bytes", db, addr, mis=11)
    return cases


FIELDS = ("r_ksrc", "r_klen", "r_vsrc", "r_vlen", "r_status", "r_report", "llen", "status", "report")


def check_valid(cases, outs):
    for c, o in zip(cases, outs):
        w = expected(c)
        assert o["guard"] == 1, ("guard", c["_name"])
        for f in FIELDS:
            if o[f] != w[f]:
                bad = next(i for i in range(len(w[f])) if o[f][i] != w[f][i])
                raise AssertionError((c["_name"], c.get("mis"), f, "entry", bad, "got", o[f][bad], "want", w[f][bad]))
        got = bytes.fromhex(o["text"])
        if got != w["text"]:
            bad = next((i for i in range(min(len(got), len(w["text"]))) if got[i] != w["text"][i]), -1)
            raise AssertionError((c["_name"], c.get("mis"), "text byte", bad, len(got), len(w["text"])))


def test_valid_cases(exe, tmp_path):
    cases = valid_cases(tmp_path)
    names = {c["_name"] for c in cases}
    assert {"enumeration", "one_byte_run", "longest", "bad_runs", "blocked_4096", "blocked_8192", "second_trip",
            "not_text"} <= names
    rc, outs, err = run(exe, cases)
    assert rc == 0, err
    assert len(outs) == len(cases)
    check_valid(cases, outs)


# ---- hostile input ------------------------------------------------------------------------------------------------

def hostile_slots():
    """Stage 1 over slots that decode to each BAD_ADDR clause, both layouts; the statuses are the restatement's."""
    rng = np.random.default_rng(11)
    out = []
    recs = [(b"k%d" % i, clean(rng, 10)) for i in range(12)]
    db, addr = compact_db(recs, parts=3)
    size = db["size"]
    last = [max(a for a in addr if a >> 56 == p) for p in range(3)]
    crafted = bytearray(db["image"])
    at = db["base"][2] + size[2] - 3                       # a header at a partition's end that claims 65 535 bytes
    crafted[at: at + 3] = b"\x05\xff\xff"
    index = addr + [1 << 63, U64, 3 << 56, 127 << 56 | 4, 1 << 56 | size[1], 1 << 56 | (size[1] - 1), 1 << 56 | (size[1] - 2),
                    1 << 56 | (size[1] - 3), 0 << 56 | 5, 2 << 56 | (size[2] - 3), (1 << 56) - 1] + last
    out.append(dict(db, image=bytes(crafted), index=index, sep=32, _name="compact_clauses"))
    out.append(dict(db, index=index, sep=32, dparts=2, _name="fewer_partitions"))
    out.append(dict(image=b"\x01\x00", base=[0], size=[2], format=0, index=[0, 1, 2], sep=32, _name="file_below_a_header"))
    out.append(dict(image=b"", base=[0], size=[0], format=0, index=[0, 1 << 56], sep=32, _name="empty_file"))
    brecs = [(b"b%d" % i, clean(rng, 50)) for i in range(40)]

    def baddr(part, pages, page_pos, rec):
        return part << 56 | pages << 48 | page_pos << 16 | rec

    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        bdb, baddrs = blocked_db(brecs, 1, PAGE, tmp)
    pages = bdb["size"][0] // PAGE
    index = baddrs + [baddr(0, 0, 0, 0), baddr(0, 1, pages, 0), baddr(0, 2, pages - 1, 0), baddr(0, 1, 0, 4096), baddr(0, 1, 0, 4094),
                      baddr(0, 1, 0, 4093), baddr(0, 255, 0xFFFFFFFF, 0), baddr(1, 1, 0, 0), 1 << 63 | baddrs[0], baddr(0, 1, 0, 2)]
    out.append(dict(bdb, index=index, sep=9, _name="blocked_clauses"))
    return out


def hostile_descriptors():
    """Stage 2 over descriptors and offsets that no records kernel wrote."""
    rng = np.random.default_rng(13)
    recs = [(b"h%d" % i, clean(rng, int(l))) for i, l in enumerate(rng.integers(1, 50, 40))]
    db, addr = compact_db(recs)
    w = expected(dict(db, index=addr, sep=32))
    base = dict(image=db["image"], ksrc=w["r_ksrc"], klen=w["r_klen"], vsrc=w["r_vsrc"], vlen=w["r_vlen"], status=[0] * 40, sep=32)
    I, out = len(db["image"]), []

    def variant(name, **kw):
        c = {k: (list(v) if isinstance(v, list) else v) for k, v in base.items()}
        for k, f in kw.items():
            c[k] = f(c[k]) if callable(f) else f
        out.append(dict(c, mis=len(out) % 16, _name=name))

    def at(idx, vals):
        def f(lst):
            for i, v in zip(idx, vals):
                lst[i] = v
            return lst
        return f

    some = [0, 5, 17, 39]
    variant("ksrc_past_the_image", ksrc=at(some, [I - 1, I, I + 1, I + 1000]))
    variant("vsrc_past_the_image", vsrc=at(some, [I - 1, I, I + 7, 1 << 62]))
    variant("src_wraps", ksrc=at(some, [U64, U64 - 3, 1 << 63, U64 - 20]), vsrc=at(some, [U64 - 1, U64 - 8, U64 - 300, U64]))
    variant("klen_no_header_holds", klen=at(some, [256, 65536, U32, 1 << 31]))
    variant("vlen_no_header_holds", vlen=at(some, [65536, 65537, U32, 1 << 31]))
    variant("both_lengths_all_ones", klen=at(some, [U32] * 4), vlen=at(some, [U32] * 4))
    variant("both_lengths_largest", klen=at(some, [255] * 4), vlen=at(some, [65535] * 4))
    variant("status_bytes_no_code", status=at(some, [3, 4, 200, 255]))
    n = len(recs)
    true_loff = np.concatenate([[0], np.cumsum(w["llen"])]).tolist()
    total = true_loff[-1]
    variant("loff_random", loff=sorted(int(x) for x in rng.integers(0, total, n + 1)), text_bytes=total)
    variant("loff_unsorted", loff=[int(x) for x in rng.integers(0, total, n + 1)], text_bytes=total)
    variant("loff_decreasing", loff=true_loff[::-1], text_bytes=total)
    variant("loff_total_larger", loff=true_loff[:-1] + [total + 3000], text_bytes=total + 3000)
    variant("loff_all_equal", loff=[0] * n + [700], text_bytes=700)
    variant("loff_first_not_zero", loff=[x + 100 for x in true_loff], text_bytes=total + 100)
    variant("loff_words", loff=[int(rng.integers(0, U64, dtype=np.uint64)) for _ in range(n + 1)], text_bytes=total)
    variant("text_shorter_than_the_scan", text_bytes=total - 21)
    variant("text_longer_than_the_scan", text_bytes=total + 37)
    # the families of piece_cases.gather_hostile: its offsets as the lines' scan, its sources as both positions
    for g in P.gather_hostile():
        cnt = len(g["src"])
        image = bytes(P.image_byte(i) for i in range(g["image_bytes"]))
        out.append(dict(image=image, ksrc=g["src"], vsrc=g["src"][::-1], klen=[int(x) for x in rng.integers(0, 12, cnt)],
                        vlen=[int(x) for x in rng.integers(0, 12, cnt)], status=[0] * cnt, sep=32, loff=g["voff"],
                        text_bytes=g["value_bytes"], mis=g["mis"], _name="gather_" + g["_family"]))
    return out


def owed_text(c):
    """The text a true scan owes for any descriptors whose positions do not wrap: lengths cut to what a header
    holds, a byte at or past the image's end 0."""
    image, out = c["image"], bytearray()

    def fetch(pos, n):
        return bytes(image[p] if p < len(image) else 0 for p in range(pos, pos + n))

    for ks, kl, vs, vl, st in zip(c["ksrc"], c["klen"], c["vsrc"], c["vlen"], c["status"]):
        if st in (OK, NOT_TEXT):
            out += fetch(ks, min(kl, 255)) + bytes([c["sep"]]) + fetch(vs, min(vl, 65535)) + b"\n"
    return bytes(out)


def test_hostile_cases_leave_no_report_and_no_dead_guard(exe):
    cases = hostile_slots() + hostile_descriptors()
    rc, outs, err = run(exe, cases)
    assert rc == 0, err                       # no sanitizer report
    assert len(outs) == len(cases)
    for c, o in zip(cases, outs):
        name = c["_name"]
        assert o["guard"] == 1, ("guard", name)
        count = len(o["status"])
        assert all(s in (OK, BAD_ADDR, NOT_TEXT) for s in o["status"]), name
        rep = o["report"]
        assert rep[0] == count == sum(rep[1:4]) and rep[1:4] == [o["status"].count(s) for s in range(3)], (name, rep)
        bad = [i for i, s in enumerate(o["status"]) if s]
        assert rep[7] == (bad[0] if bad else U64), name
        assert all(l <= 255 + 65535 + 2 for l in o["llen"]) and rep[6] == sum(o["llen"]), name
        if "index" in c:                      # slots: the restatement decides every word, the text included
            w = expected(c)
            assert [o[f] for f in FIELDS] == [w[f] for f in FIELDS], name
            assert bytes.fromhex(o["text"]) == w["text"], name
        elif "loff" not in c and "text_bytes" not in c and name != "src_wraps":
            assert bytes.fromhex(o["text"]) == owed_text(c), name
    by = {c["_name"]: o for c, o in zip(cases, outs)}
    # every clause occurs: the crafted 65 535-byte record and the header across a file's end among them
    st = by["compact_clauses"]["r_status"]
    assert st[:12] == [OK] * 12 and st[12:23] == [BAD_ADDR] * 11 and st[23:] == [OK] * 3
    assert by["fewer_partitions"]["r_status"].count(BAD_ADDR) > by["compact_clauses"]["r_status"].count(BAD_ADDR)
    assert by["file_below_a_header"]["r_status"] == [BAD_ADDR] * 3 and by["empty_file"]["r_status"] == [BAD_ADDR] * 2
    st = by["blocked_clauses"]["r_status"]
    assert st[:40] == [OK] * 40 and st[40:].count(BAD_ADDR) == 9 and st[45] == OK   # (a header of zeros at a block's end: an empty record)
    some = [0, 5, 17, 39]
    assert [by["status_bytes_no_code"]["status"][i] for i in some] == [BAD_ADDR] * 4
    for name in ("klen_no_header_holds", "vlen_no_header_holds", "both_lengths_all_ones"):
        assert [by[name]["status"][i] for i in some] == [NOT_TEXT] * 4, name
    assert [by["both_lengths_all_ones"]["llen"][i] for i in some] == [255 + 65535 + 2] * 4


# ---- mutations: the harness notices a subtly wrong kernel -------------------------------------------------------

MUTATIONS = [
    ("terminator_one_byte_early", "dump_kernels.hip", "const uint32_t t = kl + 1 + vl;", "const uint32_t t = kl + vl;"),
    ("separator_in_the_text_test", "dump_kernels.hip", "lo |= dump_byte_range(j < 8 ? j : 8, je < 8 ? je : 8);",
     "lo |= dump_byte_range(j < 8 ? j : 8, je < 8 ? je + 1 : 8);"),
    ("record_end_test_strict", "get_kernels.hip", "s.ok = s.p + 3 + s.kl + s.vb <= s.lim;", "s.ok = s.p + 3 + s.kl + s.vb < s.lim;"),
    ("first_bad_not_a_slot", "dump_kernels.hip", "if (st != DUMP_OK && first_bad == DUMP_NONE) first_bad = a.first + r;",
     "if (st != DUMP_OK && first_bad == DUMP_NONE) first_bad = r;"),
    ("byte_test_carries", "dump_kernels.hip", "return ~(((y & m) + m) | y | m);", "return (y - 0x0101010101010101ull) & ~y & ~m;"),
]


@pytest.fixture(scope="module")
def mutants(cxx, exe, tmp_path_factory):
    top = tmp_path_factory.mktemp("dump_mutants")

    def make(m):
        name, fname, old, new = m
        d = str(top / name)
        shutil.copytree(CSRC, d, ignore=shutil.ignore_patterns("*.o", "*.so", "*.so.*", "*.a"))
        path = os.path.join(d, fname)
        text = open(path).read()
        if text.count(old) != 1:              # a refactor moved the line: the entry must follow it
            return name, None, f"{fname}: {old!r} occurs {text.count(old)} times, not once"
        with open(path, "w") as f:
            f.write(text.replace(old, new))
        r = build(cxx, os.path.join(d, "dump_host_check"), d)
        return name, os.path.join(d, "dump_host_check"), r.stderr[-3000:] if r.returncode else None

    with concurrent.futures.ThreadPoolExecutor(max(1, min(4, os.cpu_count() or 1))) as pool:
        return {name: (path, err) for name, path, err in pool.map(make, MUTATIONS)}


@pytest.mark.parametrize("name", [m[0] for m in MUTATIONS])
def test_mutation(mutants, name, tmp_path):
    """The one substitution makes a valid case fail: a wrong word or byte, or a sanitizer report."""
    path, err = mutants[name]
    assert err is None, err
    cases = valid_cases(tmp_path)
    rc, outs, stderr = run(path, cases)
    if rc != 0:
        assert "Sanitizer" in stderr or "runtime error" in stderr, stderr
        return
    assert len(outs) == len(cases)
    with pytest.raises(AssertionError):
        check_valid(cases, outs)
