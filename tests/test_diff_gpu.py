"""GPU: two resident databases compared on the device (bsdb_db_diff,
bsdb_dev_db_diff, bsdb_dev_db_select; Database.diff, BSDBReader.diff,
bsdb_amd.diff and its command line).

All comparisons are exact.  Ground truth is Python's: two dicts of bytes ->
bytes, plus the slot order the existing checked lookup gives every key (the
rank is the slot), as tests/test_dump_gpu.py computes by_slot.  A record of X
whose key Y holds is SAME, VALUE_LEN or VALUE_BYTES by comparing the two
values; a key Y does not hold gets the status Y's own checked lookup gives it
(REJECTED for rank -1, else KEY_MISMATCH), as restate in tests/test_check_gpu.py."""
import os
import shutil
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_check_gpu import flip, pack, rand_bytes  # noqa: E402

SAME, REJECTED, KEY_MISMATCH, BAD_ADDR, VALUE_LEN, VALUE_BYTES, BAD_SLOT = range(7)
NAMES = ("same", "rejected", "key_mismatch", "bad_addr", "value_len", "value_bytes", "bad_slot")
U64 = (1 << 64) - 1
N = 5_000
EINVAL = -22
LENS = [1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 100, 255, 4096, 32510]  # up to the text's limit
ABSENT, UPSERT = 0x06, 0x36


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def lines_of(records, sep=b" "):
    return b"".join(k + sep + v + b"\n" for k, v in records)


class Side:
    """A database directory open on the shared context: its dict, and its records in slot order."""

    def __init__(self, directory, truth, ctx, approximate=False):
        from bsdb_amd.reader import BSDBReader
        self.dir, self.truth = directory, truth
        self.reader = BSDBReader(directory, approximate=approximate, ctx=ctx)
        self.db, self.mph = self.reader.db, self.reader.mph
        keys = list(truth)
        rank = self.mph.lookup_var(*pack(keys), check=True)
        assert sorted(rank.tolist()) == list(range(len(keys)))
        self.by_slot = [(keys[i], truth[keys[i]]) for i in np.argsort(rank)]

    def close(self):
        self.reader.close()


def expected(x, y):
    """X -> Y: (status per slot of X, the report)."""
    absent = [k for k, _ in x.by_slot if k not in y.truth]
    ranks = dict(zip(absent, y.mph.lookup_var(*pack(absent), check=True).tolist())) if absent else {}
    status, compared = [], 0
    for k, v in x.by_slot:
        if k in y.truth:
            w = y.truth[k]
            st = VALUE_LEN if len(w) != len(v) else SAME if w == v else VALUE_BYTES
            compared += len(v) if len(w) == len(v) else 0
        else:
            st = REJECTED if ranks[k] < 0 else KEY_MISMATCH
        status.append(st)
    return status, report_of(status, compared)


def report_of(status, compared, first=0):
    diff = [i for i, s in enumerate(status) if s]
    return dict(slots=len(status), **{n: status.count(i) for i, n in enumerate(NAMES)},
                first_diff=first + diff[0] if diff else U64, compared_bytes=compared)


def build(tmp, name, truth, **kw):
    from bsdb_amd.builder import build_text
    text, d = str(tmp / f"{name}.txt"), str(tmp / name)
    with open(text, "wb") as f:
        f.write(lines_of(truth.items()))
    assert build_text(text, d, verify=True, **kw)["records"] == len(truth)
    return d


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """A: 5 000 records, compact, one partition.  B: A's dict with about 300 keys dropped, 200 new keys, same-length
    edits at the first, the last and a middle byte, and length changes; blocked, two partitions.  B0: B's text built
    without checksum bits.  A2: A's text in the other layout.  All open on one context."""
    _need_gpu()
    from bsdb_amd import Context
    tmp = tmp_path_factory.mktemp("diff_db")
    rng = np.random.default_rng(2026)
    keys = [b"%d:" % i + rand_bytes(rng, rng.integers(0, 21)) for i in range(N)]
    lens = (LENS * 4 + [int(l) for l in rng.integers(1, 121, N)])[:N]
    a = {k: rand_bytes(rng, l) for k, l in zip(keys, lens)}
    b, kinds = {}, {}
    for i, (k, v) in enumerate(a.items()):
        # the first four runs of LENS: kept, then edited at the first, the last and the middle byte; then by i mod 17
        kind = i // len(LENS) if i < 4 * len(LENS) else i % 17
        if kind == 0 and i >= 4 * len(LENS):
            kinds[k] = "dropped"
            continue
        if kind in (1, 2, 3):
            b[k] = flip(v, (0, len(v) - 1, len(v) // 2)[kind - 1])
            kinds[k] = "edited"
        elif kind == 4:
            b[k] = v + b"+"
            kinds[k] = "longer"
        elif kind == 5 and len(v) > 1:
            b[k] = v[:-1]
            kinds[k] = "shorter"
        else:
            b[k] = v
    for j in range(200):
        b[b"new%d:" % j + rand_bytes(rng, rng.integers(0, 9))] = rand_bytes(rng, LENS[j % len(LENS)] if j < 30 else rng.integers(1, 90))
    assert 290 <= sum(k == "dropped" for k in kinds.values()) <= 300 and len(b) - sum(k in a for k in b) == 200
    assert {len(v) for k, v in a.items() if kinds.get(k) == "edited"} >= set(LENS)
    dirs = dict(A=build(tmp, "A", a, partitions=1), B=build(tmp, "B", b, partitions=2, layout="blocked"),
                B0=build(tmp, "B0", b, partitions=2, layout="blocked", checksum_bits=0),
                A2=build(tmp, "A2", a, partitions=2, layout="blocked"))
    ctx = Context(0)
    sides = {n: Side(d, a if n[0] == "A" else b, ctx) for n, d in dirs.items()}
    yield dict(tmp=tmp, ctx=ctx, **sides)
    for s in sides.values():
        s.close()
    ctx.close()
    torch.cuda.empty_cache()


def delta_of(x, y, st_xy, st_yx):
    """(upsert, removed) records of the delta X -> Y."""
    return ([r for r, s in zip(y.by_slot, st_yx) if UPSERT >> s & 1], [r for r, s in zip(x.by_slot, st_xy) if ABSENT >> s & 1])


def check_diff(x, y, tmp, name):
    up, rm = str(tmp / f"{name}.upsert"), str(tmp / f"{name}.removed")
    res = x.db.diff(y.db, upsert=up, removed=rm)
    (st_xy, rep_xy), (st_yx, rep_yx) = expected(x, y), expected(y, x)
    assert res["ab"] == rep_xy and res["ba"] == rep_yx, (res, rep_xy, rep_yx)
    for f in ("same", "value_len", "value_bytes", "compared_bytes"):
        assert res["ab"][f] == res["ba"][f], f
    assert res["identical"] == (x.truth == y.truth)
    upsert, removed = delta_of(x, y, st_xy, st_yx)
    assert open(up, "rb").read() == lines_of(upsert) and open(rm, "rb").read() == lines_of(removed)
    for rep, recs, path in ((res["upsert"], upsert, up), (res["removed"], removed, rm)):
        assert (rep["slots"], rep["ok"], rep["bad_addr"], rep["not_text"], rep["first_bad"]) == (len(recs), len(recs), 0, 0, U64)
        assert rep["text_bytes"] == os.path.getsize(path)
    return res, upsert, removed


# ---- the host form: reports and the delta ------------------------------------------------------------------------

def test_reports_and_delta(world):
    from bsdb_amd.builder import check_text
    from bsdb_amd.native import DUMP_MAX_LINE
    A, B, tmp = world["A"], world["B"], world["tmp"]
    res, upsert, removed = check_diff(A, B, tmp, "ab")
    assert not res["identical"] and res["ab"]["first_diff"] == next(i for i, (k, v) in enumerate(A.by_slot) if B.truth.get(k) != v)
    assert res["ab"]["rejected"] + res["ab"]["key_mismatch"] == len(removed) == sum(k not in B.truth for k in A.truth) > 280
    assert res["ba"]["rejected"] + res["ba"]["key_mismatch"] == 200 and min(res["ab"]["value_len"], res["ab"]["value_bytes"]) > 400
    # the delta applied in Python gives B, and B holds every line of the upsert file
    applied = dict(A.truth)
    for k, _ in removed:
        del applied[k]
    applied.update(upsert)
    assert applied == B.truth
    chk = check_text([str(tmp / "ab.upsert")], B.dir)
    assert chk["ok"] and chk["check"]["ok"] == chk["text"]["records"] == len(upsert)
    # in chunks of 1 000 slots, the text in the smallest pieces there are: the same reports and the same files
    for s in (A, B):
        s.db.set_batch(1000)
        s.db.set_text_chunk(DUMP_MAX_LINE)
    try:
        res2, _, _ = check_diff(A, B, tmp, "ab_chunks")
        assert res2 == res
        # without files the diff reports are the same; the text reports are empty
        res3 = A.db.diff(B.db)
        assert (res3["ab"], res3["ba"]) == (res["ab"], res["ba"]) and res3["upsert"]["slots"] == res3["removed"]["slots"] == 0
    finally:
        for s in (A, B):
            s.db.set_batch(0)
            s.db.set_text_chunk(0)
    # the other way round is the inverse delta; another separator gives the same counts
    back, _, _ = check_diff(B, A, tmp, "ba")
    assert (back["ab"], back["ba"]) == (res["ba"], res["ab"])
    tab = A.reader.diff(B.reader, upsert=str(tmp / "tab.upsert"), separator="\t")
    assert (tab["ab"], tab["ba"]) == (res["ab"], res["ba"]) and open(tmp / "tab.upsert", "rb").read() == lines_of(upsert, b"\t")
    with pytest.raises(Exception) as e:
        A.db.diff(B.db, upsert=str(tmp / "no" / "such" / "dir" / "f"))
    assert e.value.code == -9


def test_without_checksum_bits(world):
    A, B0, tmp = world["A"], world["B0"], world["tmp"]
    res, _, removed = check_diff(A, B0, tmp, "ab0")
    absent = [k for k in A.truth if k not in B0.truth]
    ranks = B0.mph.lookup_var(*pack(absent), check=False)
    # nothing is rejected unless a rank is >= n
    assert res["ab"]["rejected"] == int((ranks >= len(B0.truth)).sum()) + int((ranks < 0).sum())
    assert res["ab"]["rejected"] + res["ab"]["key_mismatch"] == len(absent) == len(removed)
    assert res["ab"]["key_mismatch"] > res["ab"]["rejected"]


def test_identical(world, capsys):
    from bsdb_amd import diff as diff_module
    A, A2, B, tmp = world["A"], world["A2"], world["B"], world["tmp"]
    for other, name in ((A, "aa"), (A2, "aa2")):
        res, upsert, removed = check_diff(A, other, tmp, name)
        assert res["identical"] and not upsert and not removed
        assert os.path.getsize(tmp / f"{name}.upsert") == os.path.getsize(tmp / f"{name}.removed") == 0
        assert res["ab"]["same"] == res["ba"]["same"] == N and res["ab"]["first_diff"] == U64
        assert res["ab"]["compared_bytes"] == sum(len(v) for v in A.truth.values())
    # the command line: one line of counts per direction; 0 when identical, 2 when not
    capsys.readouterr()
    assert diff_module.main([A.dir, A2.dir, "--upsert", str(tmp / "cli.upsert"), "--removed", str(tmp / "cli.removed")]) == 0
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 2 and out[0].startswith(f"A->B  slots {N}  same {N}  rejected 0") and "first_diff none" in out[1]
    assert os.path.getsize(tmp / "cli.upsert") == os.path.getsize(tmp / "cli.removed") == 0
    assert diff_module.main([A.dir, B.dir, "--upsert", str(tmp / "cli.upsert"), "--removed", str(tmp / "cli.removed")]) == 2
    out = capsys.readouterr().out.splitlines()
    (st_ab, rep_ab), (st_ba, rep_ba) = expected(A, B), expected(B, A)
    # (the command line opens B on a context of its own: what its lookup rejects is the same function of the files)
    assert out[0].startswith(f"A->B  slots {N}  same {rep_ab['same']}  ") and out[1].startswith(f"B->A  slots {len(B.truth)}  same {rep_ba['same']}  ")
    upsert, removed = delta_of(A, B, st_ab, st_ba)
    assert open(tmp / "cli.upsert", "rb").read() == lines_of(upsert) and open(tmp / "cli.removed", "rb").read() == lines_of(removed)


# ---- the device forms by hand ---------------------------------------------------------------------------------

def dev_diff(ctx, x, y, first, count):
    """records -> gather keys -> locate in Y -> diff -> select over slots [first, first + count) of X."""
    ksrc, klen, vsrc, vlen, st_a, _ = ctx.db_records(x.db, first, count)
    if count:
        koff = ctx.edge_offsets(klen)
        blob = ctx.db_gather(x.db, ksrc, koff)
        src, vl, status, _ = ctx.db_locate_var(y.db, blob, koff)
    else:
        src, vl, status = (torch.empty(0, dtype=t, device="cuda") for t in (torch.int64, torch.int32, torch.uint8))
    status, rep = ctx.db_diff(x.db, y.db, vsrc, vlen, st_a, src, vl, status, slot_base=first)
    return (ksrc, klen, vsrc, vlen), status, [v & U64 for v in rep.cpu().tolist()]


def test_device_forms_on_windows(world):
    ctx, A, B = world["ctx"], world["A"], world["B"]
    st_all, _ = expected(A, B)
    edges = (0, 1, 63, 64, 65, N - 1, N)
    for first in edges:
        for count in sorted({c for c in edges if first + c <= N}):
            desc, status, rep = dev_diff(ctx, A, B, first, count)
            want = st_all[first: first + count]
            part = A.by_slot[first: first + count]
            assert status.cpu().tolist() == want, (first, count)              # record by record
            compared = sum(len(v) for (_, v), s in zip(part, want) if s in (SAME, VALUE_BYTES))
            assert rep == list(report_of(want, compared, first).values()), (first, count)
            for mask in (0, UPSERT, ABSENT, 0x3F, 1 << VALUE_LEN):
                sel, ksrc, klen, vsrc, vlen = ctx.db_select(A.db, status, mask, *desc)
                keep = [i for i, s in enumerate(want) if mask >> s & 1]
                assert sel.cpu().tolist() == keep, (first, count, mask)
                assert klen.cpu().tolist() == [len(part[i][0]) for i in keep] and vlen.cpu().tolist() == [len(part[i][1]) for i in keep]
                if mask == UPSERT and keep:
                    # the selection feeds the dump's text kernels unchanged, with a zeroed status array
                    zero = torch.zeros(len(keep), dtype=torch.uint8, device="cuda")
                    text, st, srep = ctx.db_dump_text(A.db, ksrc, klen, vsrc, vlen, zero)
                    assert text.cpu().numpy().tobytes() == lines_of([part[i] for i in keep]) and not st.any().item()
                    assert srep.cpu().tolist()[:4] == [len(keep), len(keep), 0, 0]
    # a report accumulates over windows into the whole
    rep = ctx.diff_report("cuda")
    for first, count in ((0, 64), (64, 1), (65, N - 65)):
        ksrc, klen, vsrc, vlen, st_a, _ = ctx.db_records(A.db, first, count)
        koff = ctx.edge_offsets(klen)
        src, vl, status, _ = ctx.db_locate_var(B.db, ctx.db_gather(A.db, ksrc, koff), koff)
        ctx.db_diff(A.db, B.db, vsrc, vlen, st_a, src, vl, status, slot_base=first, report=rep)
    assert dict(zip(expected(A, B)[1], [v & U64 for v in rep.cpu().tolist()])) == expected(A, B)[1]


# ---- untrusted index.db -------------------------------------------------------------------------------------

def test_untrusted_index(world):
    """A few slots of a copy of A's index.db name addresses outside the file: data is corrupted, not the process."""
    ctx, A, B, tmp = world["ctx"], world["A"], world["B"], world["tmp"]
    d = str(tmp / "A_bad")
    shutil.copytree(A.dir, d)
    ip = os.path.join(d, "index.db")
    index = np.fromfile(ip, ">u8")
    size = os.path.getsize(os.path.join(d, "kv.db.0"))
    in_b = [i for i, (k, _) in enumerate(A.by_slot) if k in B.truth]
    slots = [in_b[0], in_b[7], in_b[len(in_b) // 2], in_b[-1]]
    for s, addr in zip(slots, (size + 64, (1 << 63) | int(index[slots[1]]), (5 << 56) | 5, size - 1)):
        index[s] = addr
    index.tofile(ip)
    from bsdb_amd.reader import BSDBReader
    with BSDBReader(d, ctx=ctx) as bad:
        res = bad.db.diff(B.db, upsert=str(tmp / "bad.upsert"), removed=str(tmp / "bad.removed"))
        st_ab, _ = expected(A, B)
        want_ab = [BAD_SLOT if i in slots else s for i, s in enumerate(st_ab)]
        compared = sum(len(v) for (_, v), s in zip(A.by_slot, want_ab) if s in (SAME, VALUE_BYTES))
        assert res["ab"] == report_of(want_ab, compared) and res["ab"]["bad_slot"] == 4
        # B's records whose key lives in one of those slots find no whole record there
        # (nor does a key A never held whose rank in A happens to be one of them: the address is tested before the key)
        hit = {A.by_slot[s][0] for s in slots}
        new = [k for k, _ in B.by_slot if k not in A.truth]
        hit |= {k for k, r in zip(new, A.mph.lookup_var(*pack(new), check=True).tolist()) if r in slots}
        st_ba, _ = expected(B, A)
        want_ba = [BAD_ADDR if k in hit else s for (k, _), s in zip(B.by_slot, st_ba)]
        compared = sum(len(v) for (_, v), s in zip(B.by_slot, want_ba) if s in (SAME, VALUE_BYTES))
        assert res["ba"] == report_of(want_ba, compared) and res["ba"]["bad_addr"] == len(hit) >= 4
        for rep in (res["ab"], res["ba"]):
            assert rep["slots"] == sum(rep[n] for n in NAMES)
        # neither file holds a record of a damaged slot
        assert open(tmp / "bad.removed", "rb").read() == lines_of([r for r, s in zip(A.by_slot, want_ab) if ABSENT >> s & 1])
        assert open(tmp / "bad.upsert", "rb").read() == lines_of([r for r, s in zip(B.by_slot, want_ba) if UPSERT >> s & 1])
        # the device form says which slots
        ksrc, klen, vsrc, vlen, st_a, _ = ctx.db_records(bad.db, 0, N)
        koff = ctx.edge_offsets(klen)
        src, vl, status, _ = ctx.db_locate_var(B.db, ctx.db_gather(bad.db, ksrc, koff), koff)
        status, _ = ctx.db_diff(bad.db, B.db, vsrc, vlen, st_a, src, vl, status)
        assert status.cpu().tolist() == want_ab


# ---- refusals -----------------------------------------------------------------------------------------------

def test_refusals(world):
    from bsdb_amd import Context
    from bsdb_amd.builder import build_text
    from bsdb_amd.native import BsdbError
    from bsdb_amd.reader import BSDBReader
    ctx, A, B, tmp = world["ctx"], world["A"], world["B"], world["tmp"]

    def refused(call):
        with pytest.raises(BsdbError) as e:
            call()
        assert e.value.code == EINVAL

    # an approximate database, on either side
    text, d = str(tmp / "approx.txt"), str(tmp / "approx")
    with open(text, "wb") as f:
        f.write(lines_of(list(A.truth.items())[:200]))
    build_text(text, d, partitions=1, approximate=True)
    with BSDBReader(d, approximate=True, ctx=ctx) as ap:
        refused(lambda: A.db.diff(ap.db))
        refused(lambda: ap.db.diff(A.db))
    # two contexts
    with Context(0) as other, BSDBReader(B.dir, ctx=other) as b2:
        refused(lambda: A.db.diff(b2.db))
        refused(lambda: b2.db.diff(A.db, upsert=str(tmp / "never.upsert")))
    assert not os.path.exists(tmp / "never.upsert")                            # refused before any file is touched
    # a mask that names BAD_SLOT, or a status there is none of
    desc, status, _ = dev_diff(ctx, A, B, 0, 100)
    for mask in (0x40, 0x41, 0x80, 1 << 31):
        refused(lambda: ctx.db_select(A.db, status, mask, *desc))
    # a bad separator
    refused(lambda: A.db.diff(B.db, separator="\n"))
    # a freed MPHF, on either side
    gone = BSDBReader(B.dir, ctx=ctx)
    gone.mph.close()
    refused(lambda: A.db.diff(gone.db))
    refused(lambda: gone.db.diff(A.db))
    refused(lambda: ctx.db_diff(A.db, gone.db, *(torch.empty(0, dtype=t, device="cuda") for t in
                                                 (torch.int64, torch.int32, torch.uint8, torch.int64, torch.int32, torch.uint8))))
    gone.close()
    # the two that are left still answer
    assert A.db.diff(A.db)["identical"]
