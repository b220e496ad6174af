"""GPU: resident databases merged into a new directory (bsdb_db_merge,
bsdb_dev_db_merge_status, bsdb_dev_db_pack; Database.merge, bsdb_amd.merge and
its command line).

All comparisons are exact.  Ground truth is Python's: dicts of bytes -> bytes,
plus the slot order the existing checked lookup gives every key (the rank is
the slot), as tests/test_diff_gpu.py computes by_slot.  The output of
merge(base, delta, removed) is base's kept records in base's slot order, then
delta's in delta's slot order; the kv.db files are restated with
kvfiles.write_compact / write_blocked per run of the partition rule
(text_run_bound), and the device pack is compared byte for byte with the text
pack (the unchanged text kernels) fed the same records as text."""
import os
import shutil
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_check_gpu import flip, pack, rand_bytes  # noqa: E402
from test_diff_gpu import LENS, Side, build, lines_of  # noqa: E402

KEPT, REPLACED, REMOVED, BAD_SLOT, BAD_ADDR = range(5)
FOUND, REJECTED, KEY_MISMATCH, GET_BAD_ADDR = range(4)
N, NT = 5_000, 1_500
EINVAL, EFILE, EVERIFY = -22, -9, -74
FIELDS = ("base_slots", "kept", "replaced", "removed", "bad_slot", "bad_addr", "delta_slots", "delta_written", "delta_bad_slot",
          "out_records", "out_key_bytes", "out_value_bytes")
NOT_TEXT_VALUES = [b"a b", b"line\nfeed", b"carriage\rreturn", b"nul\x00byte", b" ", b"\n", b"\r\n", b"\x00" * 40, bytes(range(256))]


def is_text(b):
    return not any(c in b for c in b" \n\r")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def write_db(tmp, name, truth, partitions=1):
    """A compact database of arbitrary bytes (BSDBWriter: no text in between)."""
    from bsdb_amd.writer import BSDBWriter
    d = str(tmp / name)
    w = BSDBWriter(d, checksum_bits=4, partitions=partitions, fused_index=True)
    try:
        for k, v in truth.items():
            w.put(k, v)
        w.build(verify=True).close()
    finally:
        w.close()
    return d


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """A: 5 000 records, values of 1 .. 32 510 bytes, some NOT_TEXT; compact, one partition.  U: 200 new keys plus edits
    of A's (same length and other lengths); blocked, two partitions.  R: 291 of A's keys with arbitrary values, a few of
    them also in U.  At / Bt: 1 500 text-only records and an edit of them, for the diff -> merge loop and the text pack."""
    _need_gpu()
    from bsdb_amd import Context
    tmp = tmp_path_factory.mktemp("merge_db")
    a, u, r, at, bt = datasets()
    dirs = dict(A=write_db(tmp, "A", a), U=build(tmp, "U", u, partitions=2, layout="blocked"), R=build(tmp, "R", r, partitions=1),
                At=build(tmp, "At", at, partitions=1), Bt=build(tmp, "Bt", bt, partitions=2, layout="blocked", block_size=8192))
    ctx = Context(0)
    truths = dict(A=a, U=u, R=r, At=at, Bt=bt)
    sides = {n: Side(d, truths[n], ctx) for n, d in dirs.items()}
    yield dict(tmp=tmp, ctx=ctx, **sides)
    for s in sides.values():
        s.close()
    ctx.close()
    torch.cuda.empty_cache()


def datasets():
    rng = np.random.default_rng(2027)
    keys = [b"%d:" % i + rand_bytes(rng, rng.integers(0, 21)) for i in range(N)]
    lens = (LENS * 4 + [int(l) for l in rng.integers(1, 121, N)])[:N]
    a = {k: rand_bytes(rng, l) for k, l in zip(keys, lens)}
    for j, v in enumerate(NOT_TEXT_VALUES * 3):
        a[keys[100 + 37 * j]] = v + (rand_bytes(rng, 5000 * (j % 3)) if j % 3 else b"")
    a[b"key with spaces"] = b"plain"
    a[b"k\n\r"] = b"v\n"
    u = {}
    for i, k in enumerate(keys):
        if i % 23 == 3:
            u[k] = flip(a[k], len(a[k]) // 2) if is_text(a[k]) else rand_bytes(rng, len(a[k]))
        elif i % 23 == 4:
            u[k] = rand_bytes(rng, (len(a[k]) * 2) % 7000 + 1)
    for j in range(200):
        u[b"new%d:" % j + rand_bytes(rng, rng.integers(0, 9))] = rand_bytes(rng, LENS[j % len(LENS)] if j < 30 else rng.integers(1, 90))
    r_keys = [k for i, k in enumerate(keys) if i % 17 in (5, 6) and i % 23 not in (3, 4)][:285] + [k for k in u if k in a][:6]
    r = {k: rand_bytes(rng, 1 + i % 9) for i, k in enumerate(r_keys)}
    assert len(r) == 291 and sum(k in u for k in r) == 6 and sum(k not in a for k in u) == 200
    tkeys = [b"t%d:" % i + rand_bytes(rng, rng.integers(0, 12)) for i in range(NT)]
    at = {k: rand_bytes(rng, LENS[i % len(LENS)] if i < 45 else rng.integers(1, 200)) for i, k in enumerate(tkeys)}
    bt = {k: (v if i % 7 else v + b"+" if len(v) < 32510 else v[:-1]) for i, (k, v) in enumerate(at.items()) if i % 11 != 2}
    bt.update({b"tn%d" % j: rand_bytes(rng, 1 + j % 50) for j in range(120)})
    assert all(is_text(k + v) and 1 <= len(v) <= 32510 and len(k) <= 255 for d in (u, r, at, bt) for k, v in d.items()) and sum(not is_text(k + v) for k, v in a.items()) >= 20
    return a, u, r, at, bt


# ---- the restatement ---------------------------------------------------------------------------------------------

def merged_records(base, delta=None, removed=None):
    """(status per slot of base, the output's records in order)."""
    d, r = (delta.truth if delta else {}), (removed.truth if removed else {})
    status = [REPLACED if k in d else REMOVED if k in r else KEPT for k, _ in base.by_slot]
    out = [rec for rec, s in zip(base.by_slot, status) if s == KEPT] + (delta.by_slot if delta else [])
    return status, out


def report_of(status, out, delta=None):
    nd = len(delta.by_slot) if delta else 0
    return dict(zip(FIELDS, [len(status)] + [status.count(s) for s in range(5)] + [nd, nd, 0, len(out), sum(len(k) for k, _ in out),
                                                                                 sum(len(v) for _, v in out)]))


def run_bound(k, parts, p):
    return p * k // parts  # text_run_bound


def kv_files(tmp, name, records, parts, block_size=None):
    """The kv.db files of one pack of `records`: run p by the single-partition writer; (files' bytes, addresses)."""
    from bsdb_amd import kvfiles
    files, addr = [], []
    for p in range(parts):
        run = records[run_bound(len(records), parts, p): run_bound(len(records), parts, p + 1)]
        base = str(tmp / f"{name}.want.{p}")
        kb, ko = pack([k for k, _ in run])
        vb, vo = pack([v for _, v in run])
        a = kvfiles.write_compact(base, 1, kb, ko, vb, vo) if block_size is None else kvfiles.write_blocked(base, 1, kb, ko, vb, vo, block_size)
        files.append(open(base + ".0", "rb").read())
        addr += [int(x) | p << 56 for x in a]
    return files, addr


def do_merge(world, name, base, delta=None, removed=None, partitions=1, layout="compact", block_size=4096, approximate=False):
    """Database.merge into a fresh directory with config and hash.dump, opened as a Side on the shared context."""
    from bsdb_amd.builder import LAYOUTS, _write_config
    d = str(world["tmp"] / name)
    os.makedirs(d)
    kv, index, index_a = os.path.join(d, "kv.db"), os.path.join(d, "index.db"), os.path.join(d, "index_a.db")
    rep, mph = base.db.merge(kv, partitions, 4, index, index_a if approximate else None, approximate, LAYOUTS[layout], block_size,
                             delta.db if delta else None, removed.db if removed else None)
    try:
        _write_config(d, dict(records=rep["out_records"], key_bytes=rep["out_key_bytes"], value_bytes=rep["out_value_bytes"],
                              max_key_len=255, max_value_len=32510), approximate, 4, layout, block_size)
        mph.dump(os.path.join(d, "hash.dump"))
        ok = mph.verify_kv(kv, partitions, index, index_a, approximate, fmt=LAYOUTS[layout], block_size=block_size)
    finally:
        mph.close()
    return d, rep, ok


def check_content(world, d, out):
    """items() over all slots and get_var of every key give exactly `out`."""
    truth = dict(out)
    assert len(truth) == len(out)
    side = Side(d, truth, world["ctx"])
    try:
        got = list(side.reader.items())
        assert len(got) == len(out) and dict(got) == truth
        assert got == side.by_slot
        keys = list(truth)
        res = side.db.get_var(*pack(keys))
        assert not res["status"].any()
        vals, voff = res["values"].tobytes(), res["voff"].tolist()
        assert all(vals[voff[i]: voff[i + 1]] == truth[k] for i, k in enumerate(keys))
        return side
    except Exception:
        side.close()
        raise


# ---- rebuild, byte for byte ------------------------------------------------------------------------------------

@pytest.mark.parametrize("parts,layout,bs", [(1, "compact", None), (1, "blocked", 4096), (1, "blocked", 8192), (3, "compact", None),
                                             (3, "blocked", 4096)])
def test_rebuild_byte_for_byte(world, parts, layout, bs):
    A, tmp = world["A"], world["tmp"]
    name = f"re_{parts}_{layout}_{bs}"
    d, rep, ok = do_merge(world, name, A, partitions=parts, layout=layout, block_size=bs or 4096)
    status, out = merged_records(A)
    assert rep == report_of(status, out) and rep["kept"] == rep["out_records"] == len(A.truth) and ok["ok"]
    files, addr = kv_files(tmp, name, out, parts, bs)
    for p in range(parts):
        got = open(os.path.join(d, f"kv.db.{p}"), "rb").read()
        assert len(got) == len(files[p]) and got == files[p], p
    # the addresses index.db holds are those records' (slot = the new MPHF's rank of the key)
    side = check_content(world, d, out)
    try:
        index = np.fromfile(os.path.join(d, "index.db"), ">u8")
        rank = side.mph.lookup_var(*pack([k for k, _ in out]), check=True)
        assert index[rank].tolist() == addr
        assert sum(1 for k, v in out if not is_text(k + v)) >= 20                        # NOT_TEXT records went along
    finally:
        side.close()


def test_second_trip_of_the_piece_loop(world, tmp_path):
    """An image of more pieces than the pack's largest grid has threads (32 workgroups per CU): one byte over
    merge_second_trip_bytes, some workgroup goes round its piece loop again."""
    ctx = world["ctx"]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    second_trip = cus * 32 * 256 * 16 + 1                                                # merge_second_trip_bytes(0, cus)
    rng = np.random.default_rng(5)
    n = second_trip // (3 + 8 + 32510) + 40
    big = {b"big%05d" % i: rand_bytes(rng, 32510 - i % 3) for i in range(n)}
    side = Side(write_db(tmp_path, "big", big), big, ctx)
    try:
        world2 = dict(world, tmp=tmp_path)
        d, rep, ok = do_merge(world2, "big_out", side)
        files, _ = kv_files(tmp_path, "big", side.by_slot, 1)
        assert len(files[0]) > second_trip and ok["ok"] and rep["out_records"] == n
        assert open(os.path.join(d, "kv.db.0"), "rb").read() == files[0]
    finally:
        side.close()


# ---- merge -----------------------------------------------------------------------------------------------------

def test_merge_report_and_content(world):
    A, U, R = world["A"], world["U"], world["R"]
    status, out = merged_records(A, U, R)
    d, rep, ok = do_merge(world, "m_aur", A, U, R, partitions=2, layout="blocked", block_size=8192)
    want = report_of(status, out, U)
    assert rep == want and ok["ok"] and ok["records"] == len(out)
    assert rep["replaced"] == sum(k in A.truth for k in U.truth) > 400 and rep["removed"] == 285 and rep["delta_written"] == len(U.truth)
    assert rep["base_slots"] == rep["kept"] + rep["replaced"] + rep["removed"] and rep["out_records"] == rep["kept"] + rep["delta_written"]
    expected = {k: v for k, v in A.truth.items() if k not in R.truth}
    expected.update(U.truth)
    assert dict(out) == expected
    side = check_content(world, d, out)
    try:
        gone = [k for k in R.truth if k not in U.truth]
        assert len(gone) == 285 and side.db.get_var(*pack(gone))["status"].all()           # the removed keys are absent
    finally:
        side.close()
    # in chunks of 1 000 slots, packs under the smallest cap: the same content, another placement
    from bsdb_amd.native import DUMP_MAX_LINE
    for s in (A, U):
        s.db.set_batch(1000)
        s.db.set_text_chunk(DUMP_MAX_LINE)
    try:
        d2, rep2, ok2 = do_merge(world, "m_aur_chunks", A, U, R, partitions=2, layout="blocked", block_size=8192)
        assert rep2 == want and ok2["ok"]
        check_content(world, d2, out).close()
        d3, rep3, ok3 = do_merge(world, "m_aur_chunks_c", A, U, R, partitions=3)
        assert rep3 == want and ok3["ok"]
        check_content(world, d3, out).close()
    finally:
        for s in (A, U):
            s.db.set_batch(0)
            s.db.set_text_chunk(0)
    # delta alone and removed alone
    for name, dl, rm in (("m_au", U, None), ("m_ar", None, R)):
        st, o = merged_records(A, dl, rm)
        d4, rep4, ok4 = do_merge(world, name, A, dl, rm)
        assert rep4 == report_of(st, o, dl) and ok4["ok"]
        check_content(world, d4, o).close()


def test_diff_then_merge_gives_b(world):
    """The loop: A.diff(B) -> upsert / removed text -> two small databases -> merge(A, up, rm) holds what B holds."""
    from bsdb_amd.builder import build_text
    At, Bt, tmp, ctx = world["At"], world["Bt"], world["tmp"], world["ctx"]
    up, rm = str(tmp / "loop.upsert"), str(tmp / "loop.removed")
    res = At.db.diff(Bt.db, upsert=up, removed=rm)
    assert not res["identical"] and os.path.getsize(up) and os.path.getsize(rm)
    build_text(up, str(tmp / "loop_up"), partitions=1)
    build_text(rm, str(tmp / "loop_rm"), partitions=2, layout="blocked")
    upsert = dict(l.split(b" ", 1) for l in open(up, "rb").read().split(b"\n") if l)
    removed = dict(l.split(b" ", 1) for l in open(rm, "rb").read().split(b"\n") if l)
    s_up, s_rm = Side(str(tmp / "loop_up"), upsert, ctx), Side(str(tmp / "loop_rm"), removed, ctx)
    try:
        d, rep, ok = do_merge(world, "loop_out", At, s_up, s_rm, partitions=2)
        assert ok["ok"] and rep["out_records"] == len(Bt.truth)
        m = Side(d, Bt.truth, ctx)
        try:
            back = m.db.diff(Bt.db)
            assert back["identical"] and back["ab"]["same"] == back["ba"]["same"] == len(Bt.truth)
        finally:
            m.close()
    finally:
        s_up.close()
        s_rm.close()


# ---- the device forms by hand ------------------------------------------------------------------------------------

def guarded(nbytes, mis):
    """A uint8 view of `nbytes` bytes at `mis` past a 16-byte aligned address, between 0xA5 guard bytes."""
    buf = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    lead = 64 + (-buf.data_ptr()) % 16 + mis
    return buf, buf[lead: lead + nbytes], lead


def intact(buf, lead, written, nbytes):
    b = buf.cpu().numpy()
    return (b[:lead] == 0xA5).all() and (b[lead + written:] == 0xA5).all() and b.size == nbytes + 256


def dev_pack(ctx, side, first, count, parts, bs, mis, approximate=True):
    ksrc, klen, vsrc, vlen, st, _ = ctx.db_records(side.db, first, count)
    assert not st.any().item()
    records = sum(3 + len(k) + len(v) for k, v in side.by_slot[first: first + count])
    cap = (2 * records + parts * bs if bs else records) + 16                              # the header's bound, no more
    ibuf, image, ilead = guarded(cap, mis)
    bbuf, blob, blead = guarded(255 * count + 16, (mis + 5) % 16)
    sizes = [4096 * 3 * p for p in range(parts)]
    res = ctx.db_pack(side.db, ksrc, klen, vsrc, vlen, parts, sizes, approximate=approximate, count=count, image=image, blob=blob,
                      block_size=bs)
    torch.cuda.synchronize()
    assert intact(ibuf, ilead, sum(res["run_bytes"]), cap) and intact(bbuf, blead, res["blob"].numel(), 255 * count + 16)
    return res, sizes


def host(res):
    return dict(image=res["image"].cpu().numpy().tobytes(), run_bytes=res["run_bytes"], addr=[x & (2**64 - 1) for x in res["addr"].cpu().tolist()],
                blob=res["blob"].cpu().numpy().tobytes(), off=res["off"].cpu().tolist(), value8=res["value8"].cpu().tolist(),
                value_len=res["value_len"].cpu().tolist())


@pytest.mark.parametrize("bs", [None, 4096, 8192])
def test_device_pack_equals_the_text_pack(world, bs):
    """Text records: db_pack of a window = text_pack of the window's dump_text output through text_split."""
    ctx, At = world["ctx"], world["At"]
    edges = (0, 1, 63, 64, 65, NT - 1, NT)
    pairs = [(f, c) for f in edges for c in edges if c and f + c <= NT]
    for j, (first, count) in enumerate(pairs):
        parts, mis = (1, 2, 3)[j % 3], (1, 7, 8, 15, 0, 3)[j % 6]
        got, sizes = dev_pack(ctx, At, first, count, parts, bs, mis)
        ksrc, klen, vsrc, vlen, st, _ = ctx.db_records(At.db, first, count)
        text, st, _ = ctx.db_dump_text(At.db, ksrc, klen, vsrc, vlen, st)
        aligned = torch.zeros(text.numel() + 32, dtype=torch.uint8, device="cuda")
        aligned = aligned[(-aligned.data_ptr()) % 16:][: text.numel()]
        aligned.copy_(text)
        desc, rep = ctx.text_split(aligned)
        assert int(rep[1]) == count and not st.any().item()
        want = ctx.text_pack(aligned, desc, count, parts, sizes, approximate=True, block_size=bs)
        assert host(got) == host(want), (first, count, parts, bs)
    ksrc, klen, vsrc, vlen, _, _ = ctx.db_records(At.db, NT, 0)                           # the window at n: no record
    res = ctx.db_pack(At.db, ksrc, klen, vsrc, vlen, 2, [0, 4096], count=0, block_size=bs)
    assert res["run_bytes"] == [0, 0] and res["blob"].numel() == 0 and res["off"].cpu().tolist() == [0]


@pytest.mark.parametrize("bs", [None, 4096])
def test_device_pack_of_not_text_records(world, bs):
    """Records no text carries: the image against the writers' restatement, the heads against the values."""
    ctx, A, tmp = world["ctx"], world["A"], world["tmp"]
    hard = [i for i, (k, v) in enumerate(A.by_slot) if not is_text(k + v)]
    assert len(hard) >= 20
    for first in hard[:6]:
        first = max(0, first - 3)
        count, parts = 9, 2
        res, sizes = dev_pack(ctx, A, first, count, parts, bs, 5)
        recs = A.by_slot[first: first + count]
        got = host(res)
        files, addr = kv_files(tmp, f"nt_{first}_{bs}", recs, parts, bs)
        assert got["image"] == b"".join(files) and got["run_bytes"] == [len(f) for f in files]
        # the addresses start behind files of `sizes` bytes: compact adds the bytes, blocked the pages
        shift = [(s if bs is None else (s // 4096) << 16) for s in sizes]
        assert got["addr"] == [a + shift[a >> 56] for a in addr]
        assert got["blob"] == b"".join(k for k, _ in recs) and got["off"] == np.cumsum([0] + [len(k) for k, _ in recs]).tolist()
        assert got["value_len"] == [min(len(v), 8) for _, v in recs]
        assert [x & (2**64 - 1) for x in got["value8"]] == [int.from_bytes((v[:8] + bytes(8))[:8], "little") for _, v in recs]


def test_merge_status_every_combination(world):
    ctx = world["ctx"]
    combos = [(b, d, r) for b in (0, 1, 2, 7) for d in (0, 1, 2, 3, 9, 255) for r in (0, 1, 2, 3, 4, 200)] * 3
    base, delta, removed = (torch.tensor([c[i] for c in combos], dtype=torch.uint8, device="cuda") for i in range(3))

    def restate(b, d, r):
        if b not in (0, 2):
            return BAD_SLOT
        if (d is not None and d >= GET_BAD_ADDR) or (r is not None and r >= GET_BAD_ADDR):
            return BAD_ADDR
        return REPLACED if d == FOUND else REMOVED if r == FOUND else KEPT

    total = np.zeros(12, np.int64)
    report = torch.zeros(12, dtype=torch.int64, device="cuda")
    for use_d, use_r in ((True, True), (False, True), (True, False), (False, False)):
        st, report = ctx.db_merge_status(base, delta if use_d else None, removed if use_r else None, report=report)
        want = [restate(b, d if use_d else None, r if use_r else None) for b, d, r in combos]
        assert st.cpu().tolist() == want, (use_d, use_r)
        total[0] += len(want)
        for s in range(5):
            total[1 + s] += want.count(s)
    assert report.cpu().tolist() == total.tolist() and total[0] == total[1:6].sum() and (total[1:6] > 0).all()
    st, rep = ctx.db_merge_status(base[:0])
    assert st.numel() == 0 and not rep.any().item()


# ---- damage, approximate output, refusals, the command line ------------------------------------------------------------

def damaged_copy(side, tmp, name, slots):
    d = str(tmp / name)
    shutil.copytree(side.dir, d)
    ip = os.path.join(d, "index.db")
    index = np.fromfile(ip, ">u8")
    for s in slots:
        index[s] = (1 << 40) + 64 * s + 1          # an address outside the file
    index.tofile(ip)
    return d


def test_damaged_inputs_stop_the_merge(world, capsys):
    from bsdb_amd import merge as merge_module
    from bsdb_amd.native import BsdbError
    from bsdb_amd.reader import BSDBReader
    ctx, A, U, R, tmp = world["ctx"], world["A"], world["U"], world["R"], world["tmp"]
    bad_a = damaged_copy(A, tmp, "A_bad", [3, 2500, N - 1])
    # a slot of U that no key of the small base R ranks onto (hash.dump carries no checksum bits: an absent key gets
    # some slot's rank, and locate tests the slot's address before the key): the base pass never sees it
    hit = set(U.mph.lookup_var(*pack(list(R.truth)), check=True).tolist())
    slot_u = next(i for i, (k, _) in enumerate(U.by_slot) if k not in R.truth and i not in hit)
    bad_u = damaged_copy(U, tmp, "U_bad", [slot_u])
    # ... and one that a key of A ranks onto: locate in delta answers BAD_ADDR
    slot_u2 = next(i for i, (k, _) in enumerate(U.by_slot) if k in A.truth)
    bad_u2 = damaged_copy(U, tmp, "U_bad2", [slot_u2])
    for name, base_dir, delta_dir, field, count in (("dmg_a", bad_a, U.dir, "bad_slot", 3), ("dmg_u", R.dir, bad_u, "delta_bad_slot", 1),
                                                    ("dmg_u2", A.dir, bad_u2, "bad_addr", None)):
        out = str(tmp / name)
        os.makedirs(out)
        with BSDBReader(base_dir, ctx=ctx) as b, BSDBReader(delta_dir, ctx=ctx) as dl:
            with pytest.raises(BsdbError) as e:
                b.db.merge(os.path.join(out, "kv.db"), 1, 4, os.path.join(out, "index.db"), delta=dl.db)
        rep = e.value.merge_report
        assert e.value.code == EVERIFY and not os.path.exists(os.path.join(out, "index.db")), name
        assert (rep[field] == count) if count else (rep[field] >= 1), (name, rep)
        assert rep["base_slots"] == rep["kept"] + rep["replaced"] + rep["removed"] + rep["bad_slot"] + rep["bad_addr"]
        assert rep["out_records"] == rep["kept"] + rep["delta_written"]
    # the command line: 2 on a damaged input and no index file, 0 and a verified directory otherwise
    capsys.readouterr()
    out = str(tmp / "cli_bad")
    assert merge_module.main([bad_a, "-o", out, "--delta", U.dir]) == 2
    assert "bad_slot 3" in capsys.readouterr().out and not os.path.exists(os.path.join(out, "index.db"))
    out = str(tmp / "cli_ok")
    assert merge_module.main([A.dir, "-o", out, "--delta", U.dir, "--removed", R.dir, "-p", "2", "-l", "blocked", "-bs", "8192", "-v"]) == 0
    line = capsys.readouterr().out.strip()
    status, recs = merged_records(A, U, R)
    assert line == "  ".join(f"{k} {v}" for k, v in report_of(status, recs, U).items())
    check_content(world, out, recs).close()
    with BSDBReader(out, ctx=ctx) as rd:
        assert (rd.partitions, rd.db.info()["format"], rd.db.info()["block_size"]) == (2, 1, 8192)
    with pytest.raises(SystemExit):
        merge_module.main([A.dir, "-o", A.dir])
    with pytest.raises(SystemExit):
        merge_module.main([A.dir, "-o", U.dir + "/", "--delta", U.dir])


def test_approximate_output(world):
    A, U = world["A"], world["U"]
    status, out = merged_records(A, U)
    d, rep, ok = do_merge(world, "m_approx", A, U, partitions=2, approximate=True)
    assert ok["ok"] and rep == report_of(status, out, U)
    side = check_content(world, d, out)
    try:
        keys = [k for k, _ in out]
        heads = [(v[:8] + bytes(8))[:8] for _, v in out]
        with side.mph.open_db(None, 0, os.path.join(d, "index_a.db"), approximate=True) as db:
            res = db.get_var(*pack(keys))
            assert not res["status"].any() and res["values"].tobytes() == b"".join(heads)
    finally:
        side.close()


def test_refusals(world):
    from bsdb_amd import Context
    from bsdb_amd.builder import build_text
    from bsdb_amd.native import BsdbError
    from bsdb_amd.reader import BSDBReader
    ctx, A, U, tmp = world["ctx"], world["A"], world["U"], world["tmp"]
    out = str(tmp / "refused")
    os.makedirs(out)
    kv, index = os.path.join(out, "kv.db"), os.path.join(out, "index.db")

    def refused(call, code=EINVAL):
        with pytest.raises(BsdbError) as e:
            call()
        assert e.value.code == code

    text, d = str(tmp / "approx.txt"), str(tmp / "approx")
    with open(text, "wb") as f:
        f.write(lines_of(list(world["At"].truth.items())[:200]))
    build_text(text, d, partitions=1, approximate=True)
    with BSDBReader(d, approximate=True, ctx=ctx) as ap:                                  # an approximate input, anywhere
        refused(lambda: ap.db.merge(kv, 1, 4, index))
        refused(lambda: A.db.merge(kv, 1, 4, index, delta=ap.db))
        refused(lambda: A.db.merge(kv, 1, 4, index, removed=ap.db))
    with Context(0) as other, BSDBReader(U.dir, ctx=other) as u2:                         # two contexts
        refused(lambda: A.db.merge(kv, 1, 4, index, delta=u2.db))
        refused(lambda: A.db.merge(kv, 1, 4, index, removed=u2.db))
    for parts, fmt, bs in ((0, 0, 4096), (129, 0, 4096), (1, 2, 4096), (1, 1, 0), (1, 1, 5000), (1, 1, 131072)):
        refused(lambda: A.db.merge(kv, parts, 4, index, fmt=fmt, block_size=bs))
    refused(lambda: A.db.merge(kv, 1, 4, index, approximate=True))                       # approximate without index_a_path
    refused(lambda: A.db.merge(kv, 1, 65, index))
    gone = BSDBReader(U.dir, ctx=ctx)
    gone.mph.close()
    refused(lambda: A.db.merge(kv, 1, 4, index, delta=gone.db))
    refused(lambda: gone.db.merge(kv, 1, 4, index))
    gone.close()
    assert not os.path.exists(kv + ".0") and not os.path.exists(index)                   # refused before any file is touched
    refused(lambda: A.db.merge(str(tmp / "no" / "such" / "kv.db"), 1, 4, index), EFILE)
    # the device pack's refusals: alignment, block size, part sizes, caps
    ksrc, klen, vsrc, vlen, _, _ = ctx.db_records(A.db, 0, 64)
    refused(lambda: ctx.db_pack(A.db, ksrc, klen, vsrc, vlen, 1, [0], block_size=5000))
    refused(lambda: ctx.db_pack(A.db, ksrc, klen, vsrc, vlen, 1, [100], block_size=4096))
    refused(lambda: ctx.db_pack(A.db, ksrc, klen, vsrc, vlen, 0, []))
    refused(lambda: ctx.db_pack(A.db, ksrc, klen, vsrc, vlen, 1, [0], image=torch.empty(64, dtype=torch.uint8, device="cuda")))
    refused(lambda: ctx.db_pack(A.db, ksrc, klen, vsrc, vlen, 1, [0], blob=torch.empty(8, dtype=torch.uint8, device="cuda")))
    # the ones that are left still answer
    assert ctx.db_pack(A.db, ksrc, klen, vsrc, vlen, 1, [0])["run_bytes"] == [sum(3 + len(k) + len(v) for k, v in A.by_slot[:64])]
