"""GPU: a resident database enumerated by slot (bsdb_db_scan, bsdb_db_dump_text,
bsdb_dev_db_records, bsdb_dev_db_dump_lengths, bsdb_dev_db_dump_text;
Database.items / dump_text, BSDBReader.items / dump_text and its command line).

All comparisons are exact.  Ground truth is what the test wrote: the order is
the rank the existing checked lookup gives every key (the rank is the slot), a
record's line is key + separator + value + "\\n", and a record is text exactly
when tests/text_rule.py reads that line back as that one record.  For a
rewritten index.db the status and the record of a slot are a Python
restatement of the header's rule over the files' bytes."""
import os
import shutil
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import text_rule as R  # noqa: E402
from test_check_gpu import built, pack, rand_bytes  # noqa: E402,F401  (built: the fixture, a database of its own here)
from test_get_gpu import LAST_P0, N1, PARTS, dbs, source  # noqa: E402,F401  (dbs, source: fixtures)

OK, BAD_ADDR, NOT_TEXT = 0, 1, 2
U64 = (1 << 64) - 1
N = 5_000
EINVAL = -22


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def is_text(k, v, sep=b" "):
    recs, _ = R.restate(k + sep + v + b"\n", sep)
    return [(rk, rv) for _, rk, _, rv in recs] == [(k, v)]


def report_of(records, status, first=0, text=True):
    """The report of slots whose records (key, value; None: BAD_ADDR) and final statuses are these."""
    bad = [i for i, s in enumerate(status) if s]
    live = [r for r in records if r is not None]
    return dict(slots=len(status), ok=status.count(OK), bad_addr=status.count(BAD_ADDR), not_text=status.count(NOT_TEXT),
                key_bytes=sum(len(k) for k, _ in live), value_bytes=sum(len(v) for _, v in live),
                text_bytes=sum(len(k) + len(v) + 2 for k, v in live) if text else 0, first_bad=first + bad[0] if bad else U64)


def check_items(res, records):
    """res: Database.items' dict; records: per slot (key, value), or None for a BAD_ADDR slot."""
    live = [r if r is not None else (b"", b"") for r in records]
    status = [OK if r is not None else BAD_ADDR for r in records]
    assert res["status"].tolist() == status
    for blob, off, j in ((res["keys"], res["koff"], 0), (res["values"], res["voff"], 1)):
        lens = np.array([len(r[j]) for r in live], np.uint64)
        assert np.array_equal(off, np.concatenate([np.zeros(1, np.uint64), np.cumsum(lens, dtype=np.uint64)]))
        assert blob.tobytes() == b"".join(r[j] for r in live)
    assert res["report"] == report_of(records, status, text=False)


@pytest.fixture(scope="module")
def reader(built):
    from bsdb_amd.reader import BSDBReader
    with BSDBReader(built["dir"]) as rd:
        yield rd
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def by_slot(built, reader):
    """The fixture's (key, value) pairs in slot order."""
    rank = reader.mph.lookup_var(*pack(built["keys"]), check=True)
    assert sorted(rank.tolist()) == list(range(N))
    order = np.argsort(rank)
    return [(built["keys"][i], built["vals"][i]) for i in order]


def lines_of(records, sep=b" "):
    return b"".join(k + sep + v + b"\n" for k, v in records)


# ---- round trip and order -----------------------------------------------------------------------------------------

def test_round_trip_and_order(built, reader, by_slot, tmp_path):
    from bsdb_amd.builder import build_text, check_text
    from bsdb_amd.reader import BSDBReader
    out = str(tmp_path / "dump.txt")
    rep = reader.dump_text(out)
    want = lines_of(by_slot)
    assert open(out, "rb").read() == want
    assert rep == report_of(by_slot, [OK] * N) and rep["text_bytes"] == os.path.getsize(out) and rep["first_bad"] == U64
    # the dump is the database's text: the check finds every record, and all of them
    res = check_text([out], built["dir"])
    assert res["ok"] and res["complete"] and res["check"]["ok"] == N and res["text"]["records"] == N
    # ... and a build from it, in the other layout and another partition count, holds the same records
    d2 = str(tmp_path / "db2")
    rep2 = build_text(out, d2, partitions=2, layout="blocked", verify=True)
    assert rep2["records"] == N
    with BSDBReader(d2) as rd2:
        out2 = str(tmp_path / "dump2.txt")
        assert rd2.dump_text(out2)["ok"] == N
        pairs2 = list(rd2.items())
    assert sorted(open(out2, "rb").read().splitlines()) == sorted(want.splitlines())
    assert sorted(pairs2) == sorted(by_slot)
    # the same records packed, and as pairs
    check_items(reader.db.items(), by_slot)
    assert list(reader.items(batch=1234)) == by_slot


def test_windows_and_chunks(reader, by_slot, tmp_path):
    from bsdb_amd.native import DUMP_MAX_LINE, BsdbError
    db, out = reader.db, str(tmp_path / "w.txt")
    edges = (0, 1, 63, 64, 65, N - 1, N)
    for first in edges:
        for count in sorted({c for c in edges if first + c <= N} | {N - first}):
            rep = db.dump_text(out, first=first, count=count)
            part = by_slot[first: first + count]
            assert open(out, "rb").read() == lines_of(part), (first, count)
            assert rep == report_of(part, [OK] * count, first), (first, count)
    check_items(db.items(64, 65), by_slot[64: 129])
    check_items(db.items(N, 0), [])
    # windows appended to one file are the whole
    open(out, "wb").write(b"stale")
    for i, (first, count) in enumerate(((0, 64), (64, 1), (65, N - 65), (N, 0))):
        db.dump_text(out, first=first, count=count, append=i > 0)
    whole = lines_of(by_slot)
    assert open(out, "rb").read() == whole
    # chunks of 1 000 slots, each cut to the smallest text chunk there is: the same bytes and the same report
    db.set_batch(1000)
    db.set_text_chunk(DUMP_MAX_LINE)
    try:
        assert db.dump_text(out) == report_of(by_slot, [OK] * N) and open(out, "rb").read() == whole
        check_items(db.items(), by_slot)
        check_items(db.items(key_cap=10, value_cap=10), by_slot)      # BSDB_E2BIG, then once more with the reported sizes
        check_items(db.items(key_cap=1 << 20, value_cap=10), by_slot)  # only the values are too many
        with pytest.raises(BsdbError) as e:
            db.set_text_chunk(DUMP_MAX_LINE - 1)
        assert e.value.code == EINVAL
    finally:
        db.set_batch(0)
        db.set_text_chunk(0)
    for call in (lambda: db.dump_text(out, first=1, count=N), lambda: db.dump_text(out, first=N + 1, count=0),
                 lambda: db.items(N - 1, 2), lambda: db.items(U64, 2), lambda: reader.ctx.db_records(db, 2, N - 1)):
        with pytest.raises(BsdbError) as e:
            call()
        assert e.value.code == EINVAL
    assert open(out, "rb").read() == whole                            # a refused call leaves the file alone


# ---- more than one trip of the grid-stride loops -----------------------------------------------------------------

def test_more_slots_than_one_grid_has_lanes(tmp_path):
    """1 100 000 records: the record kernels' grid is capped at CUs x 16 workgroups of 256 lanes, 1 048 576 on 256
    CUs, so this is the smallest round size that enters the second trip."""
    _need_gpu()
    from bsdb_amd import Context, kvfiles
    n = 1_100_000
    kv, ip, out = str(tmp_path / "kv.db"), str(tmp_path / "index.db"), str(tmp_path / "big.txt")
    with Context(0) as ctx:
        keys = ctx.gen_keys13(0, n).cpu().numpy().reshape(n, 13).copy()
        vals = (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)).view(np.uint8).reshape(n, 8)
        addr = kvfiles.write_compact(kv, 1, keys.reshape(-1), np.arange(n + 1, dtype=np.uint64) * 13, vals.reshape(-1),
                                     np.arange(n + 1, dtype=np.uint64) * 8)
        with ctx.mph_build_index_fixed(keys, 13, 4, addr, ip) as mph, mph.open_db(kv, 1, ip) as db:
            rank = mph.lookup_fixed(keys, 13, check=True)
            rows = np.empty((n, 23), np.uint8)
            rows[rank, :13], rows[rank, 13], rows[rank, 14:22], rows[rank, 22] = keys, 0x20, vals, 0x0A
            rep = db.dump_text(out)
            got = np.fromfile(out, np.uint8)
            assert got.size == 23 * n and np.array_equal(got.reshape(n, 23), rows)
            payload = np.delete(rows, (13, 22), axis=1)
            flagged = np.isin(payload, (0x20, 0x0A, 0x0D)).any(axis=1)  # 21 bytes, none empty: the bytes' part decides
            assert rep == dict(slots=n, ok=n - int(flagged.sum()), bad_addr=0, not_text=int(flagged.sum()), key_bytes=13 * n,
                               value_bytes=8 * n, text_bytes=23 * n, first_bad=int(np.flatnonzero(flagged)[0]) if flagged.any() else U64)
            res = db.items()
            assert np.array_equal(res["keys"].reshape(n, 13), rows[:, :13]) and np.array_equal(res["values"].reshape(n, 8), rows[:, 14:22])
            assert not res["status"].any() and res["report"]["slots"] == res["report"]["ok"] == n


# ---- edges through the device forms --------------------------------------------------------------------------------

def dev_dump(ctx, db, records, sep, first=0, mis=5):
    """The device forms over slots [first, first + len(records)): the descriptors against `records` (slot order),
    the packed keys and values by the get's scan and gather, the text into a misaligned view between guard bytes."""
    n = len(records)
    ksrc, klen, vsrc, vlen, status, rep1 = ctx.db_records(db, first, n)
    assert klen.cpu().tolist() == [len(k) for k, _ in records] and vlen.cpu().tolist() == [len(v) for _, v in records]
    assert not status.any().item()
    assert [x & U64 for x in rep1.cpu().tolist()] == list(report_of(records, [OK] * n, first, text=False).values())
    for src, ln, j in ((ksrc, klen, 0), (vsrc, vlen, 1)):
        off = ctx.edge_offsets(ln)
        assert ctx.db_gather(db, src, off).cpu().numpy().tobytes() == b"".join(r[j] for r in records)
    llen, loff = ctx.db_dump_lengths(db, klen, vlen, status)
    want = lines_of(records, sep)
    assert llen.cpu().tolist() == [len(k) + len(v) + 2 for k, v in records] and int(loff[n]) == len(want)
    big = torch.full((mis + len(want) + 43,), 0xA5, dtype=torch.uint8, device="cuda")
    text, status, rep2 = ctx.db_dump_text(db, ksrc, klen, vsrc, vlen, status, sep, first, text=big[mis: mis + len(want)],
                                          llen=llen, loff=loff)
    torch.cuda.synchronize()
    got = big.cpu().numpy()
    assert text.data_ptr() == big.data_ptr() + mis and text.data_ptr() % 16 == mis % 16
    assert got[mis: mis + len(want)].tobytes() == want
    assert (got[:mis] == 0xA5).all() and (got[mis + len(want):] == 0xA5).all()  # nothing written outside the text
    st = [OK if is_text(k, v, sep) else NOT_TEXT for k, v in records]
    assert status.cpu().tolist() == st
    assert [x & U64 for x in rep2.cpu().tolist()] == list(report_of(records, st, first).values())
    return st


def test_edges_through_the_device_forms(tmp_path):
    _need_gpu()
    from bsdb_amd import Context, kvfiles
    n = 3_000
    rng = np.random.default_rng(3)
    vl = rng.integers(0, 12, n)                # the value lengths of test_get_gpu's edge test
    vl[100], vl[101] = 65_535, 60_000
    vl[102:140] = 0
    vl[200:240] = 1
    vl[240:340] = 0
    vl[300:340:2] = 1
    vl[400], vl[401], vl[402] = 16, 17, 0
    vl[0] = vl[n - 1] = 0
    keys = [b"k%d" % i for i in range(n)]
    keys[500], keys[501] = b"K" * 255, b"L" * 254 + b"\t"
    vals = [rng.integers(0, 256, int(l), dtype=np.uint8).tobytes() for l in vl]
    kv, ip = str(tmp_path / "kv.db"), str(tmp_path / "index.db")
    kblob, koff = pack(keys)
    with Context(0) as ctx:
        addr = kvfiles.write_compact(kv, 2, kblob, koff, *kvfiles.pack_values(vals))
        with ctx.mph_build_index_var(kblob, koff, 4, addr, ip) as mph, mph.open_db(kv, 2, ip) as db:
            order = np.argsort(mph.lookup_var(kblob, koff, check=True))
            records = [(keys[i], vals[i]) for i in order]
            st = dev_dump(ctx, db, records, b"\t")
            assert st.count(NOT_TEXT) >= 150 and st.count(OK) > 2_000  # the empty values, the two long ones, stray bytes
            for first, count, mis in ((0, 1, 0), (1, 1, 15), (7, 40, 9), (n - 3, 3, 1)):
                dev_dump(ctx, db, records[first: first + count], b"\t", first, mis)
            out = str(tmp_path / "edges.txt")
            assert db.dump_text(out, "\t") == report_of(records, st) and open(out, "rb").read() == lines_of(records, b"\t")


@pytest.mark.parametrize("block", [4096, 8192])
def test_blocked_layout(tmp_path, block):
    _need_gpu()
    from bsdb_amd import Context, kvfiles
    n, parts = 4_000, 2
    rng = np.random.default_rng(block)
    keys = [str(i).encode() for i in range(1, n + 1)]
    vl = rng.integers(0, 60, n)
    first = list(range(0, 20, parts))          # partition 0's first ten records fill its first block to the last byte
    vl[first[:9]] = 400
    vl[first[9]] = block - sum(3 + len(keys[i]) + 400 for i in first[:9]) - 3 - len(keys[first[9]])
    vl[1_001] = 9_000                          # larger than a block: a page-aligned block of its own
    vals = [rand_bytes(rng, l) for l in vl]
    kv, ip = str(tmp_path / "kv.db"), str(tmp_path / "index.db")
    kblob, koff = pack(keys)
    addr = kvfiles.write_blocked(kv, parts, kblob, koff, *kvfiles.pack_values(vals), block)
    a = int(addr[first[9]])
    assert (a & 0xFFFF) + 3 + len(keys[first[9]]) + int(vl[first[9]]) == block == ((a >> 48) & 0xFF) * 4096
    assert ((int(addr[1_001]) >> 48) & 0xFF) * 4096 == 12_288
    with Context(0) as ctx:
        with ctx.kv_build_index(kv, parts, 4, ip, str(tmp_path / "index_a.db"), False, fmt=1, block_size=block) as mph:
            with mph.open_db(kv, parts, ip, fmt=1, block_size=block) as db:
                order = np.argsort(mph.lookup_var(kblob, koff, check=True))
                records = [(keys[i], vals[i]) for i in order]
                st = dev_dump(ctx, db, records, b"\t", mis=block // 4096)
                assert st.count(NOT_TEXT) >= int((vl == 0).sum()) > 0 and st.count(OK) > n // 2
                check_items(db.items(), records)


# ---- NOT_TEXT ---------------------------------------------------------------------------------------------------

def test_not_text(tmp_path):
    _need_gpu()
    from bsdb_amd import Context, kvfiles
    from bsdb_amd import reader as reader_module
    rng = np.random.default_rng(17)
    special = [(b"sep in key", b"v1"), (b"nl", b"a\nb"), (b"cr", b"ab\r"), (b"cr-first", b"\rab"), (b"sep-last", b"ab "),
               (b"sep-only", b" "), (b"empty", b""), (b"long", rand_bytes(rng, 32_511)), (b"longest-ok", rand_bytes(rng, 32_510)),
               (b"tab\tis\tno\tseparator\there", b"a\tb"), (b"nl\nkey", b"v")]
    recs = [(b"r%d" % i, rand_bytes(rng, rng.integers(1, 50))) for i in range(600)]
    for j, s in enumerate(special):
        recs.insert(37 + 50 * j, s)
    keys, vals = [k for k, _ in recs], [v for _, v in recs]
    kv, ip = str(tmp_path / "kv.db"), str(tmp_path / "index.db")
    kblob, koff = pack(keys)
    with Context(0) as ctx:
        addr = kvfiles.write_compact(kv, 3, kblob, koff, *kvfiles.pack_values(vals))
        with ctx.mph_build_index_var(kblob, koff, 4, addr, ip) as mph, mph.open_db(kv, 3, ip) as db:
            order = np.argsort(mph.lookup_var(kblob, koff, check=True))
            records = [recs[i] for i in order]
            st = dev_dump(ctx, db, records, b" ", mis=11)      # (the statuses there are the oracle's)
            flagged = {records[i] for i, s in enumerate(st) if s}
            assert flagged == set(special) - {special[8], special[9]}  # exactly those: 9 of the 11
            out = str(tmp_path / "raw.txt")
            rep = db.dump_text(out)
            assert open(out, "rb").read() == lines_of(records)  # every byte written raw
            assert rep == report_of(records, st) and rep["first_bad"] == st.index(NOT_TEXT) and rep["not_text"] == 9
            mph.dump(str(tmp_path / "hash.dump"))
    # the command line: the counts, and exit status 2 because the text does not carry the database
    with open(tmp_path / "config.properties", "w") as f:
        f.write("kv.compact=true\nindex.approximate=false\n")
    assert reader_module.main(["--dump", str(tmp_path / "cli.txt"), "-d", str(tmp_path)]) == 2
    assert open(tmp_path / "cli.txt", "rb").read() == lines_of(records)


def test_command_line(built, by_slot, tmp_path, capsys):
    from bsdb_amd import reader as reader_module
    out = str(tmp_path / "cli.txt")
    assert reader_module.main(["--dump", out, "-d", built["dir"], "--first", "10", "--count", "100"]) == 0
    assert open(out, "rb").read() == lines_of(by_slot[10:110])
    assert "slots 100  ok 100  bad_addr 0  not_text 0" in capsys.readouterr().out
    # with a tab as the separator the values that hold a tab do not read back: the counts say so, and the exit status
    st = [OK if is_text(k, v, b"\t") else NOT_TEXT for k, v in by_slot]
    assert 0 < st.count(NOT_TEXT) < N
    assert reader_module.main(["--dump", out, "-d", built["dir"], "-s", "\t"]) == 2
    assert open(out, "rb").read() == lines_of(by_slot, b"\t")
    assert f"slots {N}  ok {st.count(OK)}  bad_addr 0  not_text {st.count(NOT_TEXT)}" in capsys.readouterr().out


# ---- untrusted index.db ---------------------------------------------------------------------------------------

def slot_record(files, addr):
    """The (key, value) the header's rule gives for a compact address over the partition files' bytes, or None."""
    if addr >> 63 or addr >> 56 >= len(files):
        return None
    f, pos = files[addr >> 56], addr & ((1 << 56) - 1)
    if pos + 3 > f.size:
        return None
    klen, vlen = int(f[pos]), int(f[pos + 1]) << 8 | int(f[pos + 2])
    if pos + 3 + klen + vlen > f.size:
        return None
    return bytes(f[pos + 3: pos + 3 + klen]), bytes(f[pos + 3 + klen: pos + 3 + klen + vlen])


def test_untrusted_index(source, dbs, tmp_path):
    d0, w, mph = dbs()
    d = str(tmp_path / "copy")
    shutil.copytree(d0, d)
    kv, ip = os.path.join(d, "kv.db"), os.path.join(d, "index.db")
    files = [np.fromfile(f"{kv}.{p}", np.uint8) for p in range(PARTS)]
    keys, vals = source["keys"], source["vals"]
    rank = mph.lookup_var(*pack(keys), check=True)
    index = np.fromfile(ip, ">u8")
    addr = index[rank].astype(np.uint64)
    # the rewritten slots of test_get_gpu: past partition 0's end (inside the image), into the middle of records, the
    # crafted 65 535-byte record at partition 0's end; and the top bit set, a partition that does not exist
    index[rank[300]] = files[0].size + 64
    for ib, other, delta in ((600, 603, 1), (901, 904, 2), (1202, 1205, 4)):
        index[rank[ib]] = int(addr[other]) + delta
    k = keys[LAST_P0]
    pos = (int(addr[LAST_P0]) & ((1 << 56) - 1)) + 3 + len(k)
    assert pos + len(vals[LAST_P0]) == files[0].size
    index[rank[LAST_P0]] = pos
    index[rank[1500]] = (1 << 63) | int(addr[1500])
    index[rank[1501]] = (PARTS << 56) | 5
    index[rank[1502]] = (127 << 56) | 5
    index.tofile(ip)
    records = [slot_record(files, int(a)) for a in index]
    for i in (300, LAST_P0, 1500, 1501, 1502):
        assert records[rank[i]] is None
    own = np.ones(N1, bool)
    own[[300, 600, 901, 1202, LAST_P0, 1500, 1501, 1502]] = False
    for i in np.flatnonzero(own)[::97]:
        assert records[rank[i]] == (keys[i], vals[i])
    live = [r for r in records if r is not None]
    assert N1 - 8 <= len(live) <= N1 - 5
    with mph.open_db(kv, PARTS, ip) as db:
        check_items(db.items(), records)
        out = str(tmp_path / "u.txt")
        rep = db.dump_text(out)
        assert open(out, "rb").read() == lines_of(live)         # BAD_ADDR slots write nothing; no byte of partition 1
        st = [BAD_ADDR if r is None else OK if is_text(*r) else NOT_TEXT for r in records]
        assert rep == report_of(records, st) and rep["bad_addr"] == N1 - len(live)


# ---- refusals and lifetime ---------------------------------------------------------------------------------------

def test_approximate_database_is_refused(source, dbs, tmp_path):
    from bsdb_amd.native import BsdbError
    d, w, mph = dbs(approx=True)
    with mph.open_db(None, 0, os.path.join(d, "index_a.db"), approximate=True) as db:
        for call in (lambda: db.items(0, 10), lambda: db.dump_text(str(tmp_path / "a.txt"), count=10), lambda: db.set_text_chunk(0),
                     lambda: mph.ctx.db_records(db, 0, 10)):
            with pytest.raises(BsdbError) as e:
                call()
            assert e.value.code == EINVAL
    assert not os.path.exists(tmp_path / "a.txt")


def test_lifetime(source, dbs, tmp_path):
    from bsdb_amd import Context
    from bsdb_amd.native import BsdbError
    d, w, _ = dbs()
    out = str(tmp_path / "l.txt")
    ctx = Context(0)
    mph = ctx.mph_load(os.path.join(d, "hash.dump"))
    db = mph.open_db(os.path.join(d, "kv.db"), PARTS, os.path.join(d, "index.db"))
    rep = db.dump_text(out, count=10)
    assert (rep["slots"], rep["bad_addr"]) == (10, 0) and os.path.getsize(out) == rep["text_bytes"] > 0
    ctx.close()  # the context first: the db is detached
    for call in (lambda: db.items(0, 10), lambda: db.dump_text(out, count=10), lambda: db.set_text_chunk(0)):
        with pytest.raises(BsdbError) as e:
            call()
        assert e.value.code == EINVAL
    db.close()  # freeing stays safe, in either order
    mph.close()
    with Context(0) as ctx2:
        mph2 = ctx2.mph_load(os.path.join(d, "hash.dump"))
        db2 = mph2.open_db(os.path.join(d, "kv.db"), PARTS, os.path.join(d, "index.db"))
        mph2.close()  # the MPHF freed before its db
        for call in (lambda: db2.items(0, 10), lambda: db2.dump_text(out, count=10), lambda: ctx2.db_records(db2, 0, 10)):
            with pytest.raises(BsdbError) as e:
                call()
            assert e.value.code == EINVAL
        db2.close()
