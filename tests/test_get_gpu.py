"""GPU: the batched get (bsdb_db_*, bsdb_dev_db_*) -- key -> rank -> index.db
slot -> record -> value bytes.

All comparisons are exact.  Ground truth is what the test itself wrote (the
keys and values it put); for absent keys it is the existing lookup
(Mph.lookup_*(check=True)): rank -1 must give REJECTED, a rank >= 0
KEY_MISMATCH (approximate mode: FOUND with the slot's 8 bytes)."""
import os
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from locate_cases import header_rule  # noqa: E402  (the header's rule, restated once for the host and the GPU tests)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FOUND, REJECTED, KEY_MISMATCH, BAD_ADDR = 0, 1, 2, 3
N1, PARTS = 20_000, 3
LAST_P0 = (N1 - 1) // PARTS * PARTS  # the last record of partition 0 (record i goes to partition i % PARTS)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def pack(items):
    off = np.zeros(len(items) + 1, np.uint64)
    if items:
        off[1:] = np.cumsum([len(k) for k in items])
    return np.frombuffer(b"".join(items), np.uint8) if items else np.zeros(0, np.uint8), off


def check(res, status, values):
    """res: a get's dict; status / values: what every query must give."""
    status = np.asarray(status, np.uint8)
    assert np.array_equal(res["status"], status)
    vlen = np.array([len(v) for v in values], np.uint64)
    assert np.array_equal(res["voff"], np.concatenate([np.zeros(1, np.uint64), np.cumsum(vlen, dtype=np.uint64)]))
    assert res["values"].tobytes() == b"".join(values)
    rep = res["report"]
    assert rep == {"queries": len(status), "found": int((status == FOUND).sum()),
                   "rejected": int((status == REJECTED).sum()), "key_mismatch": int((status == KEY_MISMATCH).sum()),
                   "bad_addr": int((status == BAD_ADDR).sum()), "value_bytes": int(vlen.sum())}


def absent_status(mph, keys):
    """REJECTED where the checked lookup gives -1, else KEY_MISMATCH; and the ranks."""
    r = mph.lookup_var(*pack(keys), check=True)
    return np.where(r < 0, REJECTED, KEY_MISMATCH).astype(np.uint8), r


@pytest.fixture(scope="module")
def source():
    """20 000 records: keys "1".."20000", values of 0..59 bytes, several of them empty.  The last record of
    partition 0 carries, as its VALUE, the header and key of a record of 65 535 value bytes (test 6 (c))."""
    rng = np.random.default_rng(11)
    keys = [str(i).encode() for i in range(1, N1 + 1)]
    vl = rng.integers(0, 60, N1)
    vl[[0, 7, 8, 500, 19_000]] = 0
    vals = [rng.integers(0, 256, int(l), dtype=np.uint8).tobytes() for l in vl]
    k = keys[LAST_P0]
    vals[LAST_P0] = bytes([len(k), 0xFF, 0xFF]) + k + bytes(range(20))
    absent = [b"a%d" % i for i in range(5_000)]
    return {"keys": keys, "vals": vals, "absent": absent}


@pytest.fixture(scope="module")
def dbs(source, tmp_path_factory):
    """The compact 3-partition database of `source`, exact or approximate: (directory, writer, Mph)."""
    _need_gpu()
    from bsdb_amd.writer import BSDBWriter
    cache = {}

    def get(approx=False):
        if approx not in cache:
            d = str(tmp_path_factory.mktemp(f"get_db_{int(approx)}"))
            w = BSDBWriter(d, checksum_bits=4, approximate_mode=approx, partitions=PARTS, fused_index=True)
            w.put_batch(*pack(source["keys"]), source["vals"])
            cache[approx] = (d, w, w.build())
        return cache[approx]

    yield get
    for _, w, mph in cache.values():
        mph.close()
        w.close()


def test_round_trip_compact_three_partitions(source, dbs):
    from bsdb_amd import BSDBReader
    d, w, mph = dbs()
    rng = np.random.default_rng(1)
    order = rng.permutation(N1)
    # present keys shuffled, the absent ones spread among them
    q = [source["keys"][i] for i in order] + source["absent"]
    truth = [source["vals"][i] for i in order] + [b""] * len(source["absent"])
    st_abs, _ = absent_status(mph, source["absent"])
    status = np.concatenate([np.zeros(N1, np.uint8), st_abs])
    mix = rng.permutation(len(q))
    q, truth, status = [q[i] for i in mix], [truth[i] for i in mix], status[mix]
    assert (status == REJECTED).sum() > 0 and (status == KEY_MISMATCH).sum() > 0  # cb = 4: both occur among 5 000
    with mph.open_db(os.path.join(d, "kv.db"), PARTS, os.path.join(d, "index.db")) as db:
        info = db.info()
        assert (info["n"], info["partitions"], info["format"], info["approximate"]) == (N1, PARTS, 0, 0)
        assert info["index_bytes"] == 8 * N1 and info["image_bytes"] >= sum(
            os.path.getsize(os.path.join(d, f"kv.db.{p}")) for p in range(PARTS))
        blob, off = pack(q)
        one = db.get_var(blob, off)
        check(one, status, truth)
        db.set_batch(1000)  # 25 chunks: the offsets stitch
        assert db.info()["batch"] == 1000
        chunked = db.get_var(blob, off)
        check(chunked, status, truth)
        retried = db.get_var(blob, off, value_cap=10)  # BSDB_E2BIG, then once more with the reported size
        check(retried, status, truth)
        db.set_batch(0)
        check(db.get_var(*pack([])), [], [])  # nq = 0
    with BSDBReader(d) as r:  # hash.dump carries no checksum bits: absent keys end at the key compare
        assert r.approximate is False and r.partitions == PARTS
        for i in (0, 7, 1234, LAST_P0, N1 - 1):
            assert r.get(source["keys"][i]) == source["vals"][i]
        for k in source["absent"][:5] + [b"20001", b"0"]:
            assert r.get(k) is None
        res = r.get_batch(*pack([b"5", b"nope", b"6"]))
        assert res["values"].tobytes() == source["vals"][4] + source["vals"][5]
        assert res["status"][0] == FOUND and res["status"][1] != FOUND and res["status"][2] == FOUND


@pytest.fixture(scope="module")
def fixed_dbs(tmp_path_factory):
    """Fixed-length key sets behind their own one-partition compact database: key_len -> (keys, values, db)."""
    _need_gpu()
    from bsdb_amd import Context, kvfiles
    ctx = Context(0)
    cache = {}

    def get(key_len):
        if key_len in cache:
            return cache[key_len][:3]
        rng = np.random.default_rng(key_len)
        n = 300 if key_len == 255 else 5_000
        if key_len == 13:
            keys = ctx.gen_keys13(0, n).cpu().numpy().reshape(n, 13).copy()
            vals = [bytes([i & 0xFF]) for i in range(n)]  # 1-byte values: the 2.5 M-query output stays small
        else:
            keys = np.unique(rng.integers(0, 256, (n + 50, key_len), dtype=np.uint8), axis=0)[:n]
            keys = keys[rng.permutation(n)]
            vals = [rng.integers(0, 256, int(l), dtype=np.uint8).tobytes() for l in rng.integers(0, 21, n)]
        assert keys.shape == (n, key_len)
        d = str(tmp_path_factory.mktemp(f"get_fixed_{key_len}"))
        kv = os.path.join(d, "kv.db")
        addr = kvfiles.write_compact(kv, 1, keys.reshape(-1), np.arange(n + 1, dtype=np.uint64) * key_len,
                                     *kvfiles.pack_values(vals))
        mph = ctx.mph_build_index_fixed(keys, key_len, 4, addr, os.path.join(d, "index.db"))
        db = mph.open_db(kv, 1, os.path.join(d, "index.db"))
        cache[key_len] = (keys, vals, db, mph)
        return keys, vals, db

    yield get
    for _, _, db, mph in cache.values():
        db.close()
        mph.close()
    ctx.close()


@pytest.mark.parametrize("key_len", [13, 8, 255])
def test_fixed_length_readers_and_the_wave_tail(fixed_dbs, key_len):
    keys, vals, db = fixed_dbs(key_len)
    rng = np.random.default_rng(5)
    for count in (0, 1, 63, 64, 65, 4_999):
        idx = rng.integers(0, keys.shape[0], count)
        res = db.get_fixed(keys[idx].reshape(-1), key_len)
        check(res, np.zeros(count, np.uint8), [vals[i] for i in idx])
    # an absent key of the same length among present ones
    odd = keys[:3].copy()
    odd[1, -1] ^= 0x5A
    res = db.get_fixed(odd.reshape(-1), key_len)
    assert res["status"][0] == FOUND and res["status"][2] == FOUND and res["status"][1] in (REJECTED, KEY_MISMATCH)
    assert res["values"].tobytes() == vals[0] + vals[2]


def test_more_queries_than_one_grid_has_threads(fixed_dbs):
    keys, vals, db = fixed_dbs(13)
    nq = 2_500_000
    idx = np.random.default_rng(6).integers(0, keys.shape[0], nq)
    res = db.get_fixed(keys[idx].reshape(-1), 13)
    assert not res["status"].any()
    assert np.array_equal(res["voff"], np.arange(nq + 1, dtype=np.uint64))
    assert np.array_equal(res["values"], (idx & 0xFF).astype(np.uint8))
    assert res["report"] == {"queries": nq, "found": nq, "rejected": 0, "key_mismatch": 0, "bad_addr": 0,
                             "value_bytes": nq}


def test_gather_edges_through_the_device_forms(tmp_path):
    _need_gpu()
    from bsdb_amd import Context, kvfiles
    from bsdb_amd.native import GET_WORDS
    n = 3_000
    rng = np.random.default_rng(3)
    vl = rng.integers(0, 12, n)
    vl[100], vl[101] = 65_535, 60_000   # the longest value, immediately followed by a long one
    vl[102:140] = 0                     # empty values after them
    vl[200:240] = 1                     # 40 consecutive 1-byte values: many sources in one 16-byte piece
    vl[240:340] = 0
    vl[300:340:2] = 1                   # 1-byte values with empty ones in between
    vl[400], vl[401], vl[402] = 16, 17, 0
    vl[0] = 0                           # the output starts with an empty value ...
    vl[n - 1] = 0                       # ... and ends with one
    keys = [b"k%d" % i for i in range(n)]
    vals = [rng.integers(0, 256, int(l), dtype=np.uint8).tobytes() for l in vl]
    kv, ip = str(tmp_path / "kv.db"), str(tmp_path / "index.db")
    kblob, koff = pack(keys)
    with Context(0) as ctx:
        addr = kvfiles.write_compact(kv, 1, kblob, koff, *kvfiles.pack_values(vals))
        with ctx.mph_build_index_var(kblob, koff, 4, addr, ip) as mph, mph.open_db(kv, 1, ip) as db:
            want = b"".join(vals)
            d_blob = torch.from_numpy(kblob.copy()).cuda()
            d_off = torch.from_numpy(koff.astype(np.int64)).cuda()
            report = torch.zeros(GET_WORDS, dtype=torch.int64, device="cuda")
            src, vlen, status, report = ctx.db_locate_var(db, d_blob, d_off, report=report)
            voff = ctx.edge_offsets(vlen)
            total = int(voff[n])
            assert total == len(want) and not status.any().item()
            assert np.array_equal(vlen.cpu().numpy(), vl) and np.array_equal(voff.cpu().numpy()[1:], np.cumsum(vl))
            assert report.cpu().tolist() == [n, n, 0, 0, 0, total]
            big = torch.full((5 + total + 43,), 0xA5, dtype=torch.uint8, device="cuda")
            out = ctx.db_gather(db, src, voff, values=big[5: 5 + total], value_bytes=total)
            torch.cuda.synchronize()
            got = big.cpu().numpy()
            assert out.data_ptr() == big.data_ptr() + 5
            assert got[5: 5 + total].tobytes() == want
            assert (got[:5] == 0xA5).all() and (got[5 + total:] == 0xA5).all()  # nothing written outside the output
            # a second locate accumulates into the same report
            ctx.db_locate_var(db, d_blob, d_off, src=src, vlen=vlen, status=status, report=report)
            assert report.cpu().tolist() == [2 * n, 2 * n, 0, 0, 0, 2 * total]
            check(db.get_var(kblob, koff), np.zeros(n, np.uint8), vals)  # the host form: the same bytes


@pytest.fixture(scope="module")
def short_located(tmp_path_factory):
    """Three queries with values of 1, 20 and 9 bytes, located once in a 50-record database: ctx, db and, for the
    first query alone and for all three, (src, voff, the value bytes)."""
    _need_gpu()
    from bsdb_amd import Context, kvfiles
    d = tmp_path_factory.mktemp("get_short")
    keys = [b"k%d" % i for i in range(50)]
    vals = [bytes(range(i, i + n)) for i, n in enumerate([1, 20, 9] + [5] * 47)]
    kv, ip = str(d / "kv.db"), str(d / "index.db")
    kblob, koff = pack(keys)
    with Context(0) as ctx:
        addr = kvfiles.write_compact(kv, 1, kblob, koff, *kvfiles.pack_values(vals))
        with ctx.mph_build_index_var(kblob, koff, 4, addr, ip) as mph, mph.open_db(kv, 1, ip) as db:
            cases = []
            for nq in (1, 3):
                qblob, qoff = pack(keys[:nq])
                src, vlen, status, _ = ctx.db_locate_var(db, torch.from_numpy(qblob.copy()).cuda(),
                                                         torch.from_numpy(qoff.astype(np.int64)).cuda())
                assert not status.any().item()
                cases.append((src, ctx.edge_offsets(vlen), b"".join(vals[:nq])))
            yield ctx, db, cases


@pytest.mark.parametrize("mis", range(16))
def test_gather_short_outputs_at_every_misalignment(short_located, mis):
    """A 1-byte and a 30-byte output at `mis` bytes past an aligned address, between guards: an output shorter than
    a piece, whose first piece is its last, and one of two or three pieces with both ends partial."""
    ctx, db, cases = short_located
    for src, voff, want in cases:
        assert len(want) in (1, 30)
        big = torch.full((mis + len(want) + 37,), 0xA5, dtype=torch.uint8, device="cuda")
        view = big[mis: mis + len(want)]
        assert view.data_ptr() % 16 == mis
        ctx.db_gather(db, src, voff, values=view, value_bytes=len(want))
        torch.cuda.synchronize()
        got = big.cpu().numpy()
        assert got[mis: mis + len(want)].tobytes() == want
        assert (got[:mis] == 0xA5).all() and (got[mis + len(want):] == 0xA5).all()


@pytest.mark.parametrize("block", [4096, 8192])
def test_blocked_layout(tmp_path, block):
    _need_gpu()
    from bsdb_amd import Context, kvfiles
    n, parts = 20_000, 2
    rng = np.random.default_rng(block)
    keys = [str(i).encode() for i in range(1, n + 1)]
    vl = rng.integers(0, 60, n)
    # partition 0's first ten records fill its first block to the last byte: the tenth ends at the block's end
    first = list(range(0, 20, parts))
    vl[first[:9]] = 400
    vl[first[9]] = block - sum(3 + len(keys[i]) + 400 for i in first[:9]) - 3 - len(keys[first[9]])
    vl[5_001] = 9_000  # larger than a block: a page-aligned block of its own
    vals = [rng.integers(0, 256, int(l), dtype=np.uint8).tobytes() for l in vl]
    kv, ip = str(tmp_path / "kv.db"), str(tmp_path / "index.db")
    kblob, koff = pack(keys)
    addr = kvfiles.write_blocked(kv, parts, kblob, koff, *kvfiles.pack_values(vals), block)
    a = int(addr[first[9]])
    assert (a & 0xFFFF) + 3 + len(keys[first[9]]) + int(vl[first[9]]) == block == ((a >> 48) & 0xFF) * 4096
    assert ((int(addr[5_001]) >> 48) & 0xFF) * 4096 == 12_288 and int(addr[5_001]) & 0xFFFF == 0
    with Context(0) as ctx:
        with ctx.kv_build_index(kv, parts, 4, ip, str(tmp_path / "index_a.db"), False, fmt=1, block_size=block) as mph:
            with mph.open_db(kv, parts, ip, fmt=1, block_size=block) as db:
                order = rng.permutation(n)
                res = db.get_var(*pack([keys[i] for i in order]))
                check(res, np.zeros(n, np.uint8), [vals[i] for i in order])
                st, _ = absent_status(mph, [b"x1", b"x2", b"x3"])
                check(db.get_var(*pack([b"x1", b"x2", b"x3"])), st, [b""] * 3)


def test_approximate_mode(source, dbs):
    d, w, mph = dbs(approx=True)
    index_a = np.fromfile(os.path.join(d, "index_a.db"), np.uint8).reshape(-1, 8)
    heads = [(v[:8] + bytes(8))[:8] for v in source["vals"]]  # W:140-142: value head, zero padding
    st_abs, r = absent_status(mph, source["absent"])
    status = np.concatenate([np.zeros(N1, np.uint8), np.where(r < 0, REJECTED, FOUND).astype(np.uint8)])
    truth = heads + [index_a[x].tobytes() if x >= 0 else b"" for x in r]  # false positives: the slot's raw bytes
    assert (r >= 0).sum() > 0 and (r < 0).sum() > 0
    with mph.open_db(None, 0, os.path.join(d, "index_a.db"), approximate=True) as db:
        assert db.info()["approximate"] == 1 and db.info()["image_bytes"] == 8 * N1
        check(db.get_var(*pack(source["keys"] + source["absent"])), status, truth)
        db.set_batch(777)
        check(db.get_var(*pack(source["keys"] + source["absent"])), status, truth)


def test_untrusted_index(source, dbs, tmp_path):
    from bsdb_amd import Context
    from bsdb_amd.native import BSDB_EVERIFY, BsdbError
    d0, w, mph = dbs()
    d = str(tmp_path / "copy")
    shutil.copytree(d0, d)
    kv, ip = os.path.join(d, "kv.db"), os.path.join(d, "index.db")
    files = [np.fromfile(f"{kv}.{p}", np.uint8) for p in range(PARTS)]
    assert all(f.size > 100_000 for f in files)
    keys, vals = source["keys"], source["vals"]
    rank = mph.lookup_var(*pack(keys), check=True)
    index = np.fromfile(ip, ">u8")
    addr = index[rank].astype(np.uint64)  # every record's own address
    assert (rank >= 0).all() and (addr[LAST_P0] >> np.uint64(56)) == 0
    status = np.zeros(N1, np.uint8)
    # (a) an offset past partition 0's end that still lies inside the image (partitions 1 and 2 follow it)
    ia = 3 * 100
    index[rank[ia]] = files[0].size + 64
    status[ia] = BAD_ADDR
    # (b) into the middle of other records of its own partition: the header's rule over the file bytes decides
    for ib, other, delta in ((3 * 200, 3 * 201, 1), (3 * 300 + 1, 3 * 301 + 1, 2), (3 * 400 + 2, 3 * 401 + 2, 4)):
        new = int(addr[other]) + delta
        index[rank[ib]] = new
        part, pos = new >> 56, new & ((1 << 56) - 1)
        status[ib] = header_rule(files[part], files[part].size, pos, keys[ib])
        assert status[ib] in (KEY_MISMATCH, BAD_ADDR)
    # (c) the last record of partition 0: its value parses as its own key with 65 535 value bytes, which would
    # run into partition 1; its slot points at the value's start
    k = keys[LAST_P0]
    pos = (int(addr[LAST_P0]) & ((1 << 56) - 1)) + 3 + len(k)
    assert pos + len(vals[LAST_P0]) == files[0].size
    assert header_rule(files[0], 1 << 40, pos, k) == FOUND and header_rule(files[0], files[0].size, pos, k) == BAD_ADDR
    index[rank[LAST_P0]] = pos
    status[LAST_P0] = BAD_ADDR
    index.tofile(ip)
    truth = [v if s == FOUND else b"" for v, s in zip(vals, status)]
    assert (status != FOUND).sum() == 5
    with mph.open_db(kv, PARTS, ip) as db:
        res = db.get_var(*pack(keys))
        check(res, status, truth)  # every other key is still FOUND; no byte of partition 1 for (c)
    # an index.db that is not 8 n bytes
    with open(ip, "ab") as f:
        f.write(bytes(8))
    with pytest.raises(BsdbError) as e:
        mph.open_db(kv, PARTS, ip)
    assert e.value.code == BSDB_EVERIFY
    index.tofile(ip)
    # a hash.dump whose E is no offset array: the open refuses it
    dump = np.fromfile(os.path.join(d, "hash.dump"), np.uint64)
    dump[4 + 3] = (dump[4 + 3] & np.uint64(0xFF << 56)) | np.uint64(1 << 40)  # E[3]'s offset far beyond E[4]'s
    dump.tofile(os.path.join(d, "hash.dump"))
    with Context(0) as ctx, ctx.mph_load(os.path.join(d, "hash.dump")) as bad:
        with pytest.raises(BsdbError) as e:
            bad.open_db(kv, PARTS, ip)
        assert e.value.code == BSDB_EVERIFY


def test_lifetime(source, dbs):
    from bsdb_amd import Context
    from bsdb_amd.native import BsdbError
    d, w, _ = dbs()
    blob, off = pack(source["keys"][:10])
    ctx = Context(0)
    mph = ctx.mph_load(os.path.join(d, "hash.dump"))
    db = mph.open_db(os.path.join(d, "kv.db"), PARTS, os.path.join(d, "index.db"))
    check(db.get_var(blob, off), np.zeros(10, np.uint8), source["vals"][:10])
    ctx.close()  # the context first: the db is detached
    for call in (lambda: db.get_var(blob, off), lambda: db.get_fixed(blob[:8], 4), lambda: db.set_batch(5)):
        with pytest.raises(BsdbError) as e:
            call()
        assert e.value.code == -22
    db.close()  # freeing stays safe, in either order
    mph.close()
    # and the MPHF freed before its db
    with Context(0) as ctx2:
        mph2 = ctx2.mph_load(os.path.join(d, "hash.dump"))
        db2 = mph2.open_db(os.path.join(d, "kv.db"), PARTS, os.path.join(d, "index.db"))
        mph2.close()
        with pytest.raises(BsdbError) as e:
            db2.get_var(blob, off)
        assert e.value.code == -22
        db2.close()
