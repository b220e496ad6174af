"""GPU: the fused database check (bsdb_dev_verify_*, bsdb_mph_verify_index_*,
bsdb_kv_verify_index) -- key -> rank -> index.db slot -> index_a.db bytes.

Expected counts never come from the code under test: they are numpy over the
ranks of the existing lookup kernel (Mph.lookup_var / Context.lookup), the
files' bytes and the records' addresses from kv_scan (``expected``)."""
import os
import shutil

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NONE = 2**64 - 1
N_DB = 100_003
PARTS = 3
BLOCK = 4096
COUNTERS = ("records", "rejected", "in_window", "wrong_addr", "wrong_value", "min_bad_addr")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def expected(mph, rec, index_path, index_a_path, approx):
    """The six counters restated in numpy from the existing lookup's ranks."""
    r = mph.lookup_var(rec["blob"], rec["offsets"], check=True)
    addr = rec["addr"]
    idx = np.fromfile(index_path, ">u8").astype(np.uint64)
    rej = r < 0
    ok = ~rej
    bad = rej.copy()
    wa = idx[r[ok]] != addr[ok]
    bad[ok] |= wa
    wv = np.zeros(int(ok.sum()), bool)
    if approx:
        ia = np.fromfile(index_a_path, np.uint8).reshape(-1, 8)
        v8 = np.ascontiguousarray(rec["value8"][ok]).view(np.uint8).reshape(-1, 8)
        live = np.arange(8)[None, :] < rec["vlen"][ok][:, None]  # bytes past vlen are not compared
        wv = ((ia[r[ok]] != v8) & live).any(axis=1)
        bad[ok] |= wv
    return {"records": int(r.size), "rejected": int(rej.sum()), "in_window": int(ok.sum()),
            "wrong_addr": int(wa.sum()), "wrong_value": int(wv.sum()),
            "min_bad_addr": int(addr[bad].min()) if bad.any() else NONE}


def counters(rep):
    return {k: rep[k] for k in COUNTERS}


class Db:
    """One built database: its directory (kv.db.<p>, index.db, index_a.db), the MPHF and its records."""

    def __init__(self, d, fmt, approx, mph, keep):
        self.dir, self.fmt, self.approx, self.mph, self.keep = d, fmt, approx, mph, keep
        self.n = N_DB

    def paths(self, d=None):
        d = d or self.dir
        return os.path.join(d, "kv.db"), os.path.join(d, "index.db"), os.path.join(d, "index_a.db")

    def records(self, d=None):
        from bsdb_amd.native import kv_scan
        return kv_scan(self.paths(d)[0], PARTS, self.fmt, BLOCK)

    def verify(self, d=None, windows=0, mph=None):
        kv, ip, ap = self.paths(d)
        return (mph or self.mph).verify_kv(kv, PARTS, ip, ap, self.approx, fmt=self.fmt, block_size=BLOCK,
                                           windows=windows)

    def copy(self, tmp_path):
        d = str(tmp_path / "copy")
        shutil.copytree(self.dir, d)
        return d


@pytest.fixture(scope="module")
def source():
    """n = 100 003 records: keys "1".."n", values of 0..59 bytes (vlen 0..8 all occur)."""
    rng = np.random.default_rng(7)
    keys = [str(i).encode() for i in range(1, N_DB + 1)]
    koff = np.zeros(N_DB + 1, np.uint64)
    koff[1:] = np.cumsum([len(k) for k in keys])
    vl = rng.integers(0, 60, N_DB)
    vl[:9] = np.arange(9)
    voff = np.zeros(N_DB + 1, np.uint64)
    voff[1:] = np.cumsum(vl)
    vblob = rng.integers(0, 256, int(voff[-1]), dtype=np.uint8)
    vals = [vblob[int(voff[i]): int(voff[i + 1])].tobytes() for i in range(N_DB)]
    return {"kblob": np.frombuffer(b"".join(keys), np.uint8), "koff": koff, "vblob": vblob, "voff": voff, "vals": vals}


@pytest.fixture(scope="module")
def dbs(source, tmp_path_factory):
    """Databases built on demand, once per (layout, approximate, from_files), shared by the module's tests:
    compact through BSDBWriter, blocked (4 096) through kvfiles.write_blocked and the context's builds."""
    from bsdb_amd import Context, kvfiles
    from bsdb_amd.native import kv_scan
    from bsdb_amd.writer import BSDBWriter
    cache, blocked_kv = {}, {}

    def get(layout="compact", approx=False, from_files=False):
        key = (layout, approx, from_files)
        if key in cache:
            return cache[key]
        d = str(tmp_path_factory.mktemp(f"db_{layout}_{int(approx)}_{int(from_files)}"))
        if layout == "compact":
            w = BSDBWriter(d, checksum_bits=4, approximate_mode=approx, partitions=PARTS, fused_index=True,
                           from_files=from_files)
            w.put_batch(source["kblob"], source["koff"], source["vals"])
            db = Db(d, 0, approx, w.build(), w)
        else:
            kv = os.path.join(d, "kv.db")
            if not blocked_kv:
                kvfiles.write_blocked(kv, PARTS, source["kblob"], source["koff"], source["vblob"], source["voff"], BLOCK)
                blocked_kv["dir"] = d
            else:
                for p in range(PARTS):
                    shutil.copyfile(os.path.join(blocked_kv["dir"], f"kv.db.{p}"), f"{kv}.{p}")
            ctx = Context(0)
            ip, ap = os.path.join(d, "index.db"), os.path.join(d, "index_a.db")
            if from_files:
                mph = ctx.kv_build_index(kv, PARTS, 4, ip, ap, approx, fmt=1, block_size=BLOCK)
            else:
                rec = kv_scan(kv, PARTS, 1, BLOCK)
                mph = ctx.mph_build_index_var(rec["blob"], rec["offsets"], 4, rec["addr"], ip, ap, approx,
                                              rec["value8"], rec["vlen"])
            db = Db(d, 1, approx, mph, ctx)
        cache[key] = db
        return db

    yield get
    for db in cache.values():
        db.mph.close()
        db.keep.close()


# ---- clean databases ----------------------------------------------------------

@pytest.mark.parametrize("from_files", [False, True])
@pytest.mark.parametrize("approx", [False, True])
@pytest.mark.parametrize("layout", ["compact", "blocked"])
def test_clean_database(dbs, layout, approx, from_files):
    """Every count is the same for 1, 3 and 7 windows (bounds at unaligned ranks: n = 100 003)."""
    _need_gpu()
    db = dbs(layout, approx, from_files)
    rec = db.records()
    kv, ip, ap = db.paths()
    exp = expected(db.mph, rec, ip, ap, approx)
    assert exp == {"records": N_DB, "rejected": 0, "in_window": N_DB, "wrong_addr": 0, "wrong_value": 0,
                   "min_bad_addr": NONE}
    for windows in (1, 3, 7):
        rep = db.verify(windows=windows)
        assert rep["ok"] and rep["flags"] == 0 and rep["windows"] == windows, rep
        assert counters(rep) == exp, (windows, rep)
        assert rep["records"] == rep["in_window"] == N_DB and rep["min_bad_addr"] == NONE
        # the same records from host memory
        rep = db.mph.verify_index_var(rec["blob"], rec["offsets"], rec["addr"], ip, ap, approx, rec["value8"],
                                      rec["vlen"], windows=windows)
        assert rep["ok"] and rep["windows"] == windows and counters(rep) == exp, (windows, rep)
    rep = db.verify(windows=0)  # sized by the device: one window here
    assert rep["ok"] and rep["windows"] == 1 and counters(rep) == exp


def _fixed_keys(key_len, n):
    import oracle as O
    if key_len == 13:
        return O.gen_keys13(31, n)
    k = np.zeros((n, key_len), np.uint8)  # distinct 16-byte keys
    k[:, :8] = np.arange(n, dtype=np.uint64).view(np.uint8).reshape(n, 8)
    k[:, 8:] = np.random.default_rng(3).integers(0, 256, (n, key_len - 8), dtype=np.uint8)
    return k.reshape(-1)


def _expected_fixed(mph, keys, key_len, addr, ip, ap, approx, v8, vl):
    n = keys.size // key_len
    rec = {"blob": keys, "offsets": np.arange(n + 1, dtype=np.uint64) * np.uint64(key_len), "addr": addr,
           "value8": v8, "vlen": vl}
    return expected(mph, rec, ip, ap, approx)


@pytest.mark.parametrize("key_len", [13, 16])
@pytest.mark.parametrize("approx", [False, True])
def test_fixed_keys(tmp_path, key_len, approx):
    """n = 4 501: 4 buckets, the 1 500 boundary touched on both sides; then one slot zeroed."""
    _need_gpu()
    from bsdb_amd import Context
    n = 4501
    rng = np.random.default_rng(key_len)
    keys = _fixed_keys(key_len, n)
    addr = rng.permutation(n).astype(np.uint64) * np.uint64(977) + np.uint64(1 << 56)
    v8 = rng.integers(0, 1 << 63, n, dtype=np.uint64)
    vl = rng.integers(0, 9, n).astype(np.uint8)
    ip, ap = str(tmp_path / "index.db"), str(tmp_path / "index_a.db")
    with Context(0) as ctx:
        mph = ctx.mph_build_index_fixed(keys, key_len, 4, addr, ip, ap, approx, v8, vl)
        assert mph.info()["num_buckets"] == 4
        exp = _expected_fixed(mph, keys, key_len, addr, ip, ap, approx, v8, vl)
        assert exp["in_window"] == n and exp["wrong_addr"] == exp["wrong_value"] == 0
        for windows in (1, 3):
            rep = mph.verify_index_fixed(keys, key_len, addr, ip, ap, approx, v8, vl, windows=windows)
            assert rep["ok"] and rep["windows"] == windows and counters(rep) == exp, rep
        r = mph.lookup_fixed(keys, key_len)
        with open(ip, "r+b") as f:
            f.seek(8 * int(r[1499]))
            f.write(bytes(8))
        exp = _expected_fixed(mph, keys, key_len, addr, ip, ap, approx, v8, vl)
        assert exp["wrong_addr"] == 1 and exp["min_bad_addr"] == int(addr[1499])
        rep = mph.verify_index_fixed(keys, key_len, addr, ip, ap, approx, v8, vl, windows=3)
        assert not rep["ok"] and rep["flags"] == 0 and counters(rep) == exp, rep
        mph.close()


@pytest.mark.parametrize("n", [0, 1])
@pytest.mark.parametrize("approx", [False, True])
def test_tiny_sets(tmp_path, n, approx):
    _need_gpu()
    from bsdb_amd import Context
    keys = _fixed_keys(13, n)
    addr = np.full(n, 0x0200000000000040, np.uint64)
    v8, vl = np.full(n, 0x1122334455667788, np.uint64), np.full(n, 3, np.uint8)
    ip, ap = str(tmp_path / "index.db"), str(tmp_path / "index_a.db")
    with Context(0) as ctx:
        mph = ctx.mph_build_index_fixed(keys, 13, 4, addr, ip, ap, approx, v8, vl)
        for windows in (0, 1, 7):
            rep = mph.verify_index_fixed(keys, 13, addr, ip, ap, approx, v8, vl, windows=windows)
            assert rep["ok"] and rep["flags"] == 0 and rep["windows"] == 1, rep
            assert counters(rep) == {"records": n, "rejected": 0, "in_window": n, "wrong_addr": 0, "wrong_value": 0,
                                     "min_bad_addr": NONE}
        mph.close()


# ---- index corruption -----------------------------------------------------------

def _ranks(db, rec):
    return db.mph.lookup_var(rec["blob"], rec["offsets"], check=True)


def test_swapped_and_zeroed_slots(dbs, tmp_path):
    _need_gpu()
    db = dbs("compact", False, True)
    d = db.copy(tmp_path)
    rec = db.records(d)
    r = _ranks(db, rec)
    kv, ip, ap = db.paths(d)
    i, j = 12_345, 77_777
    idx = np.fromfile(ip, ">u8")
    idx[[r[i], r[j]]] = idx[[r[j], r[i]]]
    idx.tofile(ip)
    exp = expected(db.mph, rec, ip, ap, False)
    assert exp["wrong_addr"] == 2 and exp["min_bad_addr"] == int(min(rec["addr"][i], rec["addr"][j]))
    for windows in (1, 3):
        rep = db.verify(d, windows=windows)
        assert not rep["ok"] and rep["flags"] == 0 and counters(rep) == exp, rep
    shutil.copyfile(db.paths()[1], ip)
    k = 50_001
    assert rec["addr"][k] != 0
    with open(ip, "r+b") as f:
        f.seek(8 * int(r[k]))
        f.write(bytes(8))
    exp = expected(db.mph, rec, ip, ap, False)
    assert exp["wrong_addr"] == 1 and exp["min_bad_addr"] == int(rec["addr"][k])
    rep = db.verify(d, windows=3)
    assert not rep["ok"] and counters(rep) == exp, rep


def test_value_bytes(dbs, tmp_path):
    """A byte inside the first vlen bytes is compared, a byte past vlen is not (W:141)."""
    _need_gpu()
    db = dbs("compact", True, False)
    d = db.copy(tmp_path)
    rec = db.records(d)
    r = _ranks(db, rec)
    kv, ip, ap = db.paths(d)
    short = np.flatnonzero((rec["vlen"] >= 1) & (rec["vlen"] < 8))
    i = int(short[1000])
    l = int(rec["vlen"][i])

    def flip(byte):
        with open(ap, "r+b") as f:
            f.seek(8 * int(r[i]) + byte)
            b = f.read(1)
            f.seek(-1, 1)
            f.write(bytes([b[0] ^ 0x40]))

    flip(l)  # past vlen: still clean
    exp = expected(db.mph, rec, ip, ap, True)
    assert exp["wrong_value"] == 0
    rep = db.verify(d, windows=3)
    assert rep["ok"] and counters(rep) == exp, rep
    flip(l - 1)  # the value's last compared byte
    exp = expected(db.mph, rec, ip, ap, True)
    assert exp["wrong_value"] == 1 and exp["wrong_addr"] == 0 and exp["min_bad_addr"] == int(rec["addr"][i])
    for windows in (1, 3):
        rep = db.verify(d, windows=windows)
        assert not rep["ok"] and rep["flags"] == 0 and counters(rep) == exp, rep


# ---- shape errors ----------------------------------------------------------------

@pytest.mark.parametrize("delta", [-8, 8])
@pytest.mark.parametrize("approx", [False, True])
def test_index_file_size(dbs, tmp_path, delta, approx):
    _need_gpu()
    db = dbs("compact", approx, False)
    d = db.copy(tmp_path)
    kv, ip, ap = db.paths(d)
    target = ap if approx else ip
    with open(target, "r+b") as f:
        f.truncate(8 * N_DB + delta)
    rep = db.verify(d)
    assert not rep["ok"] and rep["flags"] & 2 and rep["records"] == 0 and rep["windows"] == 0, rep


def test_missing_index_file_is_a_file_error(dbs, tmp_path):
    _need_gpu()
    from bsdb_amd.native import BsdbError
    db = dbs("compact", False, False)
    d = db.copy(tmp_path)
    os.remove(db.paths(d)[1])
    with pytest.raises(BsdbError) as e:
        db.verify(d)
    assert e.value.code == -9


def test_truncated_and_extended_partition(dbs, tmp_path):
    _need_gpu()
    db = dbs("compact", False, True)
    d = db.copy(tmp_path)
    kv, ip, ap = db.paths(d)
    rec = db.records(d)
    part, pos = rec["addr"] >> np.uint64(56), rec["addr"] & np.uint64((1 << 56) - 1)
    last = int(pos[part == 1].max())  # partition 1 cut before its last record
    with open(f"{kv}.1", "r+b") as f:
        f.truncate(last)
    exp = expected(db.mph, db.records(d), ip, ap, False)
    assert exp == {"records": N_DB - 1, "rejected": 0, "in_window": N_DB - 1, "wrong_addr": 0, "wrong_value": 0,
                   "min_bad_addr": NONE}
    rep = db.verify(d, windows=3)
    assert not rep["ok"] and rep["flags"] == 4 and counters(rep) == exp, rep
    # one extra record: rejected by its checksum, or accepted onto another record's slot
    shutil.copyfile(f"{db.paths()[0]}.1", f"{kv}.1")
    key, val = b"not-a-key-of-the-set", b"xyz"
    with open(f"{kv}.2", "ab") as f:
        f.write(bytes([len(key)]) + len(val).to_bytes(2, "big") + key + val)
    exp = expected(db.mph, db.records(d), ip, ap, False)
    assert exp["records"] == N_DB + 1 and exp["rejected"] + exp["wrong_addr"] == 1
    for windows in (1, 3):
        rep = db.verify(d, windows=windows)
        assert not rep["ok"] and rep["flags"] == 4 and counters(rep) == exp, rep


# ---- MPHF corruption (export -> edit -> import) ----------------------------------

def test_corrupted_mphf(dbs):
    """Only edits that keep every lookup in bounds: checksum bits, a values word, E[m]'s offset."""
    _need_gpu()
    db = dbs("compact", True, False)
    rec = db.records()
    kv, ip, ap = db.paths()
    E, vals, sb = db.mph.export()
    ctx = db.keep.ctx
    r = _ranks(db, rec)
    # one bit of one rank's checksum field
    i = 4242
    sb2 = sb.copy()
    bit = int(r[i]) * 4 + 2
    sb2[bit >> 6] ^= np.uint64(1 << (bit & 63))
    m2 = ctx.mph_import(N_DB, 4, E, vals, sb2)
    exp = expected(m2, rec, ip, ap, True)
    assert exp["rejected"] == 1 and exp["min_bad_addr"] == int(rec["addr"][i]) and exp["in_window"] == N_DB - 1
    rep = db.verify(mph=m2, windows=3)
    assert not rep["ok"] and rep["flags"] == 0 and counters(rep) == exp, rep
    m2.close()
    # one values word in the middle inverted: whatever the corrupted MPHF's own lookup says
    v2 = vals.copy()
    v2[v2.size // 2] ^= np.uint64(NONE)
    m3 = ctx.mph_import(N_DB, 4, E, v2, sb)
    exp = expected(m3, rec, ip, ap, True)
    assert exp["rejected"] + exp["wrong_addr"] > 0
    for windows in (1, 7):
        rep = db.verify(mph=m3, windows=windows)
        assert not rep["ok"] and rep["flags"] == 0 and counters(rep) == exp, rep
    m3.close()
    # E[m]'s offset n - 1: the structure is invalid, no record pass
    E2 = E.copy()
    E2[-1] = (E2[-1] & np.uint64(0xFF << 56)) | np.uint64(N_DB - 1)
    m4 = ctx.mph_import(N_DB, 4, E2, vals, sb)
    rep = db.verify(mph=m4)
    assert not rep["ok"] and rep["flags"] == 1 and rep["records"] == 0 and rep["windows"] == 0, rep
    m4.close()


@pytest.mark.parametrize("width", [0, 4, 13, 64])
def test_checksum_widths(tmp_path, width):
    """13-bit fields straddle words; width 0 has no checksum list at all."""
    _need_gpu()
    import oracle as O
    from bsdb_amd import Context
    n = 4501
    blob, off = O.gen_keys_var(9, n)
    rng = np.random.default_rng(width)
    addr = rng.permutation(n).astype(np.uint64) + np.uint64(5)
    v8 = rng.integers(0, 1 << 63, n, dtype=np.uint64)
    vl = rng.integers(0, 9, n).astype(np.uint8)
    ip, ap = str(tmp_path / "index.db"), str(tmp_path / "index_a.db")
    rec = {"blob": blob, "offsets": off, "addr": addr, "value8": v8, "vlen": vl}
    with Context(0) as ctx:
        mph = ctx.mph_build_index_var(blob, off, width, addr, ip, ap, True, v8, vl)
        exp = expected(mph, rec, ip, ap, True)
        rep = mph.verify_index_var(blob, off, addr, ip, ap, True, v8, vl, windows=3)
        assert rep["ok"] and counters(rep) == exp and exp["in_window"] == n, rep
        # absent keys: rejected by the checksum, or accepted onto a real record's slot
        blob2, off2 = O.gen_keys_var(10_000_000, 3000)
        a2 = np.arange(3000, dtype=np.uint64) + np.uint64(1 << 40)
        rec2 = {"blob": blob2, "offsets": off2, "addr": a2, "value8": v8[:3000], "vlen": vl[:3000]}
        exp = expected(mph, rec2, ip, ap, True)
        assert exp["rejected"] + exp["wrong_addr"] == 3000
        if width == 64:
            assert exp["rejected"] == 3000
        rep = mph.verify_index_var(blob2, off2, a2, ip, ap, True, v8[:3000], vl[:3000], windows=3)
        assert not rep["ok"] and rep["flags"] == 4 and counters(rep) == exp, rep
        mph.close()


# ---- device entry ------------------------------------------------------------------

def test_device_entry():
    """13-byte keys on the device, an interior window [1 000, 3 000) of n = 4 501, addresses by base + stride
    and by array; two calls over parts of the keys accumulate to one call's six words."""
    _need_gpu()
    from bsdb_amd import Context
    n, start, length, base, stride = 4501, 1000, 2000, 1 << 33, 24
    u64 = lambda t: [int(x) & NONE for x in t]
    with Context(0) as ctx:
        keys = ctx.gen_keys13(5, n)
        index = torch.zeros(n, dtype=torch.int64, device=keys.device)
        E, values, sigbits, _ = ctx.mph_build_index_passes(keys, 13, n, 4, addr_base=base, addr_stride=stride,
                                                            index=index)
        # spoil three slots: two inside the window, one outside it
        r = ctx.lookup(ctx.hash_fixed(keys, 13), n, E, values, 4, sigbits, check=True).cpu().numpy()
        assert np.array_equal(np.sort(r), np.arange(n))
        spoiled = [int(np.flatnonzero(r == q)[0]) for q in (1000, 2999, 3000)]
        index[[1000, 2999, 3000]] = 7
        torch.cuda.synchronize()
        addr = base + stride * np.arange(n, dtype=np.uint64)
        inw = (r >= start) & (r < start + length)
        exp = (n, 0, int(inw.sum()), 2, 0, int(addr[spoiled[:2]].min()))
        assert exp[2] == length
        win = index[start: start + length]
        kw = dict(start=start, length=length, width=4, sigbits=sigbits)
        got = ctx.verify_fixed(keys, 13, n, E, values, win, addr_base=base, addr_stride=stride, **kw)
        assert got == exp
        d_addr = torch.from_numpy(addr.view(np.int64)).to(keys.device)
        assert ctx.verify_fixed(keys, 13, n, E, values, win, addr=d_addr, **kw) == exp
        # two calls: keys [0, 2256) and [2256, n) (13 * 2256 bytes keeps the second part's 16-byte alignment)
        h = 2256
        out = ctx.verify_out(keys.device)
        ctx.verify_fixed(keys[: 13 * h], 13, n, E, values, win, addr_base=base, addr_stride=stride, out=out, **kw)
        got = ctx.verify_fixed(keys[13 * h:], 13, n, E, values, win, addr_base=base, addr_stride=stride, first=h,
                               out=out, **kw)
        assert got == exp and u64(out.cpu().tolist())[6:] == [0, 0]
        out = ctx.verify_out(keys.device)
        ctx.verify_fixed(keys[: 13 * h], 13, n, E, values, win, addr=d_addr[:h], out=out, **kw)
        assert ctx.verify_fixed(keys[13 * h:], 13, n, E, values, win, addr=d_addr[h:], out=out, **kw) == exp
        # the same keys as a var-len blob, with value slots
        off = torch.arange(n + 1, dtype=torch.int64, device=keys.device) * 13
        v8 = torch.arange(n, dtype=torch.int64, device=keys.device) * 0x0101010101010101
        vl = (torch.arange(n, device=keys.device) % 9).to(torch.uint8)
        rank = torch.from_numpy(r).to(keys.device)
        index_a = torch.zeros(n, dtype=torch.int64, device=keys.device)
        ctx.index_scatter(rank, d_addr, 0, n, torch.empty_like(index), v8, vl, index_a.view(torch.uint8))
        index_a[1500] ^= 1 << 60  # byte 7 of rank 1 500's slot: compared only if that record's vlen is 8
        torch.cuda.synchronize()
        hit = int(np.flatnonzero(r == 1500)[0])
        wv = 1 if hit % 9 == 8 else 0
        bad = [addr[s] for s in spoiled[:2]] + ([addr[hit]] if wv else [])
        exp_a = (n, 0, length, 2, wv, int(min(bad)))
        got = ctx.verify_var(keys, off, n, E, values, win, addr=d_addr, value8=v8, vlen=vl,
                             index_a=index_a[start: start + length], **kw)
        assert got == exp_a
        # an invalid E: no record is looked up, bit 0 of word 6
        E2 = E.clone()
        E2[-1] = n - 1
        out = ctx.verify_out(keys.device)
        got = ctx.verify_fixed(keys, 13, n, E2, values, win, addr=d_addr, out=out, **kw)
        assert got == (0, 0, 0, 0, 0, NONE) and u64(out.cpu().tolist())[6] == 1


# ---- the writer ----------------------------------------------------------------------

@pytest.mark.parametrize("approx", [False, True])
def test_writer_verify(tmp_path, approx):
    _need_gpu()
    from bsdb_amd.writer import BSDBWriter, VerifyError
    n = 20_011
    rng = np.random.default_rng(4)
    base = str(tmp_path / "db")
    w = BSDBWriter(base, checksum_bits=4, approximate_mode=approx, partitions=2, from_files=True)
    for i in range(1, n + 1):
        w.put(str(i).encode(), rng.integers(0, 256, int(rng.integers(0, 20)), dtype=np.uint8).tobytes())
    mph = w.build(verify=True)
    rep = w.verify(mph)
    assert rep["ok"] and rep["records"] == rep["in_window"] == n
    with open(os.path.join(base, "index.db"), "r+b") as f:
        f.seek(8 * 1234)
        f.write(b"\xff" * 8)
    with pytest.raises(VerifyError) as e:
        w.verify(mph)
    assert e.value.report["wrong_addr"] == 1 and not e.value.report["ok"]
    mph.close()
    w.close()
