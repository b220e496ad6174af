"""GPU: the text front end's blocked kv.db layout (bsdb_dev_text_pack_blocked,
bsdb_text_build_layout, bsdb_amd.builder with layout="blocked").

Ground truth is never the code under test: the records come from
tests/text_rule.py, and the bytes and addresses of every run are those of
``kvfiles.write_blocked`` (pinned to BlockedKVWriter's bytes by
tests/golden/make_blocked_fixture.py) over that run's records in one
partition, with the partition number and F / 4096 added to the addresses.  A
partition's file is its runs' oracle files back to back.  All comparisons are
exact.  Databases are read back with the existing scan, verifier, device
database and reader."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import text_rule as R  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAGE = 4096
GUARD = 0xA5
IGUARD = -0x5A5A5A5A5A5A5A5B
EINVAL, EDUP = -22, -17


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from bsdb_amd import Context
    c = Context(0)
    yield c
    c.close()
    torch.cuda.empty_cache()


# ---- records of a given size, texts, the oracle --------------------------------------------------------------

def record(i: int, size: int):
    """(key, value) of record i with 3 + len(key) + len(value) == size (5 .. 32 768); bytes that end no line and
    are no separator."""
    klen = 255 if size - 10 > R.MAX_VALUE else max(1, min(7, size - 4))
    key = (b"%07d" % (i % 10**7))[-klen:] if klen <= 7 else (b"%07d" % i).ljust(255, b"K")
    vlen = size - 3 - klen
    assert 1 <= vlen <= R.MAX_VALUE and len(key) == klen
    value = ((np.arange(vlen, dtype=np.uint32) * 7 + i) % 26 + 0x41).astype(np.uint8).tobytes()
    return key, value


def text_of(sizes):
    recs = [record(i, s) for i, s in enumerate(sizes)]
    return b"".join(k + b" " + v + b"\n" for k, v in recs), recs


def to_dev(text: bytes):
    t = torch.empty(len(text) + 16, dtype=torch.uint8, device="cuda")
    t[len(text):] = 0x20
    if text:
        t[:len(text)] = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def oracle_run(tmp, recs, p, B, F):
    """(file bytes, addresses) of one run: kvfiles.write_blocked over its records in one partition."""
    from bsdb_amd.kvfiles import pack_values, write_blocked
    if not recs:
        return b"", np.zeros(0, np.uint64)
    kblob, koff = pack_values([k for k, _ in recs])
    vblob, voff = pack_values([v for _, v in recs])
    base = os.path.join(tmp, "oracle.db")
    addr = write_blocked(base, 1, kblob, koff, vblob, voff, B)
    with open(base + ".0", "rb") as f:
        data = f.read()
    return data, addr + np.uint64((p << 56) + ((F // PAGE) << 16))


def oracle_chunk(tmp, recs, parts, B, sizes_before):
    """The chunk's image (the runs back to back), the runs' byte counts and the addresses in record order."""
    bound = R.run_bounds(len(recs), parts)
    image, runs, addr = b"", [], []
    for p in range(parts):
        data, a = oracle_run(tmp, recs[bound[p]:bound[p + 1]], p, B, sizes_before[p])
        image += data
        runs.append(len(data))
        addr.append(a)
    return image, runs, np.concatenate(addr) if addr else np.zeros(0, np.uint64)


def split(ctx, text):
    t = to_dev(text)
    desc, report = ctx.text_split(t, b" ", nbytes=len(text))
    torch.cuda.synchronize()
    return t, desc, int(report.cpu().numpy()[1])


def guarded_u8(n, lead):
    buf = torch.full((lead + n + 37,), GUARD, dtype=torch.uint8, device="cuda")
    return buf, buf[lead:lead + n]


def guarded_i64(n):
    buf = torch.full((n + 4,), IGUARD, dtype=torch.int64, device="cuda")
    lead = 1 if buf.data_ptr() % 16 == 0 else 2
    return buf, buf[lead:lead + n], lead


def prepare(ctx, sizes):
    """The text of records of these sizes, split on the device: (text bytes, records, text, descriptors, count)."""
    text, recs = text_of(sizes)
    t, desc, k = split(ctx, text)
    assert k == len(recs)
    return len(text), recs, t, desc, k


def check_pack(ctx, tmp, sizes, parts, B, before=None, prepared=None, lead=3):
    """Packs the records of `sizes` into blocks of B bytes, into an image view exactly as large as the oracle's
    image at a misaligned address (`lead` past an aligned one) between guard bytes and a guarded address array, and
    compares everything."""
    nbytes, recs, t, desc, k = prepared or prepare(ctx, sizes)
    before = before or [0] * parts
    image, runs, addr = oracle_chunk(str(tmp), recs, parts, B, before)
    ibuf, iview = guarded_u8(len(image), lead)
    abuf, aview, al = guarded_i64(max(k, 1))
    assert iview.data_ptr() % 16 == lead and aview.data_ptr() % 16 == 8
    out = ctx.text_pack(t, desc, k, parts, before, nbytes=nbytes, image=iview, addr=aview, block_size=B)
    torch.cuda.synchronize()
    assert out["run_bytes"] == runs and all(r % PAGE == 0 for r in runs)
    got = np.frombuffer(out["image"].cpu().numpy().tobytes(), np.uint8)
    want = np.frombuffer(image, np.uint8)
    assert got.size == want.size
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:5], got[bad[:5]], want[bad[:5]])
    ga = out["addr"].cpu().numpy().view(np.uint64)
    bad = np.flatnonzero(ga != addr)
    assert bad.size == 0, (bad[:5], [hex(int(x)) for x in ga[bad[:5]]], [hex(int(x)) for x in addr[bad[:5]]])
    h = ibuf.cpu().numpy()
    assert (h[:lead] == GUARD).all() and (h[lead + len(image):] == GUARD).all()
    h = abuf.cpu().numpy()
    assert (h[:al] == IGUARD).all() and (h[al + max(k, 1):] == IGUARD).all()
    return out


# ---- 1. the rule table ---------------------------------------------------------------------------------------

LARGE = (4097, 8192, 8193, 32768)
TABLE = {
    "exact_fill": [2048, 2048, 100, 3996, 7],          # two records fill a block exactly: no end mark, a new block
    "exact_fill_then_end": [100, 3996],
    "one_byte_too_long": [2048, 2049, 100],
    "exactly_B": [4096],
    "exactly_B_between": [100, 4096, 200, 4096, 4096, 5],
    "single": [100],
    "single_smallest": [5],
}
for L in LARGE:
    TABLE[f"large_{L}_between"] = [100, 200, L, 300, 3000, 1000]   # lands ahead of the block that is open
    TABLE[f"large_{L}_first"] = [L, 100, 200]
    TABLE[f"large_{L}_last"] = [100, 200, L]
    TABLE[f"large_{L}_twice"] = [100, L, L, 200]
    TABLE[f"large_{L}_only"] = [L, L, L]


@pytest.mark.parametrize("name", sorted(TABLE))
def test_rule_table(ctx, tmp_path, name):
    out = check_pack(ctx, tmp_path, TABLE[name], 1, PAGE)
    if name == "exact_fill":
        assert out["run_bytes"] == [3 * PAGE]
    if name.endswith("_between") and name.startswith("large"):
        a = out["addr"].cpu().numpy().view(np.uint64)
        page = (a >> np.uint64(16)) & np.uint64(0xFFFFFFFF)
        assert page[2] == 0 and page[0] == page[1] == page[3] > 0       # the large record's block comes first


def test_fewer_records_than_partitions(ctx, tmp_path):
    out = check_pack(ctx, tmp_path, [100, 5000, 7], 8, PAGE)
    assert out["run_bytes"].count(0) == 5


@pytest.mark.parametrize("mis", range(16))
def test_three_short_records_at_every_misalignment(ctx, tmp_path, mis):
    """The smallest blocked image, one block that three short records open, at every misalignment of the
    destination: its first and last pieces are partial at every one but 0."""
    out = check_pack(ctx, tmp_path, [5, 9, 12], 1, PAGE, lead=mis)
    assert out["run_bytes"] == [PAGE]


# ---- 2. tile and wave edges ----------------------------------------------------------------------------------

@pytest.mark.parametrize("sizes,parts", [([5] * 5000, 1), ([2049] * 3000, 1), ([20] * 3000, 3), ([5] * 5000, 3),
                                          ([9] * 2048 + [4000] + [9] * 2047, 2), ([5000] * 2100 + [7] * 10, 1)],
                         ids=["5000x5", "3000x2049", "bound_in_block_and_tile", "5000x5_3parts", "tile_sized", "tile_of_large"])
def test_tile_and_wave_edges(ctx, tmp_path, sizes, parts):
    """819 five-byte records a block: blocks straddle waves and the 2048-record tiles.  One 2049-byte record a
    block: the most block starts a tile can hold.  3 000 20-byte records in 3 runs: the run bounds 1000 and 2000
    fall inside what would be one block (204 records) and inside the first tile.  A tile that holds only large
    records has no block start at all."""
    check_pack(ctx, tmp_path, sizes, parts, PAGE)


# ---- 3. seeded random ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def random20000(ctx):
    rng = np.random.default_rng(97)
    cls = rng.choice(4, 20_000, p=[0.80, 0.14, 0.04, 0.02])
    sizes = np.where(cls == 0, rng.integers(5, 120, 20_000),
                     np.where(cls == 1, rng.integers(120, 4200, 20_000),
                              np.where(cls == 2, rng.integers(4000, 17000, 20_000), rng.integers(16000, 32769, 20_000))))
    sizes[[0, 1, 19_999]] = [32768, 5, 4096]
    sizes = [int(s) for s in sizes]
    return sizes, prepare(ctx, sizes)


@pytest.mark.parametrize("parts", [1, 3, 8])
@pytest.mark.parametrize("B", [4096, 8192, 16384, 65536])
def test_random_20000(ctx, tmp_path, random20000, B, parts):
    sizes, prepared = random20000
    assert min(sizes) == 5 and max(sizes) == 32768
    for before in ([0] * parts, [3 * PAGE] * parts):
        check_pack(ctx, tmp_path, sizes, parts, B, before, prepared)


# ---- 4. guards and refused arguments -------------------------------------------------------------------------

def test_refusals_write_nothing(ctx, tmp_path):
    from bsdb_amd.native import BsdbError
    sizes = [100, 200, 5000, 300]
    text, recs = text_of(sizes)
    t, desc, k = split(ctx, text)
    image, runs, addr = oracle_chunk(str(tmp_path), recs, 1, PAGE, [0])

    def refused(B=PAGE, before=(0,), n=len(image)):
        ibuf, iview = guarded_u8(n, 3)
        abuf, aview, _ = guarded_i64(k)
        with pytest.raises(BsdbError) as e:
            ctx.text_pack(t, desc, k, 1, list(before), nbytes=len(text), image=iview, addr=aview, block_size=B)
        assert e.value.code == EINVAL
        torch.cuda.synchronize()
        assert (ibuf.cpu().numpy() == GUARD).all() and (abuf.cpu().numpy() == IGUARD).all()   # the image too

    refused(n=len(image) - 1)                       # image_cap one byte short
    for B in (0, 4095, 6000, 69632):
        refused(B=B)
    refused(before=(100,))                          # F no multiple of 4096
    refused(before=(PAGE + 1,))
    refused(before=((1 << 44) - PAGE,))             # the run's 3 blocks would pass 2^44
    refused(before=(1 << 45,))
    check_pack(ctx, tmp_path, sizes, 1, PAGE, [(1 << 44) - len(image)], (len(text), recs, t, desc, k))   # ... exactly up to it


def test_other_outputs_equal_the_compact_pack(ctx):
    sizes = [100, 5, 4097, 300, 32768, 9] * 50
    text, recs = text_of(sizes)
    t, desc, k = split(ctx, text)
    a = ctx.text_pack(t, desc, k, 3, [0, 0, 0], approximate=True, nbytes=len(text))
    b = ctx.text_pack(t, desc, k, 3, [0, 0, 0], approximate=True, nbytes=len(text), block_size=PAGE)
    torch.cuda.synchronize()
    for name in ("blob", "off", "value8", "value_len"):
        assert torch.equal(a[name], b[name]), name
    assert a["blob"].cpu().numpy().tobytes() == b"".join(key for key, _ in recs)
    v8, vl = R.value_heads([(0, key, 0, v) for key, v in recs])
    assert np.array_equal(b["value8"].cpu().numpy().view(np.uint64), v8)
    assert np.array_equal(b["value_len"].cpu().numpy(), vl)


# ---- 5. streaming --------------------------------------------------------------------------------------------

CHUNK = 64 << 10


def chunks_of(data: bytes, chunk: int):
    """The chunks bsdb_text_build cuts a file of "\\n"-terminated lines into: a buffer of `chunk` bytes is cut
    after its last "\\n", the rest opens the next one."""
    out, pos, carry = [], 0, b""
    while pos < len(data) or carry:
        buf = carry + data[pos:pos + chunk - len(carry)]
        pos += len(buf) - len(carry)
        eof = pos >= len(data)
        cut = len(buf) if eof else buf.rindex(b"\n") + 1
        out.append(buf[:cut])
        carry = buf[cut:]
        if eof and not carry:
            break
    return out


def expected_files(tmp, datas, parts, B, chunk):
    """kv.db.<p> as the rule gives it: per chunk the runs of the partition rule, each run the oracle's file."""
    files = [b""] * parts
    per_part = [[] for _ in range(parts)]
    nchunks = 0
    for d in datas:
        for c in chunks_of(d, chunk):
            nchunks += 1
            recs = [(k, v) for _, k, _, v in R.restate(c, b" ")[0]]
            bound = R.run_bounds(len(recs), parts)
            for p in range(parts):
                run = recs[bound[p]:bound[p + 1]]
                files[p] += oracle_run(tmp, run, p, B, 0)[0]
                per_part[p] += run
    return files, per_part, nchunks


def stream_lines(n, seed, with_large):
    rng = np.random.default_rng(seed)
    lines = []
    for i in range(n):
        vlen = int(rng.integers(1, 120))
        if with_large and i % 97 == 5:
            vlen = int(rng.integers(4000, 20000))
        v = ((np.arange(vlen, dtype=np.uint32) * 3 + i) % 26 + 0x61).astype(np.uint8).tobytes()
        lines.append(b"s%d_%d " % (seed, i) + v)
        if i % 50 == 7:
            lines.append(b"junk%d" % i)
    return b"\n".join(lines) + b"\n"


def read_blocked(files, a):
    f = files[a >> 56]
    o = ((a >> 16) & 0xFFFFFFFF) * PAGE + (a & 0xFFFF)
    kl, vl = f[o], f[o + 1] << 8 | f[o + 2]
    return f[o + 3:o + 3 + kl], f[o + 3 + kl:o + 3 + kl + vl]


def test_streaming_one_chunk(ctx, tmp_path):
    parts = 3
    data = stream_lines(4000, 1, True)
    src = tmp_path / "in.txt"
    src.write_bytes(data)
    kv = str(tmp_path / "kv.db")
    mph, rep = ctx.text_build([str(src)], b" ", kv, parts, 4, str(tmp_path / "index.db"), str(tmp_path / "index_a.db"),
                              fmt=1, block_size=PAGE)
    want, per_part, nchunks = expected_files(str(tmp_path), [data], parts, PAGE, 256 << 20)
    assert rep["chunks"] == nchunks == 1 and rep["records"] == sum(len(x) for x in per_part)
    for p in range(parts):
        assert open(f"{kv}.{p}", "rb").read() == want[p], p
    v = mph.verify_kv(kv, parts, str(tmp_path / "index.db"), str(tmp_path / "index_a.db"), fmt=1, block_size=PAGE)
    assert v["ok"] and v["records"] == rep["records"]
    mph.close()


def test_streaming_many_chunks(ctx, tmp_path):
    from bsdb_amd.native import GET_FOUND, kv_scan
    parts, B = 3, PAGE
    datas = [stream_lines(5500, s, True) for s in (2, 3, 4)]
    assert all(900_000 < len(d) < 1_200_000 for d in datas)                  # three files of about 1 MB
    paths = []
    for i, d in enumerate(datas):
        paths.append(str(tmp_path / f"in{i}.txt"))
        open(paths[-1], "wb").write(d)
    kv = str(tmp_path / "kv.db")
    ctx.text_set_chunk(CHUNK)
    try:
        mph, rep = ctx.text_build(paths, b" ", kv, parts, 4, str(tmp_path / "index.db"), str(tmp_path / "index_a.db"),
                                  fmt=1, block_size=B)
    finally:
        ctx.text_set_chunk(0)
    want, per_part, nchunks = expected_files(str(tmp_path), datas, parts, B, CHUNK)
    assert rep["chunks"] == nchunks > 1
    files = [open(f"{kv}.{p}", "rb").read() for p in range(parts)]
    for p in range(parts):
        assert len(files[p]) % PAGE == 0 and len(files[p]) > 0
        assert files[p] == want[p], p
    # the scan: exactly the rule's records; a partition's small records in input order, and its large ones
    s = kv_scan(kv, parts, fmt=1, block_size=B)
    got = [[] for _ in range(parts)]
    for i, a in enumerate(s["addr"].tolist()):
        key, value = read_blocked(files, a)
        assert key == s["blob"][int(s["offsets"][i]):int(s["offsets"][i + 1])].tobytes()
        got[a >> 56].append((key, value))
    for p in range(parts):
        assert sorted(got[p]) == sorted(per_part[p])
        for large in (False, True):
            pick = lambda recs: [r for r in recs if (3 + len(r[0]) + len(r[1]) > B) == large]  # noqa: E731
            assert pick(got[p]) == pick(per_part[p]), (p, large)
    assert any(3 + len(k) + len(v) > B for k, v in per_part[0])
    v = mph.verify_kv(kv, parts, str(tmp_path / "index.db"), str(tmp_path / "index_a.db"), fmt=1, block_size=B)
    assert v["ok"] and v["records"] == rep["records"] == sum(len(x) for x in per_part)
    allrecs = [r for x in per_part for r in x]
    blob, off = pack_keys([k for k, _ in allrecs])
    with mph.open_db(kv, parts, str(tmp_path / "index.db"), fmt=1, block_size=B) as db:
        res = db.get_var(blob, off)
        assert (res["status"] == GET_FOUND).all()
        vo = res["voff"].astype(np.int64)
        vals = res["values"].tobytes()
        assert all(vals[vo[i]:vo[i + 1]] == allrecs[i][1] for i in range(len(allrecs)))
    mph.close()


def pack_keys(items):
    off = np.zeros(len(items) + 1, np.uint64)
    off[1:] = np.cumsum([len(k) for k in items])
    return np.frombuffer(b"".join(items), np.uint8), off


def test_compact_through_the_layout_call_is_the_same_files(ctx, tmp_path):
    data = stream_lines(3000, 5, False)
    src = tmp_path / "in.txt"
    src.write_bytes(data)
    L = __import__("bsdb_amd.native", fromlist=["lib"]).lib()
    import ctypes as C
    outs = []
    for name in ("old", "new"):
        d = tmp_path / name
        d.mkdir()
        arr = (C.c_char_p * 1)(os.fsencode(str(src)))
        report = (C.c_uint64 * 10)()
        h = C.c_void_p()
        tail = (4, 1, os.fsencode(str(d / "index.db")), os.fsencode(str(d / "index_a.db")), report, C.byref(h))
        if name == "old":
            rc = L.bsdb_text_build(ctx._h, arr, 1, 32, os.fsencode(str(d / "kv.db")), 3, *tail)
        else:
            rc = L.bsdb_text_build_layout(ctx._h, arr, 1, 32, os.fsencode(str(d / "kv.db")), 3, 0, 12345, *tail)
        assert rc == 0
        L.bsdb_mph_free(h)
        outs.append({f: open(d / f, "rb").read() for f in sorted(os.listdir(d))})
    assert outs[0].keys() == outs[1].keys() and len(outs[0]) == 5
    assert outs[0] == outs[1]
    assert sum(len(outs[0][f"kv.db.{p}"]) for p in range(3)) == sum(3 + len(k) + len(v) for _, k, _, v in R.restate(data, b" ")[0])


# ---- 6. end to end -------------------------------------------------------------------------------------------

N6, PARTS6 = 8_000, 3


@pytest.fixture(scope="module")
def source6():
    rng = np.random.default_rng(67)
    alpha = np.array([b for b in range(256) if b not in (0x0A, 0x0D, 0x20)], np.uint8)
    keys = [b"%d:" % i + alpha[rng.integers(0, alpha.size, int(rng.integers(0, 40)))].tobytes() for i in range(N6)]
    lens = rng.integers(1, 201, N6)
    lens[::500] = 6000                                                  # large records at B = 4096
    vals = [alpha[rng.integers(0, alpha.size, int(l))].tobytes() for l in lens]
    lines = [k + b" " + v for k, v in zip(keys, vals)] + [b"novalue ", b"", b"a b c"]
    return {"keys": keys, "vals": vals, "text": b"\n".join(lines) + b"\n"}


@pytest.mark.parametrize("approx", [False, True])
def test_end_to_end(ctx, tmp_path, source6, approx):
    from bsdb_amd.builder import build_text
    from bsdb_amd.native import GET_FOUND
    from bsdb_amd.reader import BSDBReader
    src = tmp_path / "in.txt"
    src.write_bytes(source6["text"])
    d = str(tmp_path / "db")
    rep = build_text(str(src), d, checksum_bits=4, approximate=approx, partitions=PARTS6, verify=True,
                     chunk_bytes=256 << 10, layout="blocked", block_size=PAGE)
    _, want = R.restate(source6["text"], b" ")
    assert {k: rep[k] for k in R.FIELDS} == want and rep["records"] == N6 and rep["chunks"] > 1
    cfg = dict(l.split(" = ") for l in open(os.path.join(d, "config.properties")).read().splitlines())
    assert cfg["kv.compact"] == "false" and cfg["kv.compress.block.size"] == str(PAGE) and cfg["kv.compressed"] == "false"
    assert all(os.path.getsize(os.path.join(d, f"kv.db.{p}")) % PAGE == 0 for p in range(PARTS6))
    blob, off = pack_keys(source6["keys"])
    with BSDBReader(d) as rd:
        res = rd.get_batch(blob, off)
        assert (res["status"] == GET_FOUND).all()
        vo = res["voff"].astype(np.int64)
        got = res["values"].tobytes()
        if approx:
            assert all(got[vo[i]:vo[i + 1]] == source6["vals"][i][:8].ljust(8, b"\0") for i in range(N6))
        else:
            assert all(got[vo[i]:vo[i + 1]] == source6["vals"][i] for i in range(N6))
            assert rd.get(b"absent") is None


def test_duplicate_key_is_named(ctx, tmp_path, source6):
    from bsdb_amd.builder import build_text
    from bsdb_amd.native import DuplicateKeyError
    lines = [k + b" " + v for k, v in zip(source6["keys"][:3000], source6["vals"][:3000])]
    lines.insert(2500, source6["keys"][17] + b" another_value")
    src = tmp_path / "dup.txt"
    src.write_bytes(b"\n".join(lines) + b"\n")
    with pytest.raises(DuplicateKeyError) as e:
        build_text([str(src)], str(tmp_path / "db"), partitions=PARTS6, chunk_bytes=CHUNK, layout="blocked")
    assert e.value.code == EDUP and e.value.keys == [source6["keys"][17]]
    assert e.value.report["found"] == 1


def test_cli_blocked_in_a_child_process(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    d = tmp_path / "in"
    d.mkdir()
    (d / "b.txt").write_bytes(b"k3,v3\nbad line\nbig," + b"x" * 9000 + b"\n")
    (d / "a.txt").write_bytes(b"k1,v1\r\nk2,v2")
    out = tmp_path / "db"
    r = subprocess.run([sys.executable, "-m", "bsdb_amd.builder", "-i", str(d), "-o", str(out), "-s", ",", "-cb", "8",
                        "-v", "-p", "2", "--layout", "blocked", "-bs", "8192"], cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "records=4" in r.stdout and "lines=5" in r.stdout and "not_two_fields=1" in r.stdout
    from bsdb_amd.reader import BSDBReader
    with BSDBReader(str(out)) as rd:
        assert [rd.get(k) for k in (b"k1", b"k2", b"k3", b"k4")] == [b"v1", b"v2", b"v3", None]
        assert rd.get(b"big") == b"x" * 9000
    cfg = (out / "config.properties").read_text()
    assert "kv.compact = false" in cfg and "kv.compress.block.size = 8192" in cfg
