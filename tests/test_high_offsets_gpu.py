"""GPU: addresses, image positions and text offsets beyond 32 bits.

Every 64-bit quantity of the read and write paths is taken out of its low 32
(or 31) bits, and compared exactly with a restatement that never shares code
with the kernels:

  A  the addresses both packs write (bsdb_dev_text_pack(_blocked),
     bsdb_dev_db_pack) for partitions that already hold 2^32 - 7 ... 2^56 -
     run bytes: kvfiles.write_compact / write_blocked per run of the
     partition rule, the partition and the prior bytes added in Python
     integers; the refusals one byte (one page) past the limits.
  B  a resident image above 4 GiB: a small database relocated by
     tests/high_cases.py so that 2^32 falls inside one record's header, key
     or value (compact) or inside a large record's block (blocked); every
     reader of the image -- records, get, locate + gather, items, dump,
     check, diff, merge -- gives what the unmoved original gives, and the
     original what Python's dict gives.
  C  text positions above 2^31: one chunk of 2^31 + 64 KiB bytes whose
     middle is a single line of "x"; the descriptors, the report, both packs
     and the check against tests/text_rule.py applied to the two ends.

The relocated files are holes: ftruncate + one pwrite, never 4 GiB of
writes.  An open reads the hole once (about 4 GiB of zeros per variant)."""
import os
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import high_cases as H  # noqa: E402
import locate_cases as L  # noqa: E402
import text_rule as R  # noqa: E402
from test_check_gpu import flip, pack, rand_bytes  # noqa: E402
from test_text_blocked_gpu import GUARD, IGUARD, guarded_i64, guarded_u8, to_dev  # noqa: E402
from test_text_gpu import join_lines, random_lines  # noqa: E402

PAGE = 4096
U64 = (1 << 64) - 1
EINVAL = -22
FOUND, REJECTED, KEY_MISMATCH, BAD_ADDR = range(4)
CHECK_VALUE_BYTES = 5
T32, T31 = 1 << 32, 1 << 31


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def ctx():
    _need_gpu()
    from bsdb_amd import Context
    c = Context(0)
    yield c
    c.close()
    torch.cuda.empty_cache()


def lines_of(records, sep=b" "):
    return b"".join(k + sep + v + b"\n" for k, v in records)


def is_text(k, v):
    recs, _ = R.restate(k + b" " + v + b"\n", b" ")
    return [(rk, rv) for _, rk, _, rv in recs] == [(k, v)]


def write_db(d, truth, partitions):
    """A compact database of arbitrary bytes (BSDBWriter: no text in between); record i goes to partition i % partitions."""
    from bsdb_amd.writer import BSDBWriter
    w = BSDBWriter(d, checksum_bits=4, partitions=partitions, fused_index=True)
    try:
        for k, v in truth.items():
            w.put(k, v)
        w.build(verify=True).close()
    finally:
        w.close()
    return d


def write_blocked_db(ctx, d, truth, partitions, block):
    """The same as blocked files: kvfiles.write_blocked, the index by the one-call build on the writer's addresses."""
    from bsdb_amd import kvfiles
    from bsdb_amd.builder import _write_config
    os.makedirs(d)
    kb, ko = pack(list(truth))
    vb, vo = pack(list(truth.values()))
    addr = kvfiles.write_blocked(os.path.join(d, "kv.db"), partitions, kb, ko, vb, vo, block)
    with ctx.mph_build_index_var(kb, ko, 4, addr, os.path.join(d, "index.db")) as mph:
        mph.dump(os.path.join(d, "hash.dump"))
        ok = mph.verify_kv(os.path.join(d, "kv.db"), partitions, os.path.join(d, "index.db"), fmt=1, block_size=block)
        assert ok["ok"] and ok["records"] == len(truth)
    _write_config(d, dict(records=len(truth), key_bytes=int(ko[-1]), value_bytes=int(vo[-1]), max_key_len=255, max_value_len=32510),
                  False, 4, "blocked", block)
    return d


def host_pack(res):
    return dict(image=res["image"].cpu().numpy().tobytes(), run_bytes=res["run_bytes"],
                addr=[x & U64 for x in res["addr"].cpu().tolist()], blob=res["blob"].cpu().numpy().tobytes(),
                off=res["off"].cpu().tolist())


def oracle_pack(tmp, name, records, parts, B):
    """The writers' restatement of one pack: run p of the partition rule through the single-partition writer.
    (image, run_bytes, every record's address in its run's own file, every record's run)."""
    from bsdb_amd import kvfiles
    bound = R.run_bounds(len(records), parts)
    image, runs, rel, run_of = b"", [], [], []
    for p in range(parts):
        run = records[bound[p]: bound[p + 1]]
        data, a = b"", []
        if run:
            base = os.path.join(tmp, f"{name}.{p}")
            kb, ko = pack([k for k, _ in run])
            vb, vo = pack([v for _, v in run])
            a = kvfiles.write_compact(base, 1, kb, ko, vb, vo) if B is None else kvfiles.write_blocked(base, 1, kb, ko, vb, vo, B)
            with open(base + ".0", "rb") as f:
                data = f.read()
            os.remove(base + ".0")
        image += data
        runs.append(len(data))
        rel += [int(x) for x in a]
        run_of += [p] * len(run)
    return image, runs, rel, run_of


def placed(rel, run_of, part_sizes, B):
    """The addresses behind files of part_sizes bytes, in Python integers: compact adds the bytes, blocked the pages."""
    return [a + (p << 56) + (part_sizes[p] if B is None else (part_sizes[p] // PAGE) << 16) for a, p in zip(rel, run_of)]


# ==== A. the addresses the packs write ============================================================================

N_A = 3000


FIVES = tuple(range(1, 40, 2))                                       # the records of 5 bytes: a key of one byte
B62 = b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz"


def sizes_a():
    rng = np.random.default_rng(2033)
    cls = rng.choice(4, N_A, p=[0.80, 0.14, 0.04, 0.02])
    sizes = np.where(cls == 0, rng.integers(6, 120, N_A),
                     np.where(cls == 1, rng.integers(120, 4200, N_A),
                              np.where(cls == 2, rng.integers(4000, 17000, N_A), rng.integers(16000, 32769, N_A))))
    sizes[list(FIVES)] = 5
    sizes[[0, 2, 4, 6, N_A - 1]] = [32768, 4096, 4097, 8193, 8192]
    return [int(s) for s in sizes]


def record_a(i, size):
    """(key, value) of record i with 3 + len(key) + len(value) == size, as text_blocked's `record`, but the keys
    are distinct: the last digits of i in base 62 (two of them tell 3 844 records apart), one letter for FIVES."""
    klen = 255 if size - 10 > R.MAX_VALUE else max(1, min(7, size - 4))
    digits = bytes(B62[i // 62 ** j % 62] for j in range(6, -1, -1))
    key = bytes([0x61 + FIVES.index(i)]) if klen == 1 else digits[-klen:] if klen <= 7 else digits.ljust(255, b"K")
    vlen = size - 3 - klen
    assert 1 <= vlen <= R.MAX_VALUE and len(key) == klen
    return key, ((np.arange(vlen, dtype=np.uint32) * 7 + i) % 26 + 0x41).astype(np.uint8).tobytes()


@pytest.fixture(scope="module")
def packs(ctx, tmp_path_factory):
    """3 000 records of 5 .. 32 768 bytes as a small resident database and, in its slot order, as text on the device:
    the two packs are given the same records in the same order."""
    from bsdb_amd.builder import build_text
    tmp = tmp_path_factory.mktemp("high_packs")
    sizes = sizes_a()
    assert min(sizes) == 5 and max(sizes) == 32768 and sum(s > 8192 for s in sizes) > 50
    recs = [record_a(i, s) for i, s in enumerate(sizes)]
    assert len({k for k, _ in recs}) == N_A and [3 + len(k) + len(v) for k, v in recs] == sizes
    src, d = str(tmp / "in.txt"), str(tmp / "db")
    with open(src, "wb") as f:
        f.write(lines_of(recs))
    assert build_text(src, d, partitions=1, verify=True)["records"] == N_A
    mph = ctx.mph_load(os.path.join(d, "hash.dump"))
    db = mph.open_db(os.path.join(d, "kv.db"), 1, os.path.join(d, "index.db"))
    rank = mph.lookup_var(*pack([k for k, _ in recs]), check=True)
    assert sorted(rank.tolist()) == list(range(N_A))
    by_slot = [recs[i] for i in np.argsort(rank)]
    text = lines_of(by_slot)
    t = to_dev(text)
    desc, report = ctx.text_split(t, b" ", nbytes=len(text))
    rec = ctx.db_records(db)
    torch.cuda.synchronize()
    assert int(report.cpu()[1]) == N_A and not rec[4].any().item()
    P = dict(ctx=ctx, tmp=str(tmp), db=db, records=by_slot, t=t, nbytes=len(text), desc=desc, rec=rec[:4], cache={})
    yield P
    db.close()
    mph.close()


def run_packs(P, parts, part_sizes, B, n_image, refused=False):
    """Both packs into an image view of exactly n_image bytes at a misaligned address between guard bytes, a guarded
    address array and a guarded key blob; the views' guards are checked.  refused: both must answer BSDB_EINVAL and
    leave every byte of the three buffers alone."""
    from bsdb_amd.native import BsdbError
    ctx, n, out = P["ctx"], len(P["records"]), {}
    nblob = sum(len(k) for k, _ in P["records"])
    for name in ("text", "db"):
        ibuf, iview = guarded_u8(n_image, 3)
        bbuf, bview = guarded_u8(nblob, 5)
        abuf, aview, al = guarded_i64(n)
        if name == "text":
            call = lambda: ctx.text_pack(P["t"], P["desc"], n, parts, part_sizes, nbytes=P["nbytes"], image=iview, addr=aview,  # noqa: E731
                                         blob=bview, block_size=B)
        else:
            call = lambda: ctx.db_pack(P["db"], *P["rec"], parts, part_sizes, count=n, image=iview, addr=aview, blob=bview,  # noqa: E731
                                       block_size=B)
        if refused:
            with pytest.raises(BsdbError) as e:
                call()
            assert e.value.code == EINVAL, name
            torch.cuda.synchronize()
            assert (ibuf.cpu().numpy() == GUARD).all() and (bbuf.cpu().numpy() == GUARD).all() and (abuf.cpu().numpy() == IGUARD).all(), name
            continue
        res = call()
        torch.cuda.synchronize()
        out[name] = host_pack(res)
        h = ibuf.cpu().numpy()
        assert (h[:3] == GUARD).all() and (h[3 + n_image:] == GUARD).all(), name
        h = bbuf.cpu().numpy()
        assert (h[:5] == GUARD).all() and (h[5 + nblob:] == GUARD).all(), name
        h = abuf.cpu().numpy()
        assert (h[:al] == IGUARD).all() and (h[al + n:] == IGUARD).all(), name
    return out


def reference(P, parts, B):
    """Per (partitions, block size), once: the writers' restatement, and the run lengths of a first call with
    part_sizes = 0 (the exact-fit sizes come from these, as a caller would get them)."""
    key = (parts, B)
    if key not in P["cache"]:
        image, runs, rel, run_of = oracle_pack(P["tmp"], f"o{parts}_{B}", P["records"], parts, B)
        first = P["ctx"].text_pack(P["t"], P["desc"], len(P["records"]), parts, [0] * parts, nbytes=P["nbytes"], block_size=B)
        torch.cuda.synchronize()
        assert first["run_bytes"] == runs
        P["cache"][key] = dict(image=image, runs=first["run_bytes"], rel=rel, run_of=run_of)
    return P["cache"][key]


def check_accepted(P, parts, part_sizes, B):
    ref = reference(P, parts, B)
    got = run_packs(P, parts, part_sizes, B, len(ref["image"]))
    want = placed(ref["rel"], ref["run_of"], part_sizes, B)
    blob = b"".join(k for k, _ in P["records"])
    for name in ("text", "db"):
        g = got[name]
        assert g["run_bytes"] == ref["runs"], name
        bad = [i for i, (x, y) in enumerate(zip(g["addr"], want)) if x != y]
        assert not bad, (name, bad[:3], [hex(g["addr"][i]) for i in bad[:3]], [hex(want[i]) for i in bad[:3]])
        assert all(a >> 63 == 0 and a >> 56 == p for a, p in zip(g["addr"], ref["run_of"])), name
        assert len(g["image"]) == len(ref["image"]) and g["image"] == ref["image"], name   # ... whatever the files held
        assert g["blob"] == blob, name
    assert got["text"] == got["db"]
    return want


def compact_sizes(parts, pick, runs):
    """part_sizes drawn from 2^32 - 7, 2^32, 2^55 + 5 in turn from `pick` on; the last partition fits exactly."""
    pool = [T32 - 7, T32, (1 << 55) + 5]
    return [pool[(p + pick) % 3] for p in range(parts - 1)] + [(1 << 56) - runs[parts - 1]]


@pytest.mark.parametrize("parts,pick", [(1, 0), (3, 0), (3, 1), (3, 2), (128, 0)])
def test_compact_addresses_beyond_32_bits(packs, parts, pick):
    ref = reference(packs, parts, None)
    if parts == 1:
        for F in (T32 - 7, T32, (1 << 55) + 5):
            check_accepted(packs, 1, [F], None)
    sizes = compact_sizes(parts, pick, ref["runs"])
    want = check_accepted(packs, parts, sizes, None)
    # the last record of the last partition ends with byte 2^56 - 1 of its file
    k, v = packs["records"][-1]
    assert want[-1] == (parts - 1) << 56 | ((1 << 56) - (3 + len(k) + len(v)))
    if parts == 128:
        assert want[-1] >> 56 == 127 and want[-1] > (1 << 63) - 40_000


@pytest.mark.parametrize("parts", [1, 3])
def test_compact_refuses_a_file_past_2_56(packs, parts):
    ref = reference(packs, parts, None)
    for p in (0, parts - 1):
        sizes = [T32] * parts
        sizes[p] = (1 << 56) - ref["runs"][p] + 1
        run_packs(packs, parts, sizes, None, len(ref["image"]), refused=True)


@pytest.mark.parametrize("parts", [1, 3])
@pytest.mark.parametrize("B", [4096, 8192])
def test_blocked_page_numbers_beyond_20_bits(packs, B, parts):
    ref = reference(packs, parts, B)
    assert all(r % PAGE == 0 and r > 3 * PAGE for r in ref["runs"])
    for sizes in ([T32 - 2 * PAGE] * parts, [1 << 43] * parts, [(1 << 44) - r for r in ref["runs"]]):
        want = check_accepted(packs, parts, sizes, B)
        page = [(a >> 16) & 0xFFFFFFFF for a in want]
        end = [pg + ((a >> 48) & 0xFF) for pg, a in zip(page, want)]
        if sizes[0] == T32 - 2 * PAGE:                                # the page numbers cross 2^20 inside every run
            assert all(min(pg for pg, p in zip(page, ref["run_of"]) if p == q) < 1 << 20 <=
                       max(pg for pg, p in zip(page, ref["run_of"]) if p == q) for q in range(parts))
        if sizes[0] + ref["runs"][0] == 1 << 44:                      # exact fit: the last block ends with page 2^32 - 1
            assert all(max(e for e, p in zip(end, ref["run_of"]) if p == q) == 1 << 32 for q in range(parts))


@pytest.mark.parametrize("B", [4096, 8192])
def test_blocked_refuses_a_file_past_2_44(packs, B):
    for parts in (1, 3):
        ref = reference(packs, parts, B)
        for p in (0, parts - 1):
            sizes = [1 << 43] * parts
            sizes[p] = (1 << 44) - ref["runs"][p] + PAGE
            run_packs(packs, parts, sizes, B, len(ref["image"]), refused=True)


# ==== B. a resident image above 4 GiB ==============================================================================

N_B, J = 3000, 702
NOT_TEXT_VALUES = [b"a b", b"line\nfeed", b"carriage\rreturn", b"nul\x00byte", b" ", b"\n", b"\r\n", b"\x00" * 40, bytes(range(256))]
VARIANTS = ("header", "key", "value", "large")


def source_records():
    """3 000 records + 4: keys of 1 .. 255 bytes, values of 0 .. 32 510 bytes, about 60 larger than a 4096-byte block,
    some no text carries.  Record J (partition 0 of both layouts) has a 24-byte key and a 12 000-byte text value."""
    rng = np.random.default_rng(2032)
    truth = {}
    for i in range(N_B):
        c = i % 100
        klen = 255 if c == 7 else int(rng.integers(100, 255)) if c == 8 else int(rng.integers(6, 41))
        vlen = (0 if c == 0 else int(rng.integers(4200, 20001)) if c in (1, 2) else 32510 if c == 3 and i < 1000 else
                int(rng.integers(64, 301)) if c < 40 else int(rng.integers(0, 64)))
        if i == J:
            klen, vlen = 24, 12000
        head = b"%d:" % i
        key, val = head + rand_bytes(rng, klen - len(head)), rand_bytes(rng, vlen)
        if c == 50:
            val = NOT_TEXT_VALUES[(i // 100) % len(NOT_TEXT_VALUES)] + val
        if c == 51:
            key = head + (b" k\n", b"\r", b"\x00 ")[(i // 100) % 3] + key[len(head):][:20]
        truth[key] = val
    truth.update({b"a": b"a key of one byte", b"\x00": b"nul key", b"key with spaces": b"plain", b"k\n\r": b"v\n"})
    keys = list(truth)
    assert len(truth) == N_B + 4 and {len(k) for k in keys} >= {1, 255} and max(len(v) for v in truth.values()) == 32510
    assert min(len(v) for v in truth.values()) == 0 and sum(len(k) >= 16 and len(v) >= 64 for k, v in truth.items()) >= 50
    assert sum(not is_text(k, v) for k, v in truth.items()) >= 60 and sum(3 + len(k) + len(v) > PAGE for k, v in truth.items()) >= 50
    assert len(keys[J]) == 24 and len(truth[keys[J]]) == 12000 and is_text(keys[J], truth[keys[J]])
    return truth


def edited_records(truth):
    """B: 200 values edited in one byte (record J's in its middle byte), 100 keys removed, 100 new.
    (B's dict, the upserts U, the removed keys with other values R)."""
    rng = np.random.default_rng(2034)
    keys = list(truth)
    b, u, r = dict(truth), {}, {}
    edit = [J] + [i for i in range(5, N_B, 14) if i != J and len(truth[keys[i]]) > 0][:199]
    for i in edit:
        v = truth[keys[i]]
        m = len(v) // 2
        u[keys[i]] = flip(v, m) if is_text(keys[i], v) else v[:m] + bytes([v[m] ^ 0x40]) + v[m + 1:]
    for i in [i for i in range(11, N_B, 13) if i not in edit][:100]:
        r[keys[i]] = rand_bytes(rng, 1 + i % 9)
        del b[keys[i]]
    for j in range(100):
        u[b"new%d:" % j + rand_bytes(rng, j % 9)] = rand_bytes(rng, 1 + 37 * j % 500)
    b.update(u)
    assert len(edit) == 200 and len(r) == 100 and len(u) == 300 and len(b) == len(truth)
    return b, u, r


class Resident:
    """A database directory resident on the shared context, and what Python knows of it."""

    def __init__(self, mph, d, parts, fmt, block, truth, own_mph=False):
        self.dir, self.parts, self.fmt, self.block, self.truth = d, parts, fmt, block, truth
        self.mph, self.own_mph = mph, own_mph
        self.kv, self.index_path = os.path.join(d, "kv.db"), os.path.join(d, "index.db")
        t0 = time.perf_counter()
        self.db = mph.open_db(self.kv, parts, self.index_path, fmt=fmt, block_size=block)
        self.open_seconds = time.perf_counter() - t0
        self.sizes = [os.path.getsize(f"{self.kv}.{p}") for p in range(parts)]
        self.index = np.fromfile(self.index_path, ">u8").astype(np.uint64)
        keys = list(truth)
        self.rank = mph.lookup_var(*pack(keys), check=True)
        assert sorted(self.rank.tolist()) == list(range(len(keys)))
        self.by_slot = [(keys[i], truth[keys[i]]) for i in np.argsort(self.rank)]
        self.memo = {}

    def close(self):
        self.db.close()
        if self.own_mph:
            self.mph.close()


def open_dir(ctx, d, truth, parts, fmt=0, block=PAGE):
    return Resident(ctx.mph_load(os.path.join(d, "hash.dump")), d, parts, fmt, block, truth, own_mph=True)


def file_pos(word, fmt):
    """(partition, the record's offset in its file) of an index word."""
    word = int(word)
    return word >> 56, (word & L.FILE_MASK) if fmt == 0 else ((word >> 16) & 0xFFFFFFFF) * PAGE + (word & 0xFFFF)


def items_of(db):
    r = db.items()
    keys, values, koff, voff = r["keys"].tobytes(), r["values"].tobytes(), r["koff"].tolist(), r["voff"].tolist()
    assert not r["status"].any()
    return [(keys[koff[i]: koff[i + 1]], values[voff[i]: voff[i + 1]]) for i in range(len(koff) - 1)], r["report"]


def guarded(nbytes, mis):
    """A uint8 view of nbytes bytes at `mis` past a 16-byte aligned address, between 0xA5 guard bytes."""
    buf = torch.full((nbytes + 256,), GUARD, dtype=torch.uint8, device="cuda")
    lead = 64 + (-buf.data_ptr()) % 16 + mis
    return buf, buf[lead: lead + nbytes], lead


def memo(side, name, make):
    if name not in side.memo:
        side.memo[name] = make()
    return side.memo[name]


def get_all(side, queries, batch=0):
    side.db.set_batch(batch)
    try:
        res = side.db.get_var(*pack(queries))
    finally:
        side.db.set_batch(0)
    vals, voff = res["values"].tobytes(), res["voff"].tolist()
    return res["status"].tolist(), [vals[voff[i]: voff[i + 1]] for i in range(len(queries))], res["report"]


def merge_into(side, out, parts, fmt, delta=None, removed=None):
    """Database.merge into the fresh directory `out`: (the report, {file name: bytes})."""
    os.makedirs(out)
    rep, mph = side.db.merge(os.path.join(out, "kv.db"), parts, 4, os.path.join(out, "index.db"), fmt=fmt, block_size=PAGE,
                             delta=delta.db if delta else None, removed=removed.db if removed else None)
    mph.close()
    files = {}
    for f in sorted(os.listdir(out)):
        with open(os.path.join(out, f), "rb") as fh:
            files[f] = fh.read()
        os.remove(os.path.join(out, f))
    return rep, files


MERGES = (("compact1", 1, 0, False), ("blocked2", 2, 1, False), ("delta_removed3", 3, 0, True))


class TestImageAbove4GiB:
    @pytest.fixture(scope="class")
    def world(self, ctx, tmp_path_factory):
        """orig: the source compact in 3 partitions; orig_b: blocked 4096 in 2 partitions; B, U, R: the small
        databases of the diff and the merge; the source's text records as a file, and the same with one byte of
        record J's value edited."""
        tmp = tmp_path_factory.mktemp("high_image")
        truth = source_records()
        b, u, r = edited_records(truth)
        keys = list(truth)
        w = dict(ctx=ctx, tmp=tmp, truth=truth, jkey=keys[J])
        w["orig"] = open_dir(ctx, write_db(str(tmp / "orig"), truth, 3), truth, 3)
        w["orig_b"] = open_dir(ctx, write_blocked_db(ctx, str(tmp / "orig_b"), truth, 2, PAGE), truth, 2, 1, PAGE)
        for name, d in (("B", b), ("U", u), ("R", r)):
            w[name] = open_dir(ctx, write_db(str(tmp / name), d, 1), d, 1)
        text = [(k, v) for k, v in truth.items() if is_text(k, v)]
        assert len(text) > 2800 and (keys[J], truth[keys[J]]) in text
        m = len(truth[keys[J]]) // 2
        w["text"], w["text_edited"], w["n_text"] = str(tmp / "source.txt"), str(tmp / "edited.txt"), len(text)
        with open(w["text"], "wb") as f:
            f.write(lines_of(text))
        with open(w["text_edited"], "wb") as f:
            f.write(lines_of([(k, flip(v, m) if k == keys[J] else v) for k, v in text]))
        w["absent"] = L.absent(np.random.default_rng(5), keys, 500, [1, 5, 9, 24, 255])
        yield w
        for name in ("orig", "orig_b", "B", "U", "R"):
            w[name].close()

    @staticmethod
    def shifts_of(world, name):
        """(the original, the shifts, x: the byte of record J that lands on image position 2^32)."""
        jkey = world["jkey"]
        klen, vlen = len(jkey), len(world["truth"][jkey])
        if name == "large":
            orig = world["orig_b"]
            word = int(orig.index[orig.rank[J]])
            part, pos = file_pos(word, 1)
            pages = (word >> 48) & 0xFF
            assert part == 0 and word & 0xFFFF == 0 and pages == -(-(3 + klen + vlen) // PAGE) >= 3   # a block of its own
            x = PAGE                                                  # the first page boundary inside the block ...
            assert 3 + klen < x < 3 + klen + vlen                     # ... lies inside the value
            return orig, [H.straddle_shift(pos, x), 0], x
        orig = world["orig"]
        part, pos = file_pos(orig.index[orig.rank[J]], 0)
        assert part == 0 and klen >= 16 and vlen >= 64
        x = {"header": 1, "key": 3 + klen // 2, "value": 3 + klen + vlen // 2}[name]
        return orig, [H.straddle_shift(pos, x), 0, 5], x

    @staticmethod
    def relocated(world, name, tag):
        orig, shifts, x = TestImageAbove4GiB.shifts_of(world, name)
        d = str(world["tmp"] / tag)
        sizes = H.relocate(orig.dir, d, orig.parts, orig.fmt, orig.block, shifts)
        return orig, shifts, x, d, sizes

    @pytest.fixture(scope="class", params=VARIANTS)
    def variant(self, world, request):
        """One relocated copy, resident: opened on the original's MPHF.  The preconditions are asserted here, so no
        test can pass without the image reaching past 2^32."""
        name = request.param
        orig, shifts, x, d, sizes = self.relocated(world, name, f"reloc_{name}")
        if name == "large":
            assert shifts[0] % PAGE == 0
        side = Resident(orig.mph, d, orig.parts, orig.fmt, orig.block, world["truth"])
        print(f"\n[beyond 32 bits] open of '{name}': {side.open_seconds:.2f} s, image {side.db.info()['image_bytes']} bytes")
        try:
            assert side.sizes == sizes and side.db.info()["image_bytes"] > T32
            ksrc, klen, vsrc, vlen, st, _ = world["ctx"].db_records(side.db)
            ksrc, klen, vsrc, vlen = (a.cpu().numpy().astype(np.int64) for a in (ksrc, klen, vsrc, vlen))
            assert not st.any().item()
            j = int(orig.rank[J])
            assert ksrc[j] - 3 + x == T32                             # byte x of record J is image byte 2^32
            if name == "header":
                assert ksrc[j] - 3 < T32 < ksrc[j]                    # the header is split
            else:
                assert ksrc[j] < T32 <= vsrc[j] + vlen[j] and ((ksrc < T32) & (vsrc + vlen >= T32)).sum() >= 1
            assert (ksrc >= T32).sum() * 3 >= ksrc.size               # a third of the records lie wholly above
            side.name, side.orig, side.shifts, side.x = name, orig, shifts, x
            yield side
        finally:
            side.close()
            for p in range(side.parts):
                os.remove(f"{side.kv}.{p}")

    # ---- records ---------------------------------------------------------------------------------------------

    def test_records(self, world, variant):
        ctx, orig = world["ctx"], variant.orig

        def rec(side):
            out = ctx.db_records(side.db)
            return [a.cpu().numpy() for a in out[:5]] + [[x & U64 for x in out[5].cpu().tolist()]]

        o = memo(orig, "records", lambda: rec(orig))
        g = rec(variant)
        for i, what in ((1, "klen"), (3, "vlen"), (4, "status")):
            assert np.array_equal(g[i], o[i]), what
        assert g[5] == o[5]
        assert o[1].tolist() == [len(k) for k, _ in orig.by_slot] and o[3].tolist() == [len(v) for _, v in orig.by_slot]
        old_base, _ = L.layout(orig.sizes)
        new_base, total = L.layout(variant.sizes)
        assert total == variant.db.info()["image_bytes"]
        step = np.array([new_base[p] + variant.shifts[p] - old_base[p] for p in range(orig.parts)], np.int64)
        part = (orig.index >> np.uint64(56)).astype(np.int64)
        assert np.array_equal(variant.index >> np.uint64(56), orig.index >> np.uint64(56))
        for i, what in ((0, "ksrc"), (2, "vsrc")):
            assert np.array_equal(g[i].astype(np.int64) - o[i].astype(np.int64), step[part]), what
        # ... and the original's positions are the files': base + the record's offset + 3 (+ klen)
        pos = np.array([old_base[p] + off for p, off in (file_pos(w, orig.fmt) for w in orig.index)], np.int64)
        assert np.array_equal(o[0].astype(np.int64), pos + 3) and np.array_equal(o[2].astype(np.int64), pos + 3 + o[1])

    # ---- get ---------------------------------------------------------------------------------------------------

    def test_get(self, world, variant):
        ctx, orig, truth = world["ctx"], variant.orig, world["truth"]
        rng = np.random.default_rng(9)
        q = list(truth) + world["absent"]
        q = [q[i] for i in rng.permutation(len(q))]
        want_status, _, want_rep = memo(orig, "get", lambda: get_all(orig, q))
        assert all((s == FOUND) == (k in truth) for s, k in zip(want_status, q)) and want_status.count(FOUND) == len(truth)
        for batch in (0, 1000):
            status, values, rep = get_all(variant, q, batch)
            assert status == want_status and rep == want_rep, batch
            bad = [k for k, v in zip(q, values) if v != truth.get(k, b"")]
            assert not bad, (batch, len(bad), bad[:3])
        # the device forms: locate, then gather into a misaligned view between guards
        blob, off = pack(q)
        d_blob = torch.from_numpy(blob.copy()).cuda()
        d_off = torch.from_numpy(off.astype(np.int64)).cuda()
        src, vl, st, rep = ctx.db_locate_var(variant.db, d_blob, d_off)
        assert st.cpu().tolist() == want_status and vl.cpu().tolist() == [len(truth.get(k, b"")) for k in q]
        assert [int(x) for x in rep.cpu().tolist()[:6]] == [want_rep[k] for k in list(want_rep)[:6]]
        voff = ctx.edge_offsets(vl)
        total = int(voff[len(q)])
        want = b"".join(truth.get(k, b"") for k in q)
        assert total == len(want)
        for mis in (5, 8):
            buf, view, lead = guarded(total, mis)
            ctx.db_gather(variant.db, src, voff, values=view, value_bytes=total)
            torch.cuda.synchronize()
            h = buf.cpu().numpy()
            assert h[lead: lead + total].tobytes() == want, mis
            assert (h[:lead] == GUARD).all() and (h[lead + total:] == GUARD).all()
        above = (src.cpu().numpy() >= T32).sum()
        assert above * 3 >= len(truth)

    # ---- items and dump ------------------------------------------------------------------------------------------

    def test_items_and_dump(self, world, variant):
        orig, tmp = variant.orig, world["tmp"]

        def dump(side, name):
            path = str(tmp / name)
            rep = side.db.dump_text(path)
            with open(path, "rb") as f:
                data = f.read()
            os.remove(path)
            return rep, data

        want_rep, want = memo(orig, "dump", lambda: dump(orig, "orig.dump"))
        assert want == lines_of(orig.by_slot) and want_rep["slots"] == len(orig.by_slot) and want_rep["bad_addr"] == 0
        rep, data = dump(variant, f"{variant.name}.dump")
        assert len(data) == len(want) and data == want and rep == want_rep
        pairs, rep = items_of(variant.db)
        assert pairs == orig.by_slot
        assert rep == memo(orig, "items", lambda: items_of(orig.db))[1]

    # ---- check ---------------------------------------------------------------------------------------------------

    def test_check(self, world, variant):
        orig = variant.orig
        for path, edited in ((world["text"], False), (world["text_edited"], True)):
            want = memo(orig, f"check{edited}", lambda: orig.db.check_text([path]))
            res = variant.db.check_text([path])
            assert res == want, edited
            n = world["n_text"]
            assert res["text"]["records"] == res["check"]["records"] == n
            if not edited:
                assert res["ok"] and res["check"]["ok"] == n and res["n_bad"] == 0
            else:
                with open(path, "rb") as f:
                    at = f.read().index(b"\n" + world["jkey"] + b" ") + 1
                assert not res["ok"] and res["check"]["ok"] == n - 1 and res["check"]["value_bytes"] == 1
                assert res["bad"] == [(path, at, CHECK_VALUE_BYTES)] and res["n_bad"] == 1

    # ---- diff ------------------------------------------------------------------------------------------------------

    def test_diff(self, world, variant):
        orig, B, tmp = variant.orig, world["B"], world["tmp"]
        n = len(world["truth"])

        def diff(x, y, name):
            up, rm = str(tmp / f"{name}.upsert"), str(tmp / f"{name}.removed")
            res = x.db.diff(y.db, upsert=up, removed=rm)
            files = []
            for p in (up, rm):
                with open(p, "rb") as f:
                    files.append(f.read())
                os.remove(p)
            return res, files

        for x, y in ((orig, variant), (variant, orig)):
            res, files = diff(x, y, "same")
            assert res["identical"] and res["ab"]["same"] == res["ba"]["same"] == n and files == [b"", b""]
            assert res["ab"]["first_diff"] == res["ba"]["first_diff"] == U64
            assert res["ab"]["compared_bytes"] == sum(len(v) for v in world["truth"].values())
        want, want_files = memo(orig, "diff_B", lambda: diff(orig, B, "orig_B"))
        assert want["ab"]["value_bytes"] == want["ba"]["value_bytes"] == 200 and want["ab"]["same"] == n - 300
        assert want["ab"]["rejected"] + want["ab"]["key_mismatch"] == want["ba"]["rejected"] + want["ba"]["key_mismatch"] == 100
        assert want_files[0] == lines_of([r for r in B.by_slot if world["truth"].get(r[0]) != r[1]])
        assert want_files[1] == lines_of([r for r in orig.by_slot if r[0] not in B.truth])
        res, files = diff(variant, B, f"{variant.name}_B")
        assert res == want and files == want_files
        back, bfiles = diff(B, variant, f"B_{variant.name}")
        wback, wbfiles = memo(orig, "diff_B_back", lambda: diff(B, orig, "B_orig"))
        assert back == wback and bfiles == wbfiles and (back["ab"], back["ba"]) == (want["ba"], want["ab"])

    # ---- merge -----------------------------------------------------------------------------------------------------

    @pytest.mark.parametrize("name,parts,fmt,delta", MERGES, ids=[m[0] for m in MERGES])
    def test_merge(self, world, variant, name, parts, fmt, delta):
        orig, tmp = variant.orig, world["tmp"]
        U, Rm = (world["U"], world["R"]) if delta else (None, None)
        want_rep, want = memo(orig, f"merge_{name}", lambda: merge_into(orig, str(tmp / f"m_{name}_{orig.fmt}"), parts, fmt, U, Rm))
        assert sorted(want) == ["index.db"] + [f"kv.db.{p}" for p in range(parts)]
        assert want_rep["out_records"] == len(world["B"].truth if delta else world["truth"]) and want_rep["bad_slot"] == want_rep["bad_addr"] == 0
        if delta:
            assert (want_rep["replaced"], want_rep["removed"], want_rep["delta_written"]) == (200, 100, 300)
        rep, files = merge_into(variant, str(tmp / f"m_{name}_{variant.name}"), parts, fmt, U, Rm)
        assert rep == want_rep and sorted(files) == sorted(want)
        for f in want:
            assert len(files[f]) == len(want[f]) and files[f] == want[f], f

    # ---- an untrusted index at high positions ----------------------------------------------------------------------

    def test_untrusted_index_at_high_positions(self, world):
        """A copy of the `value` variant with four index words rewritten by rank: into the hole, to the last two
        bytes of partition 0 (above 2^32), to record J's address + 1, and to an offset of partition 1 that is
        partition 0's size.  The expected status is the header's rule over a memmap of the file."""
        orig, shifts, x, d, sizes = self.relocated(world, "value", "reloc_untrusted")
        truth, keys = world["truth"], list(world["truth"])
        index = np.fromfile(os.path.join(d, "index.db"), ">u8").astype(np.uint64)
        addr_j = int(index[orig.rank[J]])
        victims = [3, 300, J, 1501]
        words = [1000, sizes[0] - 2, addr_j + 1, 1 << 56 | sizes[0]]
        assert words[0] + 40000 < shifts[0] and sizes[0] - 2 > T32 and sizes[0] > sizes[1]
        files = [np.memmap(os.path.join(d, f"kv.db.{p}"), np.uint8, "r") for p in range(3)]
        want, no_record = {}, []
        for i, wd in zip(victims, words):
            index[orig.rank[i]] = wd
            dec = L.decode(wd, 0, sizes)
            want[keys[i]] = BAD_ADDR if dec is None else L.header_rule(files[dec[0]], sizes[dec[0]], dec[1], keys[i])
            if dec is None or L.header_rule(files[dec[0]], sizes[dec[0]], dec[1], b"") == BAD_ADDR:   # whatever the key
                no_record.append(int(orig.rank[i]))
        assert [want[keys[i]] for i in victims] == [KEY_MISMATCH, BAD_ADDR, want[keys[J]], BAD_ADDR] and want[keys[J]] != FOUND
        del files
        index.astype(">u8").tofile(os.path.join(d, "index.db"))
        db = orig.mph.open_db(os.path.join(d, "kv.db"), 3, os.path.join(d, "index.db"))
        try:
            assert db.info()["image_bytes"] > T32
            res = db.get_var(*pack(keys))
            vals, voff = res["values"].tobytes(), res["voff"].tolist()
            assert res["status"].tolist() == [want.get(k, FOUND) for k in keys]
            assert all(vals[voff[i]: voff[i + 1]] == (b"" if k in want else truth[k]) for i, k in enumerate(keys))
            # the slots themselves: a header of zeros in the hole is a record of no bytes; the others are no record
            st = world["ctx"].db_records(db)[4].cpu().numpy()
            assert np.flatnonzero(st).tolist() == sorted(no_record) and len(no_record) >= 2
        finally:
            db.close()
            for p in range(3):
                os.remove(os.path.join(d, f"kv.db.{p}"))


# ==== C. text positions above 2^31 ==================================================================================

TEXT_CAP = T31 + (64 << 10) + 16


def high_text():
    """A + one line of G "x" + "\\n" + B: (A, G, B, the records with B's positions moved in Python integers, the
    report, the index of the record of B whose value holds byte 2^31)."""
    la, rng = random_lines(300, 200)
    A = join_lines(la, rng)
    lb, rng = random_lines(300, 225)
    B = join_lines(lb, rng)
    assert A[-1:] == b"\n"
    ra, wa = R.restate(A, b" ")
    rb, wb = R.restate(B, b" ")
    r = next(i for i in range(10, len(rb)) if len(rb[i][3]) >= 4)
    G = T31 - len(A) - 1 - rb[r][2] - len(rb[r][3]) // 2
    base = len(A) + G + 1
    recs = ra + [(kp + base, k, vp + base, v) for kp, k, vp, v in rb]
    want = {f: max(wa[f], wb[f]) if f.startswith("max") else wa[f] + wb[f] for f in R.FIELDS}
    want["lines"] += 1
    want["not_two_fields"] += 1
    for w in (wa, wb):
        assert min(w["records"], w["not_two_fields"], w["empty_key"], w["too_large"]) > 15
    assert A.count(b"\r\n") > 50 and B.count(b"\r\n") > 50
    assert base + len(B) <= TEXT_CAP - 16 and len({k for _, k, _, _ in recs}) == len(recs)   # (B's keys are not A's)
    return A, G, B, recs, want, len(ra) + r


class TestTextAbove2GiB:
    @pytest.fixture(scope="class")
    def big(self, ctx):
        from bsdb_amd.native import TEXT_FIELDS, text_max_records
        A, G, B, recs, want, at = high_text()
        base = len(A) + G + 1
        nbytes = base + len(B)
        t = torch.full((TEXT_CAP,), 0x78, dtype=torch.uint8, device="cuda")
        assert t.data_ptr() % 16 == 0
        t[:len(A)] = torch.from_numpy(np.frombuffer(A, np.uint8).copy()).cuda()
        t[len(A) + G] = 0x0A
        t[base: nbytes] = torch.from_numpy(np.frombuffer(B, np.uint8).copy()).cuda()
        desc = torch.empty((4, text_max_records(nbytes)), dtype=torch.int32, device="cuda")
        t0 = time.perf_counter()
        desc, report = ctx.text_split(t, b" ", nbytes=nbytes, desc=desc)
        torch.cuda.synchronize()
        print(f"\n[beyond 32 bits] split of {nbytes} text bytes: {time.perf_counter() - t0:.2f} s")
        rep = dict(zip(TEXT_FIELDS, report.cpu().numpy().view(np.uint64).tolist()))
        k = len(recs)
        assert sum(kp >= T31 for kp, _, _, _ in recs) >= 100           # the range is there
        assert recs[at][2] < T31 < recs[at][2] + len(recs[at][3])     # byte 2^31 lies inside a kept record's value
        yield dict(ctx=ctx, t=t, nbytes=nbytes, desc=desc, rep=rep, recs=recs, want=want, at=at, k=k)
        del t, desc
        torch.cuda.empty_cache()

    def test_report_and_descriptors(self, big):
        rep, want, recs, k = big["rep"], big["want"], big["recs"], big["k"]
        assert {f: rep[f] for f in R.FIELDS} == want, (rep, want)
        assert rep["chunks"] == 1 and rep["lines"] == rep["records"] + rep["not_two_fields"] + rep["empty_key"] + rep["too_large"]
        d = big["desc"][:, :k].cpu().numpy().view(np.uint32)
        exp = np.array([[kp, len(key), vp, len(v)] for kp, key, vp, v in recs], np.uint64).T
        assert exp.max() < T32 and (exp[0] >= T31).sum() >= 100
        bad = np.flatnonzero((d.astype(np.uint64) != exp).any(axis=0))
        assert bad.size == 0, (bad[:5], d[:, bad[:5]], exp[:, bad[:5]])

    @pytest.mark.parametrize("B", [None, 4096], ids=["compact", "blocked4096"])
    def test_pack(self, big, tmp_path, B):
        ctx, recs, k = big["ctx"], big["recs"], big["k"]
        records = [(key, v) for _, key, _, v in recs]
        parts, sizes = 2, [0, 3 * PAGE]
        image, runs, rel, run_of = oracle_pack(str(tmp_path), "c", records, parts, B)
        blob = b"".join(key for key, _ in records)
        ibuf, iview = guarded_u8(len(image), 3)
        bbuf, bview = guarded_u8(len(blob), 5)
        out = ctx.text_pack(big["t"], big["desc"], k, parts, sizes, nbytes=big["nbytes"], image=iview, blob=bview, block_size=B)
        torch.cuda.synchronize()
        got = host_pack(out)
        assert got["run_bytes"] == runs
        assert got["addr"] == placed(rel, run_of, sizes, B)
        assert len(got["image"]) == len(image) and got["image"] == image
        assert got["blob"] == blob and got["off"] == np.cumsum([0] + [len(key) for key, _ in records]).tolist()
        for buf, lead, n in ((ibuf, 3, len(image)), (bbuf, 5, len(blob))):
            h = buf.cpu().numpy()
            assert (h[:lead] == GUARD).all() and (h[lead + n:] == GUARD).all()

    def test_check_against_a_database(self, big, tmp_path):
        ctx, recs, k, t, at = big["ctx"], big["recs"], big["k"], big["t"], big["at"]
        truth = {key: v for _, key, _, v in recs}
        side = open_dir(ctx, write_db(str(tmp_path / "db"), truth, 2), truth, 2)
        try:
            nblob = sum(len(key) for key in truth)
            blob = torch.empty(nblob + 16, dtype=torch.uint8, device="cuda")
            out = ctx.text_pack(t, big["desc"], k, 1, [0], nbytes=big["nbytes"], blob=blob, want_image=False)
            assert out["blob"].cpu().numpy().tobytes() == b"".join(truth)

            def check():
                src, dbvlen, status, _ = ctx.db_locate_var(side.db, out["blob"], out["off"])
                assert not status.any().item()
                status, report = ctx.db_check(side.db, t, big["desc"][2], big["desc"][3], src, dbvlen, status, nbytes=big["nbytes"], count=k)
                torch.cuda.synchronize()
                return status.cpu().tolist(), report.cpu().numpy().view(np.uint64).tolist()

            status, report = check()
            assert status == [0] * k and report[:2] == [k, k] and report[-1] == U64
            before = int(t[T31])
            t[T31] = before ^ 0x01                                    # one text byte at position 2^31, on the device
            try:
                status, report = check()
            finally:
                t[T31] = before
            assert status == [CHECK_VALUE_BYTES if i == at else 0 for i in range(k)]
            assert report[:2] == [k, k - 1] and report[2 + CHECK_VALUE_BYTES - 1] == 1 and report[-1] == at
        finally:
            side.close()
