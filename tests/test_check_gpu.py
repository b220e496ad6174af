"""GPU: a database checked against text input (bsdb_db_check_text,
bsdb_dev_db_check, builder.check_text, build_text(verify_values=True), the
command line's -vv and --check).

All comparisons are exact.  Ground truth is a Python dict of what the test
wrote: a record of the text whose key is in the dict is OK, VALUE_LEN or
VALUE_BYTES by comparing the two values; a key that is not gets the status the
existing checked lookup gives it (REJECTED for rank -1, else KEY_MISMATCH), as
absent_status in tests/test_get_gpu.py.  The records of a text, their order and
their offsets are tests/text_rule.py's."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import text_rule as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, REJECTED, KEY_MISMATCH, BAD_ADDR, VALUE_LEN, VALUE_BYTES = range(6)
U64 = (1 << 64) - 1
N, PARTS = 5_000, 3
ALPHA = np.array([b for b in range(256) if b not in (0x0A, 0x0D, 0x20)], np.uint8)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def rand_bytes(rng, n):
    return ALPHA[rng.integers(0, ALPHA.size, int(n))].tobytes()


def flip(v, j):
    """v with byte j changed to another byte that is no separator and no terminator."""
    b = v[j] ^ 0x01
    if b in (0x0A, 0x0D, 0x20):
        b = v[j] ^ 0x02
    return v[:j] + bytes([b]) + v[j + 1:]


def pack(items):
    off = np.zeros(len(items) + 1, np.uint64)
    if items:
        off[1:] = np.cumsum([len(k) for k in items])
    return np.frombuffer(b"".join(items), np.uint8) if items else np.zeros(0, np.uint8), off


def write_files(tmp, name, lines, cut):
    """The lines as two files, the first `cut` of them in the first; the last line of each without a terminator."""
    paths = [str(tmp / f"{name}_a.txt"), str(tmp / f"{name}_b.txt")]
    for p, part in zip(paths, (lines[:cut], lines[cut:])):
        with open(p, "wb") as f:
            f.write(b"\n".join(part))
    return paths


def restate(paths, truth, mph, base=0):
    """What a check of the files against the database `truth` must give: (statuses in input order, the check
    report, the list of (path, offset of the key, status) of the records that are not OK, the text's record count)."""
    status, where = [], []
    for p in paths:
        recs, _ = R.restate(open(p, "rb").read(), b" ")
        absent = [k for _, k, _, _ in recs if k not in truth]
        ranks = dict(zip(absent, mph.lookup_var(*pack(absent), check=True).tolist())) if absent else {}
        for kpos, k, _, v in recs:
            if k in truth:
                st = OK if truth[k] == v else VALUE_LEN if len(truth[k]) != len(v) else VALUE_BYTES
            else:
                st = REJECTED if ranks[k] < 0 else KEY_MISMATCH
            status.append(st)
            where.append((p, kpos))
    bad = [(p, o, s) for (p, o), s in zip(where, status) if s]
    first = next((i for i, s in enumerate(status) if s), None)
    names = ("ok", "rejected", "key_mismatch", "bad_addr", "value_len", "value_bytes")
    rep = dict(records=len(status), **{n: status.count(i) for i, n in enumerate(names)},
               first_bad=U64 if first is None else base + first)
    return status, rep, bad


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """A 3-partition compact database of 5 000 records with keys of 2 .. 26 bytes and values of 1 .. 120 bytes,
    built by build_text(verify_values=True) from two files with junk lines among the records."""
    _need_gpu()
    from bsdb_amd.builder import build_text
    tmp = tmp_path_factory.mktemp("check_db")
    rng = np.random.default_rng(81)
    keys = [b"%d:" % i + rand_bytes(rng, rng.integers(0, 21)) for i in range(N)]
    vals = [rand_bytes(rng, l) for l in rng.integers(1, 121, N)]
    lines = [k + b" " + v for k, v in zip(keys, vals)]
    for j in (10, 2_000, 4_900):
        lines.insert(j, b"junk line %d that is no record" % j)
    paths = write_files(tmp, "own", lines, 3_001)
    d = str(tmp / "db")
    rep = build_text(paths, d, checksum_bits=4, partitions=PARTS, verify=True, verify_values=True)
    assert rep["records"] == N and rep["values"]["ok"] and rep["values"]["complete"]
    assert rep["values"]["check"] == dict(records=N, ok=N, rejected=0, key_mismatch=0, bad_addr=0, value_len=0,
                                          value_bytes=0, first_bad=U64)
    return dict(dir=d, tmp=tmp, keys=keys, vals=vals, lines=lines, paths=paths, truth=dict(zip(keys, vals)))


@pytest.fixture(scope="module")
def reader(built):
    from bsdb_amd.reader import BSDBReader
    with BSDBReader(built["dir"]) as rd:
        yield rd
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def edited(built):
    """The text with, at known lines of both files: a value changed in one byte, one a byte shorter, one a byte longer,
    an absent key, and more junk."""
    rng = np.random.default_rng(82)
    lines = list(built["lines"])
    kv = lambda i: lines[i].split(b" ")  # noqa: E731
    for i, edit in ((700, "byte"), (1_500, "shorter"), (2_999, "absent"), (3_500, "longer"), (4_200, "byte"), (4_950, "absent")):
        k, v = kv(i)
        if edit == "byte":
            lines[i] = k + b" " + flip(v, len(v) // 2)
        elif edit == "shorter":
            lines[i] = k + b" " + (v[:-1] if len(v) > 1 else v + b"x")
        elif edit == "longer":
            lines[i] = k + b" " + v + b"x"
        else:
            lines[i] = b"absent%d " % i + v
    for j in (5, 3_300):
        lines.insert(j, b"three fields here")
        lines.insert(j, b"")
    return write_files(built["tmp"], "edited", lines, 3_001 + 2)


def test_own_text_is_all_ok(built, reader):
    from bsdb_amd.builder import check_text
    res = reader.db.check_text(built["paths"])
    _, rep, bad = restate(built["paths"], built["truth"], reader.mph)
    assert res["ok"] is True and res["check"] == rep and res["bad"] == bad == [] and res["n_bad"] == 0
    assert res["check"]["ok"] == res["check"]["records"] == res["text"]["records"] == N and res["check"]["first_bad"] == U64
    assert res["text"]["lines"] == N + 3 and res["text"]["not_two_fields"] == 3
    top = check_text(built["paths"], built["dir"])                      # the directory form
    assert top["ok"] and top["complete"] and top["db_records"] == N and top["check"] == rep


@pytest.mark.parametrize("chunk", [0, 64 << 10], ids=["one_chunk", "chunks_of_64KiB"])
def test_status_classes(built, reader, edited, chunk):
    status, rep, bad = restate(edited, built["truth"], reader.mph)
    assert rep["value_bytes"] == 2 and rep["value_len"] == 2 and rep["rejected"] + rep["key_mismatch"] == 2
    assert rep["ok"] == N - 6 and {p for p, _, _ in bad} == set(edited)  # both files hold bad records
    reader.ctx.text_set_chunk(chunk)
    try:
        res = reader.db.check_text(edited)
        capped = reader.db.check_text(edited, bad_cap=2)
        none = reader.db.check_text(edited, bad_cap=0)
    finally:
        reader.ctx.text_set_chunk(0)
    assert res["ok"] is False and res["check"] == rep, (res["check"], rep)
    assert res["bad"] == bad and res["n_bad"] == len(bad) == 6
    assert res["text"]["records"] == N and res["text"]["lines"] == N + 3 + 4
    assert (res["text"]["chunks"] > 5) if chunk else (res["text"]["chunks"] == 2)   # 64 KiB: many chunks, carried tails
    assert capped["bad"] == bad[:2] and capped["n_bad"] == 6 and capped["check"] == rep
    assert none["bad"] == [] and none["n_bad"] == 6 and none["check"] == rep


def to_dev(text: bytes):
    t = torch.empty(len(text) + 16, dtype=torch.uint8, device="cuda")
    t[len(text):] = 0x20
    if text:
        t[:len(text)] = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def i32(a):
    return torch.from_numpy(np.asarray(a, np.uint32).view(np.int32).copy()).cuda()


def device_check(ctx, db, text, keys, vpos, vlen, base=0, report=None):
    """locate + check on device buffers: (the check's statuses, the report's words as unsigned)."""
    kblob, koff = pack(keys)
    src, dbvlen, status, _ = ctx.db_locate_var(db, torch.from_numpy(kblob.copy()).cuda() if kblob.size else
                                               torch.zeros(1, dtype=torch.uint8, device="cuda"),
                                               torch.from_numpy(koff.astype(np.int64)).cuda())
    status, report = ctx.db_check(db, to_dev(text), i32(vpos), i32(vlen), src, dbvlen, status, nbytes=len(text),
                                  count=len(keys), record_base=base, report=report)
    torch.cuda.synchronize()
    return status.cpu().numpy().tolist(), report.cpu().numpy().view(np.uint64).tolist(), report


def test_compare_edges_through_the_device_forms(tmp_path):
    _need_gpu()
    from bsdb_amd import Context, kvfiles
    rng = np.random.default_rng(83)
    recs = []      # (key, the database's value, the text's value)
    for j in range(33):   # a 33-byte value differing in byte j only, then an equal one-byte value
        v = rand_bytes(rng, 33)
        recs += [(b"a%d" % j, v, flip(v, j)), (b"b%d" % j, *[rand_bytes(rng, 1)] * 2)]
    big = [rand_bytes(rng, 32_510) for _ in range(2)]
    same = lambda key, n: (key, *[rand_bytes(rng, n)] * 2)  # noqa: E731
    recs += [same(b"n0", 5), (b"big0", big[0], flip(big[0], 32_509)), same(b"n1", 16), (b"big1", big[1], flip(big[1], 0)),
             same(b"n2", 3)]
    for i in range(40):   # 40 one-byte values in a row, the 17th differing
        v = rand_bytes(rng, 1)
        recs.append((b"o%d" % i, v, flip(v, 0) if i == 16 else v))
    recs += [(b"e%d" % i, b"", b"") for i in range(12)]   # empty values in the database, empty descriptors
    recs += [same(b"z0", 9), (b"e_last", b"", b"")]
    keys = [k for k, _, _ in recs]
    text, vpos, vlen = bytearray(), [], []
    for k, _, tv in recs:
        text += k + b" "
        vpos.append(len(text))
        vlen.append(len(tv))
        text += tv + b"\n"
    want = [OK if dv == tv else VALUE_BYTES for _, dv, tv in recs]
    assert want.count(VALUE_BYTES) == 33 + 2 + 1
    kv, ip = str(tmp_path / "kv.db"), str(tmp_path / "index.db")
    kblob, koff = pack(keys)
    with Context(0) as ctx:
        addr = kvfiles.write_compact(kv, 1, kblob, koff, *kvfiles.pack_values([dv for _, dv, _ in recs]))
        with ctx.mph_build_index_var(kblob, koff, 4, addr, ip) as mph, mph.open_db(kv, 1, ip) as db:
            n = len(recs)
            status, rep, report = device_check(ctx, db, bytes(text), keys, vpos, vlen, base=100)
            assert status == want
            assert rep == [n, n - 36, 0, 0, 0, 0, 36, 100]                # record 0 is the first that differs
            # a second call accumulates, and first_bad stays the smallest
            status, rep, _ = device_check(ctx, db, bytes(text), keys, vpos, vlen, base=50_000, report=report)
            assert status == want and rep == [2 * n, 2 * (n - 36), 0, 0, 0, 0, 72, 100]
            # lengths: one byte shorter and longer in the text than in the database, an empty against a non-empty
            vl2 = list(vlen)
            vl2[0], vl2[1], vl2[n - 2] = 32, 2, 0
            status, rep, _ = device_check(ctx, db, bytes(text), keys, vpos, vl2)
            w2 = list(want)
            w2[0] = w2[1] = w2[n - 2] = VALUE_LEN
            assert status == w2 and rep[5] == 3 and rep[0] == n == sum(rep[1:7]) and rep[7] == 0


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 4_999])
def test_record_counts(built, reader, count):
    """split -> key blob -> locate -> check on the device for the first `count` records, the last one's value changed."""
    ctx, db = reader.ctx, reader.db
    lines = [k + b" " + v for k, v in zip(built["keys"][:count], built["vals"][:count])]
    if count:
        lines[-1] = built["keys"][count - 1] + b" " + flip(built["vals"][count - 1], 0)
    text = b"\n".join(lines)
    t = to_dev(text)
    desc, trep = ctx.text_split(t, " ", nbytes=len(text))
    assert int(trep[1]) == count
    report = ctx.check_report("cuda")
    if count:
        out = ctx.text_pack(t, desc, count, 1, [0], nbytes=len(text))
        src, dbvlen, status, _ = ctx.db_locate_var(db, out["blob"], out["off"])
        status, report = ctx.db_check(db, t, desc[2], desc[3], src, dbvlen, status, nbytes=len(text), count=count,
                                      record_base=7, report=report)
    else:
        z32, z64, z8 = (torch.zeros(1, dtype=dt, device="cuda") for dt in (torch.int32, torch.int64, torch.uint8))
        status, report = ctx.db_check(db, t, z32, z32, z64, z32, z8, nbytes=0, count=0, report=report)
    torch.cuda.synchronize()
    assert status.cpu().numpy().tolist() == [OK] * max(count - 1, 0) + [VALUE_BYTES] * min(count, 1)
    assert report.cpu().numpy().view(np.uint64).tolist() == [count, max(count - 1, 0), 0, 0, 0, 0, min(count, 1),
                                                             7 + count - 1 if count else U64]


@pytest.mark.parametrize("block", [4096, 8192])
def test_blocked_layout(tmp_path, block):
    _need_gpu()
    from bsdb_amd.builder import build_text, check_text
    rng = np.random.default_rng(block)
    n = 2_000
    keys = [b"%d" % i for i in range(n)]
    vals = [rand_bytes(rng, l) for l in rng.integers(1, 300, n)]
    vals[1_001] = rand_bytes(rng, 9_000)            # larger than a block: a block of its own
    lines = [k + b" " + v for k, v in zip(keys, vals)]
    paths = write_files(tmp_path, "own", lines, 900)
    d = str(tmp_path / "db")
    rep = build_text(paths, d, partitions=2, layout="blocked", block_size=block, verify_values=True)
    assert rep["values"]["ok"] and rep["values"]["check"]["ok"] == n
    lines[1_001] = keys[1_001] + b" " + flip(vals[1_001], 8_999)
    lines[3] = keys[3] + b" " + vals[3] + b"y"
    other = write_files(tmp_path, "edited", lines, 900)
    res = check_text(other, d)
    off_big = sum(len(l) + 1 for l in lines[900:1_001])
    assert not res["ok"] and res["complete"] is False and res["db_records"] == n
    assert res["bad"] == [(other[0], sum(len(l) + 1 for l in lines[:3]), VALUE_LEN), (other[1], off_big, VALUE_BYTES)]
    assert res["check"] == dict(records=n, ok=n - 2, rejected=0, key_mismatch=0, bad_addr=0, value_len=1, value_bytes=1,
                                first_bad=3)


def test_approximate_mode(tmp_path):
    _need_gpu()
    from bsdb_amd.builder import build_text, check_text
    rng = np.random.default_rng(84)
    n = 2_000
    keys = [b"%d" % i for i in range(n)]
    vals = [rand_bytes(rng, l) for l in rng.integers(12, 40, n)]
    vals[5], vals[6] = rand_bytes(rng, 3), rand_bytes(rng, 8)     # a head shorter than the slot, one that fills it
    lines = [k + b" " + v for k, v in zip(keys, vals)]
    own = write_files(tmp_path, "own", lines, 1_000)
    d = str(tmp_path / "db")
    rep = build_text(own, d, partitions=2, approximate=True, verify_values=True)   # index.db and index_a.db both checked
    assert rep["values"]["ok"]
    res = check_text(own, d)                                       # the directory says index.approximate: index_a.db
    assert res["ok"] and res["complete"] and res["check"]["ok"] == n
    lines[100] = keys[100] + b" " + flip(vals[100], 3)             # within the first 8 bytes: flagged
    lines[1_500] = keys[1_500] + b" " + flip(vals[1_500], 10)      # after byte 8: the slot cannot tell
    lines[5] = keys[5] + b" " + vals[5] + b"q"                     # a longer head: flagged (there is no length status)
    other = write_files(tmp_path, "edited", lines, 1_000)
    res = check_text(other, d)
    assert res["bad"] == [(other[0], sum(len(l) + 1 for l in lines[:5]), VALUE_BYTES),
                          (other[0], sum(len(l) + 1 for l in lines[:100]), VALUE_BYTES)]
    assert res["check"] == dict(records=n, ok=n - 2, rejected=0, key_mismatch=0, bad_addr=0, value_len=0, value_bytes=2,
                                first_bad=5)
    exact = check_text(other, d, approximate=False)                # the kv.db files tell all three
    assert exact["check"]["value_bytes"] == 2 and exact["check"]["value_len"] == 1 and exact["n_bad"] == 3


def test_bad_addr(built, reader, tmp_path):
    from bsdb_amd.builder import check_text
    d = str(tmp_path / "copy")
    shutil.copytree(built["dir"], d)
    ip = os.path.join(d, "index.db")
    victim = 1_234
    rank = int(reader.mph.lookup_var(*pack([built["keys"][victim]]), check=True)[0])
    index = np.fromfile(ip, ">u8")
    part = int(index[rank]) >> 56
    index[rank] = part << 56 | (os.path.getsize(os.path.join(d, f"kv.db.{part}")) + 64)   # past its partition's end
    index.tofile(ip)
    res = check_text(built["paths"], d)
    line = victim + sum(1 for j in (10, 2_000, 4_900) if j <= victim + 1)     # (junk lines 10 and 2 000 precede it)
    assert built["lines"][line].startswith(built["keys"][victim] + b" ") and line < 3_001
    assert res["bad"] == [(built["paths"][0], sum(len(l) + 1 for l in built["lines"][:line]), BAD_ADDR)]
    assert res["check"] == dict(records=N, ok=N - 1, rejected=0, key_mismatch=0, bad_addr=1, value_len=0, value_bytes=0,
                                first_bad=victim)


def test_a_flipped_file_byte_is_found_and_the_cli_exits_2(built, tmp_path):
    from bsdb_amd.builder import check_text
    from bsdb_amd.writer import VerifyError
    d = str(tmp_path / "copy")
    shutil.copytree(built["dir"], d)
    # the first record of kv.db.1: [kLen][vLen u16 BE][key][value]; the last byte of its value flipped
    f = np.fromfile(os.path.join(d, "kv.db.1"), np.uint8)
    klen, vlen = int(f[0]), int(f[1]) << 8 | int(f[2])
    key = f[3: 3 + klen].tobytes()
    f[3 + klen + vlen - 1] ^= 0x10
    f.tofile(os.path.join(d, "kv.db.1"))
    line = next(i for i, l in enumerate(built["lines"]) if l.startswith(key + b" "))
    path = built["paths"][0 if line < 3_001 else 1]
    off = sum(len(l) + 1 for l in built["lines"][(0 if line < 3_001 else 3_001): line])
    with pytest.raises(VerifyError) as e:
        check_text(built["paths"], d, strict=True)
    assert e.value.report["bad"] == [(path, off, VALUE_BYTES)] and e.value.report["check"]["value_bytes"] == 1
    assert check_text(built["paths"], d)["ok"] is False                    # without strict: the dict
    cmd = [sys.executable, "-m", "bsdb_amd.builder", "--check", "-o", d, "-i", built["paths"][0], "-i", built["paths"][1]]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2, (r.returncode, r.stderr[-2000:])
    assert f"{path}:{off} value_bytes" in r.stdout.splitlines() and f"ok={N - 1}" in r.stdout
    good = subprocess.run(cmd[:5] + [built["dir"]] + cmd[6:], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert good.returncode == 0 and f"ok={N} " in good.stdout and "complete=true" in good.stdout, good.stderr[-2000:]
