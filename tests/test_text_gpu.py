"""GPU: the text front end (bsdb_dev_text_split / bsdb_dev_text_pack,
bsdb_builder_add_dev_var, bsdb_text_build, bsdb_amd.builder).

Ground truth is never the code under test: tests/text_rule.py restates the
record rule as bytes.splitlines(), line.split(sep) and dropping trailing empty
fields, which shares nothing with the library's position lists; images,
addresses and value heads are built from its records in Python; databases are
read back with the existing reader, verifier and scan.  All comparisons are
exact.  The report invariant (lines = records + not_two_fields + empty_key +
too_large) is asserted wherever a report is compared.

A value of 0 bytes cannot be written as a line ("key<sep>" has one field once
the trailing empty field is dropped), so the end-to-end records carry values
of 1..200 bytes and the inputs hold "key<sep>" lines that must be counted as
not_two_fields."""
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
TERMS = (b"\n", b"\r", b"\r\n")
TABLE = ["a b", "a b ", "a b  ", "a  b", " a b", "a b c", "a ", "a", "", " ", " b"]
E2BIG, EDUP = -7, -17


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from bsdb_amd import Context
    c = Context(0)
    yield c
    c.close()
    torch.cuda.empty_cache()


def to_dev(text: bytes):
    """The text at a 16-byte aligned device address, followed by 16 bytes that would
    change the result if they were classified (separators and terminators)."""
    t = torch.empty(len(text) + 16, dtype=torch.uint8, device="cuda")
    t[len(text):] = torch.from_numpy(np.frombuffer(b" \n \r,\t\n " * 2, np.uint8).copy()).cuda()
    if text:
        t[:len(text)] = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def check_split(ctx, text: bytes, sep: bytes):
    """Splits `text` on the device and compares descriptors, order and report with the restatement."""
    from bsdb_amd.native import TEXT_FIELDS
    recs, want = R.restate(text, sep)
    t = to_dev(text)
    desc, report = ctx.text_split(t, sep, nbytes=len(text))
    torch.cuda.synchronize()
    rep = dict(zip(TEXT_FIELDS, report.cpu().numpy().view(np.uint64).tolist()))
    assert {k: rep[k] for k in R.FIELDS} == want, (rep, want)
    assert rep["chunks"] == (1 if text else 0)
    assert rep["lines"] == rep["records"] + rep["not_two_fields"] + rep["empty_key"] + rep["too_large"]
    k = len(recs)
    d = desc[:, :k].cpu().numpy().view(np.uint32)
    exp = np.array([[kp, len(key), vp, len(v)] for kp, key, vp, v in recs], np.uint32).reshape(k, 4).T
    assert np.array_equal(d, exp)
    return t, desc, recs, rep


def join_lines(lines, rng):
    """The lines, each ended by one of the three terminators at random; an empty line never follows a bare "\\r"
    (the two would read as one "\\r\\n" line end)."""
    terms = [TERMS[int(i)] for i in rng.integers(0, 3, len(lines))]
    for i in range(len(lines) - 1):
        if terms[i] == b"\r" and lines[i + 1] == b"":
            terms[i] = b"\r\n"
    return b"".join(l + t for l, t in zip(lines, terms))


# ---- 1. the table and the degenerate texts -------------------------------------------------------------------

@pytest.mark.parametrize("sep", [b" ", b"\t", b","])
def test_rule_table(ctx, sep):
    rng = np.random.default_rng(sep[0])
    lines = [t.replace(" ", sep.decode()).encode() for t in TABLE] * 3
    text = join_lines(lines, rng)
    assert text.splitlines() == lines                     # every case of the table is a line of the text
    _, _, recs, rep = check_split(ctx, text, sep)
    assert (rep["records"], rep["not_two_fields"], rep["empty_key"], rep["too_large"]) == (9, 21, 3, 0)
    check_split(ctx, text.rstrip(b"\r\n"), sep)           # the same without the final terminator


@pytest.mark.parametrize("text", [b"", b"\n", b"a", b"a\n", b"a\r", b"a\r\n", b"a b", b"a b\n", b"a b\r", b"a b\r\n",
                                  b"\n\n\n", b"\r\r\r", b"\r\n\r\n", b"\r\r\n\n\r", b"\n\r", b" ", b" \n"])
def test_degenerate_texts(ctx, text):
    _, _, recs, rep = check_split(ctx, text, b" ")
    assert rep["lines"] == len(text.splitlines())
    if text == b"\r\r\n\n\r":
        assert rep["lines"] == 4 and rep["not_two_fields"] == 4


def test_split_argument_errors(ctx):
    from bsdb_amd.native import BsdbError
    t = to_dev(b"a b\n")
    for bad in (b"\r", b"\n", b"\x80", b"\xff"):
        with pytest.raises(BsdbError) as e:
            ctx.text_split(t, bad, nbytes=4)
        assert e.value.code == -22
    small = torch.empty((4, 1), dtype=torch.int32, device="cuda")   # capacity below text_max_records(4) = 2
    with pytest.raises(BsdbError) as e:
        ctx.text_split(t, b" ", nbytes=4, desc=small)
    assert e.value.code == -22
    with pytest.raises(BsdbError):                                  # a text at an unaligned address
        ctx.text_split(t[1:], b" ", nbytes=3)


# ---- 2. edges the kernels can get wrong ----------------------------------------------------------------------

EDGES = [o for T in (16, 64, 256, 4096) for o in (T - 1, T, T + 1)]


@pytest.mark.parametrize("feature", ["line_start", "separator", "crlf"])
def test_piece_and_block_edges(ctx, feature):
    """A line start, a separator, and the "\\n" of a "\\r\\n" pair at byte offsets 15/16/17 ... 4095/4096/4097:
    at 16 k the pair is split across a 16-byte piece, at 64 across a wave's pieces' edge, at 4096 across two
    workgroups."""
    for o in EDGES:
        if feature == "line_start":    # the first line is o bytes long with its terminator
            text = b"k " + b"v" * (o - 3) + b"\n" + b"x y\nz w"
            assert text.index(b"x y") == o
        elif feature == "separator":   # the second line's separator sits at o
            text = b"p " + b"q" * (o - 6) + b"\n" + b"abc val\r\nz w\n"
            assert text[o:o + 1] == b" " and text[o - 3:o] == b"abc"
        else:                          # "\r" at o - 1, "\n" at o
            text = b"k " + b"v" * (o - 3) + b"\r\n" + b"x y\rz w\r\n"
            assert text[o - 1:o + 1] == b"\r\n"
        _, _, recs, rep = check_split(ctx, text, b" ")
        assert rep["records"] == 3 and rep["lines"] == 3, (feature, o)


def test_sizes_junk_and_bytes(ctx):
    raw = bytes(b for b in range(256) if b not in (0x0A, 0x0D, 0x20))      # 0x00 and 0x80..0xFF are data
    lines = [
        b"k" * 255 + b" v", b"k" * 256 + b" v",                            # key of 255 kept, 256 too large
        b"a " + b"v" * 32510, b"b " + b"v" * 32511,                        # value of 32 510 kept, 32 511 too large
        b"x" * 70_000,                                                     # one junk line
        b"key value" + b" " * 5000,                                        # a record, then 5 000 trailing separators
        b"j " * 3000,                                                      # junk: 3 000 fields
        raw[:100] + b" " + raw[100:], b"\x00 \x00", b"\xff\x80 \x80\xff", b"\x00",
    ]
    text = join_lines(lines, np.random.default_rng(2))
    _, _, recs, rep = check_split(ctx, text, b" ")
    assert rep["records"] == 6 and rep["too_large"] == 2 and rep["not_two_fields"] == 3
    assert rep["max_key_len"] == 255 and rep["max_value_len"] == 32510
    check_split(ctx, text.rstrip(b"\r\n"), b" ")


# ---- 3. seeded random ----------------------------------------------------------------------------------------

def random_lines(n, seed, sep=b" "):
    """n lines: about 60 % records, about 10 % each of the malformed classes (not two fields in several shapes,
    empty key, too large by the key; a few too large by the value)."""
    rng = np.random.default_rng(seed)
    alpha = np.array([b for b in range(1, 256) if b not in (0x0A, 0x0D, sep[0])], np.uint8)

    def word(lo, hi):
        return alpha[rng.integers(0, alpha.size, int(rng.integers(lo, hi + 1)))].tobytes()

    lines = []
    cls = rng.choice(6, n, p=[0.6, 0.1, 0.1, 0.1, 0.09, 0.01])
    for i, c in enumerate(cls):
        key = b"%d_" % i + word(0, 20)
        if c == 0:
            lines.append(key + sep + word(1, 40) + sep * int(rng.integers(0, 3) == 0))
        elif c == 1:
            lines.append([key, key + sep, key + sep + sep + word(1, 5), sep + key + sep + word(1, 5), b"",
                          key + sep + word(1, 5) + sep + word(1, 5), sep * 3][int(rng.integers(0, 7))])
        elif c == 2:
            lines.append(key + sep + word(1, 8) + sep + word(1, 8))
        elif c == 3:
            lines.append(sep + word(1, 30))
        elif c == 4:
            lines.append(key + word(256, 300) + sep + word(1, 10))
        else:
            lines.append(key + sep + word(32511, 32600))
    return lines, rng


def test_random_20000_lines(ctx):
    lines, rng = random_lines(20_000, 23)
    text = join_lines(lines, rng)
    _, _, recs, rep = check_split(ctx, text, b" ")
    for k in ("records", "not_two_fields", "empty_key", "too_large"):
        assert rep[k] > 1500, rep
    assert len(text) > 3 * 4096


# ---- 4. pack -------------------------------------------------------------------------------------------------

GUARD = 0xA5


def guarded_u8(n, lead):
    """n bytes at an address that is `lead` (odd) past an aligned one, between guard bytes."""
    buf = torch.full((lead + n + 37,), GUARD, dtype=torch.uint8, device="cuda")
    return buf, buf[lead:lead + n]


def guarded_i64(n):
    """n int64 at an address 8 past a 16-byte aligned one, between guard words."""
    buf = torch.full((n + 4,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device="cuda")
    lead = 1 if buf.data_ptr() % 16 == 0 else 2
    return buf, buf[lead:lead + n], lead


def check_guard_u8(buf, lead, n):
    h = buf.cpu().numpy()
    assert (h[:lead] == GUARD).all() and (h[lead + n:] == GUARD).all()


def check_guard_i64(buf, lead, n):
    h = buf.cpu().numpy()
    assert (h[:lead] == -0x5A5A5A5A5A5A5A5B).all() and (h[lead + n:] == -0x5A5A5A5A5A5A5A5B).all()


def pack_text():
    rng = np.random.default_rng(31)
    lines = [b"k%d %s" % (i, bytes(rng.integers(0x30, 0x7B, int(rng.integers(1, 30)), dtype=np.uint8))) for i in range(150)]
    lines += [b"s%d %c" % (i, 65 + i % 26) for i in range(20)]                 # 20 one-byte values ...
    lines += [b"big " + bytes(rng.integers(0x30, 0x7B, 32510, dtype=np.uint8))]  # ... a 32 510-byte value ...
    lines += [b"t%d %c" % (i, 97 + i % 26) for i in range(20)]                 # ... 20 more one-byte values
    lines += [b"junk", b" nokey", b"m%d %s" % (7, b"\x00\xff\x80" * 5)]
    return join_lines(lines, rng)


@pytest.mark.parametrize("parts,count", [(1, None), (3, None), (8, None), (8, 5)])
def test_pack(ctx, parts, count):
    """The image, the addresses, the key blob + offsets and the value heads, byte for byte against a Python
    construction, for partitions that already hold bytes; written into misaligned views between guards."""
    text = pack_text()
    t, desc, recs, rep = check_split(ctx, text, b" ")
    if count is not None:                         # only 5 records over 8 partitions: some runs are empty
        recs = recs[:count]
    k = len(recs)
    assert k == (count or 192)
    image, offs = R.image_of(recs)
    blob = b"".join(key for _, key, _, _ in recs)
    koff = np.concatenate([[0], np.cumsum([len(key) for _, key, _, _ in recs])]).astype(np.uint64)
    start = [1000 * p + 7 for p in range(parts)]   # what each partition file holds already
    bound = R.run_bounds(k, parts)
    offs.append(len(image))
    addr = np.zeros(k, np.uint64)
    for p in range(parts):
        for r in range(bound[p], bound[p + 1]):
            addr[r] = p << 56 | (start[p] + offs[r] - offs[bound[p]])
    v8, vl = R.value_heads(recs)

    ibuf, iview = guarded_u8(len(image), 3)        # exactly as large as the image: nothing may be written past it
    bbuf, bview = guarded_u8(len(blob), 5)
    lbuf, lview = guarded_u8(k, 7)
    abuf, aview, al = guarded_i64(k)
    obuf, oview, ol = guarded_i64(k + 1)
    vbuf, vview, vlead = guarded_i64(k)
    assert iview.data_ptr() % 16 and bview.data_ptr() % 16 and aview.data_ptr() % 16 == 8
    out = ctx.text_pack(t, desc, k, parts, start, approximate=True, nbytes=len(text), image=iview, addr=aview,
                        blob=bview, off=oview, value8=vview, value_len=lview)
    torch.cuda.synchronize()
    assert out["run_bytes"] == [offs[bound[p + 1]] - offs[bound[p]] for p in range(parts)]
    assert sum(out["run_bytes"]) == len(image) and (count is None or 0 in out["run_bytes"])
    assert out["image"].cpu().numpy().tobytes() == image
    assert np.array_equal(out["addr"].cpu().numpy().view(np.uint64), addr)
    assert out["blob"].cpu().numpy().tobytes() == blob
    assert np.array_equal(out["off"].cpu().numpy().view(np.uint64), koff)
    assert np.array_equal(out["value8"].cpu().numpy().view(np.uint64), v8)
    assert np.array_equal(out["value_len"].cpu().numpy(), vl)
    check_guard_u8(ibuf, 3, len(image)), check_guard_u8(bbuf, 5, len(blob)), check_guard_u8(lbuf, 7, k)
    check_guard_i64(abuf, al, k), check_guard_i64(obuf, ol, k + 1), check_guard_i64(vbuf, vlead, k)


@pytest.mark.parametrize("mis", range(16))
def test_pack_short_destinations_at_every_misalignment(ctx, mis):
    """Three short records, and the first of them alone: a 17- and a 5-byte image, a 4- and a 1-byte key blob, each
    at `mis` bytes past an aligned address between guards.  Destinations shorter than a piece: their first piece is
    their last where mis + bytes <= 16, and they straddle two partial pieces where it is more."""
    text = b"a b\ncd e\nf gh\n"
    t, desc, recs, _ = check_split(ctx, text, b" ")
    assert len(recs) == 3
    for k in (1, 3):
        image, _ = R.image_of(recs[:k])
        blob = b"".join(key for _, key, _, _ in recs[:k])
        assert (len(image), len(blob)) == ((5, 1) if k == 1 else (17, 4))
        ibuf, iview = guarded_u8(len(image), mis)
        bbuf, bview = guarded_u8(len(blob), mis)
        assert iview.data_ptr() % 16 == mis and bview.data_ptr() % 16 == mis
        out = ctx.text_pack(t, desc, k, 1, [0], nbytes=len(text), image=iview, blob=bview)
        torch.cuda.synchronize()
        assert out["run_bytes"] == [len(image)]
        assert out["image"].cpu().numpy().tobytes() == image
        assert out["blob"].cpu().numpy().tobytes() == blob
        check_guard_u8(ibuf, mis, len(image)), check_guard_u8(bbuf, mis, len(blob))


def test_pack_refuses_a_small_destination(ctx):
    from bsdb_amd.native import BsdbError
    text = b"a b\nc d\n"
    t, desc, recs, _ = check_split(ctx, text, b" ")
    ibuf, iview = guarded_u8(9, 3)                 # the image needs 10 bytes
    with pytest.raises(BsdbError) as e:
        ctx.text_pack(t, desc, 2, 1, [0], nbytes=len(text), image=iview)
    assert e.value.code == -22
    torch.cuda.synchronize()
    check_guard_u8(ibuf, 0, 0)                     # nothing was written at all


# ---- 5. streaming --------------------------------------------------------------------------------------------

CHUNK = 64 << 10


def stream_file():
    """~300 KB of lines for a 64 KiB chunk: byte 65 535 is a "\\n" (the first cut falls right after it, nothing is
    carried), the second buffer therefore starts at 65 536 and its last byte, file byte 131 071, is the "\\r" of a
    "\\r\\n" whose "\\n" lies outside it; the file ends in a bare "\\r"."""
    lines, rng = random_lines(9_000, 41)
    lines = [l for l in lines if len(l) < 2000]
    out = bytearray()

    def pad_line_to(end, term):                    # a record whose terminator ends exactly at file offset `end`
        key = b"pad%d" % end
        out.extend(key + b" " + b"v" * (end - len(out) - len(key) - 1 - len(term)) + term)
        assert len(out) == end

    it = iter(lines)
    for target, term in ((CHUNK, b"\n"), (2 * CHUNK + 1, b"\r\n")):
        while len(out) < target - 3000:
            out.extend(next(it) + TERMS[int(rng.integers(0, 3))])
        if out[-1:] == b"\r":
            out.extend(b"\n")
        pad_line_to(target, term)
    while len(out) < 300_000:
        out.extend(next(it) + TERMS[int(rng.integers(0, 3))])
    out.extend(b"last one\r")
    data = bytes(out)
    assert data[CHUNK - 1:CHUNK] == b"\n" and data[2 * CHUNK - 1:2 * CHUNK + 1] == b"\r\n" and data.endswith(b"e\r")
    return data


def read_records(kv_base, parts):
    """Every record of the written files through the native scan: [(key, value)] read at the scan's addresses."""
    from bsdb_amd.native import kv_scan
    s = kv_scan(kv_base, parts)
    files = [open(f"{kv_base}.{p}", "rb").read() for p in range(parts)]
    out = []
    for i, a in enumerate(s["addr"].tolist()):
        f, o = files[a >> 56], a & ((1 << 56) - 1)
        kl, vl = f[o], f[o + 1] << 8 | f[o + 2]
        key = f[o + 3:o + 3 + kl]
        assert key == s["blob"][int(s["offsets"][i]):int(s["offsets"][i + 1])].tobytes()
        out.append((key, f[o + 3 + kl:o + 3 + kl + vl]))
    assert sum(len(f) for f in files) == sum(3 + len(k) + len(v) for k, v in out)   # nothing but records
    return out


def stream_build(ctx, tmp_path, datas, parts=3):
    paths = []
    for i, d in enumerate(datas):
        paths.append(str(tmp_path / f"in{i}.txt"))
        with open(paths[-1], "wb") as f:
            f.write(d)
    ctx.text_set_chunk(CHUNK)
    try:
        mph, rep = ctx.text_build(paths, b" ", str(tmp_path / "kv.db"), parts, 4, str(tmp_path / "index.db"),
                                  str(tmp_path / "index_a.db"))
    finally:
        ctx.text_set_chunk(0)
    want = dict.fromkeys(R.FIELDS, 0)
    recs = []
    for d in datas:                                # files do not join: each is restated on its own
        r, w = R.restate(d, b" ")
        recs += r
        for k in R.FIELDS:
            want[k] = max(want[k], w[k]) if k.startswith("max") else want[k] + w[k]
    assert {k: rep[k] for k in R.FIELDS} == want
    assert rep["lines"] == rep["records"] + rep["not_two_fields"] + rep["empty_key"] + rep["too_large"]
    got = read_records(str(tmp_path / "kv.db"), parts)
    assert sorted(got) == sorted((k, v) for _, k, _, v in recs)
    assert mph.info()["n"] == len(recs)
    if recs:
        v = mph.verify_kv(str(tmp_path / "kv.db"), parts, str(tmp_path / "index.db"), str(tmp_path / "index_a.db"))
        assert v["ok"] and v["records"] == len(recs)
    mph.close()
    return rep


def test_streaming_one_file(ctx, tmp_path):
    rep = stream_build(ctx, tmp_path, [stream_file()])
    assert rep["chunks"] >= 5


def test_streaming_three_files(ctx, tmp_path):
    """The same records over three files: the first ends without a terminator, in the middle of what was one
    file's line sequence, and must not join the third; the second is empty."""
    data = stream_file()
    cut = data.index(b"\n", 100_000)
    rep = stream_build(ctx, tmp_path, [data[:cut], b"", data[cut + 1:]])
    assert rep["chunks"] > 1
    one, _ = R.restate(data, b" ")
    assert rep["records"] == len(one)


def test_streaming_line_longer_than_the_chunk(ctx, tmp_path):
    from bsdb_amd.native import BsdbError
    p = tmp_path / "long.txt"
    p.write_bytes(b"a b\n" + b"k " + b"v" * 99_998 + b"\nc d\n")
    ctx.text_set_chunk(CHUNK)
    try:
        with pytest.raises(BsdbError) as e:
            ctx.text_build([str(p)], b" ", str(tmp_path / "kv.db"), 2, 4, str(tmp_path / "i.db"), str(tmp_path / "ia.db"))
    finally:
        ctx.text_set_chunk(0)
    assert e.value.code == E2BIG


@pytest.mark.parametrize("datas", [[], [b""], [b"\n\njunk\n"]])
def test_streaming_empty_input(ctx, tmp_path, datas):
    rep = stream_build(ctx, tmp_path, datas, parts=2)
    assert rep["records"] == 0 and rep["chunks"] == (1 if datas and datas[0] else 0)
    assert [os.path.getsize(tmp_path / f"kv.db.{p}") for p in range(2)] == [0, 0]
    assert os.path.getsize(tmp_path / "index.db") == 0


# ---- 6. end to end -------------------------------------------------------------------------------------------

N6, PARTS6 = 20_000, 3


@pytest.fixture(scope="module")
def source6():
    rng = np.random.default_rng(61)
    alpha = np.array([b for b in range(256) if b not in (0x0A, 0x0D, 0x20)], np.uint8)
    keys = [b"%d:" % i + alpha[rng.integers(0, alpha.size, int(rng.integers(0, 40)))].tobytes() for i in range(N6)]
    vals = [alpha[rng.integers(0, alpha.size, int(l))].tobytes() for l in rng.integers(1, 201, N6)]
    lines = [k + b" " + v for k, v in zip(keys, vals)]
    junk = [b"novalue%d " % i for i in range(50)] + [b"", b"a b c"]   # "key<sep>": a value of 0 bytes is no record
    for j, l in enumerate(junk):
        lines.insert(int(rng.integers(0, len(lines))), l)
    text = join_lines(lines, rng)
    return {"keys": keys, "vals": vals, "text": text, "absent": [b"absent%d" % i for i in range(2_000)]}


def pack_keys(items):
    off = np.zeros(len(items) + 1, np.uint64)
    off[1:] = np.cumsum([len(k) for k in items])
    return np.frombuffer(b"".join(items), np.uint8), off


@pytest.mark.parametrize("approx", [False, True])
def test_end_to_end(ctx, tmp_path, source6, approx):
    from bsdb_amd.builder import build_text
    from bsdb_amd.native import GET_FOUND
    from bsdb_amd.reader import BSDBReader
    from bsdb_amd.writer import BSDBWriter
    src = tmp_path / "in.txt"
    src.write_bytes(source6["text"])
    d = str(tmp_path / "db")
    rep = build_text(str(src), d, checksum_bits=4, approximate=approx, partitions=PARTS6, verify=True,
                     chunk_bytes=256 << 10)
    _, want = R.restate(source6["text"], b" ")
    assert {k: rep[k] for k in R.FIELDS} == want and rep["records"] == N6 and rep["chunks"] > 1
    assert rep["lines"] == rep["records"] + rep["not_two_fields"] + rep["empty_key"] + rep["too_large"]
    assert sorted(os.listdir(d)) == sorted(["config.properties", "hash.dump", "index.db", "index_a.db"]
                                           + [f"kv.db.{p}" for p in range(PARTS6)])
    # the MPHF does not depend on the order or the path of the adds: the existing writer gives the same hash.dump
    d2 = str(tmp_path / "db_writer")
    w = BSDBWriter(d2, checksum_bits=4, approximate_mode=approx, partitions=PARTS6, fused_index=True)
    for k, v in zip(source6["keys"], source6["vals"]):
        w.put(k, v)
    w.build().close()
    w.close()
    assert open(os.path.join(d, "hash.dump"), "rb").read() == open(os.path.join(d2, "hash.dump"), "rb").read()
    cfg = lambda p: dict(l.split(" = ") for l in open(os.path.join(p, "config.properties")).read().splitlines())  # noqa: E731
    c1, c2 = cfg(d), cfg(d2)
    assert c1.keys() == c2.keys()
    for k in c1:
        assert c1[k] == c2[k] or abs(float(c1[k]) - float(c2[k])) < 1e-9, k
    blob, off = pack_keys(source6["keys"])
    with BSDBReader(d) as rd:
        res = rd.get_batch(blob, off)
        assert (res["status"] == GET_FOUND).all()
        vo = res["voff"].astype(np.int64)
        got = res["values"].tobytes()
        if approx:   # the value heads, through the looked-up ranks
            v8, vl = R.value_heads([(0, k, 0, v) for k, v in zip(source6["keys"], source6["vals"])])
            ranks = rd.mph.lookup_var(blob, off, check=True)
            assert np.array_equal(np.sort(ranks), np.arange(N6))
            slots = np.fromfile(os.path.join(d, "index_a.db"), np.uint64)
            assert np.array_equal(slots[ranks], v8)
            assert all(got[vo[i]:vo[i + 1]] == source6["vals"][i][:8].ljust(8, b"\0") for i in range(N6))
        else:
            assert all(got[vo[i]:vo[i + 1]] == source6["vals"][i] for i in range(N6))
            ab = rd.get_batch(*pack_keys(source6["absent"]))
            assert (ab["status"] != GET_FOUND).all()
            assert os.path.getsize(os.path.join(d, "index_a.db")) == 0


def test_duplicate_key_is_named(ctx, tmp_path, source6):
    from bsdb_amd.builder import build_text
    from bsdb_amd.native import DuplicateKeyError
    lines = [k + b" " + v for k, v in zip(source6["keys"][:3000], source6["vals"][:3000])]
    lines.insert(2500, source6["keys"][17] + b" another_value")
    src = tmp_path / "dup.txt"
    src.write_bytes(b"\n".join(lines) + b"\n")
    with pytest.raises(DuplicateKeyError) as e:
        build_text([str(src)], str(tmp_path / "db"), partitions=PARTS6, chunk_bytes=CHUNK)
    assert e.value.code == EDUP and e.value.keys == [source6["keys"][17]]
    assert e.value.report["found"] == 1


def test_cli_in_a_child_process(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    d = tmp_path / "in"
    d.mkdir()
    (d / "b.txt").write_bytes(b"k3,v3\nbad line\n")
    (d / "a.txt").write_bytes(b"k1,v1\r\nk2,v2")
    out = tmp_path / "db"
    r = subprocess.run([sys.executable, "-m", "bsdb_amd.builder", "-i", str(d), "-o", str(out), "-s", ",", "-cb", "8",
                        "-v", "-p", "2"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "records=3" in r.stdout and "lines=4" in r.stdout and "not_two_fields=1" in r.stdout
    from bsdb_amd.reader import BSDBReader
    with BSDBReader(str(out)) as rd:
        assert [rd.get(k) for k in (b"k1", b"k2", b"k3", b"k4")] == [b"v1", b"v2", b"v3", None]
    assert "hash.checksum.bits = 8" in (out / "config.properties").read_text()


# ---- 7. the device-source add --------------------------------------------------------------------------------

def same_files(a, b):
    return open(a, "rb").read() == open(b, "rb").read()


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a).view(dtype).copy()).cuda()


@pytest.fixture
def key_cap(request):
    if request.param:
        os.environ["BSDB_BUILDER_DEVICE_KEY_BYTES"] = str(request.param)
    yield request.param
    os.environ.pop("BSDB_BUILDER_DEVICE_KEY_BYTES", None)


@pytest.mark.parametrize("key_cap", [0, 100_000], indirect=True)      # 100 000: the builder spills
@pytest.mark.parametrize("approx", [False, True])
def test_device_add_equals_host_add(ctx, tmp_path, source6, key_cap, approx):
    """The same 20 000 keys through add_dev_var, through add_var, and through both mixed in one builder: the
    index files are byte-identical.  Batches after the first have offsets that do not start at 0."""
    blob, off = pack_keys(source6["keys"])
    rng = np.random.default_rng(71)
    addr = rng.integers(0, 1 << 62, N6, dtype=np.uint64)
    v8 = rng.integers(0, 1 << 63, N6, dtype=np.uint64) if approx else None
    vl = rng.integers(0, 9, N6).astype(np.uint8) if approx else None
    d_blob = torch.cat([dev(blob, np.uint8), torch.zeros(16, dtype=torch.uint8, device="cuda")])
    cuts = [0, 7_000, 7_001, 15_000, N6]
    files = {}
    for mode in ("host", "dev", "mixed"):
        b = ctx.builder(0, key_capacity=N6 // 4, blob_capacity=1000, approximate=approx)
        for j, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
            a8 = v8[lo:hi] if approx else None
            al = vl[lo:hi] if approx else None
            if mode == "host" or (mode == "mixed" and j % 2):
                b.add_var(blob, off[lo:hi + 1], addr[lo:hi], a8, al)
            else:
                b.add_dev_var(d_blob, dev(off[lo:hi + 1], np.int64), dev(addr[lo:hi], np.int64),
                              dev(a8, np.int64) if approx else None, dev(al, np.uint8) if approx else None)
        assert b.count() == N6
        files[mode] = (str(tmp_path / f"{mode}_index.db"), str(tmp_path / f"{mode}_index_a.db"))
        m, _ = b.finish(4, *files[mode])
        assert m.info()["n"] == N6
        m.close()
        b.close()
    assert os.path.getsize(files["host"][0]) == 8 * N6
    for mode in ("dev", "mixed"):
        assert same_files(files["host"][0], files[mode][0]) and same_files(files["host"][1], files[mode][1]), mode
