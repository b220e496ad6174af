"""GPU: the valid cases of tests/locate_cases.py -- the cases
tests/test_locate_host_cpu.py runs on the host emulation under ASan + UBSan --
on the hardware, through the library's own entry points: mph_import and
open_db, bsdb_dev_db_locate_* and bsdb_db_get_*, bsdb_dev_lookup, bsdb_dev_sign,
bsdb_dev_index_scatter, bsdb_dev_verify_*.  This ties the emulation to the real
kernels: the two must agree with the same restatement, exactly, on every one of
them.  (The emulation proves addressing, arithmetic and uniform control flow;
the memory model, races between lanes, code generation and speed are judged
here and by the rest of the GPU suite.)

Only the valid cases: nothing hostile goes to the device.  The largest input
is 3001 keys and an image of a few hundred KB.  The launches of a group are
enqueued back to back and read back after one synchronisation."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import locate_cases as L  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MASK = (1 << 64) - 1


def dev(values, dtype=np.uint64):
    """A device tensor of these numbers (u64 as int64 bits); never a null pointer."""
    a = np.array([int(v) for v in values] + [0], dtype)
    if dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).cuda()[: len(values)]


def dev_keys(blob: bytes, kmis: int):
    """The key bytes at `kmis` bytes past a 16-byte aligned device address."""
    buf = torch.zeros(kmis + len(blob) + 16, dtype=torch.uint8, device="cuda")
    view = buf[kmis: kmis + len(blob)]
    if blob:
        view.copy_(torch.from_numpy(np.frombuffer(blob, np.uint8).copy()))
    assert view.data_ptr() % 16 == kmis
    return view


def u64(t):
    return [int(x) & MASK for x in t.cpu().tolist()]


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from bsdb_amd import Context
    with Context(0) as c:
        yield c


def mph_tensors(mph):
    return dev(mph["E"]), dev(mph["values"]), dev(mph["sigbits"]) if mph["width"] else None


def test_locate_and_get(ctx, tmp_path):
    cases = L.locate_valid()
    opened, pending = {}, []
    try:
        for c in cases:
            mph, image = c["_mph"], c["_image"]
            key = (id(mph), id(image), c["approx"])
            if key not in opened:
                d = tmp_path / f"db{len(opened)}"
                d.mkdir()
                m = ctx.mph_import(mph["n"], mph["width"], mph["E"], mph["values"], mph["sigbits"] if mph["width"] else None)
                if c["approx"]:
                    slots = np.random.default_rng(mph["n"]).integers(0, 256, 8 * mph["n"], dtype=np.uint8)
                    slots.tofile(str(d / "index_a.db"))
                    db = m.open_db(None, 0, str(d / "index_a.db"), approximate=True)
                    opened[key] = (m, db, slots.tobytes())
                else:
                    for p, f in enumerate(image.files):
                        (d / f"kv.db.{p}").write_bytes(f)
                    np.array(c["_index"], ">u8").tofile(str(d / "index.db"))
                    db = m.open_db(str(d / "kv.db"), len(image.files), str(d / "index.db"), fmt=image.fmt, block_size=image.block or L.PAGE)
                    assert db.info()["image_bytes"] == image.total
                    opened[key] = (m, db, image.bytes)
                first = True
            else:
                first = False
            m, db, data = opened[key]
            keys = dev_keys(c["keys"], c["kmis"])
            if c["_kind"] == 2:
                out = ctx.db_locate_var(db, keys, dev(c["off"]))
            else:
                out = ctx.db_locate_fixed(db, keys, c["key_len"], c["nq"])
            pending.append((c, out, keys))
            if first and c["nq"]:             # the host form once per database: the value bytes too
                st, src, vl, rep = L.locate_expected(c)
                scale = 8 if c["approx"] else 1
                blob, off = L.pack(c["_keys"])
                res = db.get_var(blob, off) if c["_kind"] == 2 else db.get_fixed(blob, c["key_len"])
                assert res["status"].tolist() == st, c["_name"]
                assert res["voff"].tolist() == [0] + np.cumsum(vl).tolist(), c["_name"]
                assert res["values"].tobytes() == b"".join(data[s * scale: s * scale + l] for s, l in zip(src, vl)), c["_name"]
                assert list(res["report"].values()) == rep, c["_name"]
        torch.cuda.synchronize()
        for c, (src, vlen, status, report), _ in pending:
            st, want_src, vl, rep = L.locate_expected(c)
            assert status.cpu().tolist() == st, c["_name"]
            assert u64(src) == want_src and vlen.cpu().tolist() == vl, c["_name"]
            assert u64(report) == rep, c["_name"]
    finally:
        for m, db, _ in opened.values():
            db.close()
            m.close()


def test_lookup_and_sign(ctx):
    cases, pending, tensors = L.mph_valid(), [], {}
    for c in cases:
        mph = c["_mph"]
        if id(mph) not in tensors:
            tensors[id(mph)] = mph_tensors(mph)
        E, values, sigbits = tensors[id(mph)]
        sig = dev(c["sig"]).reshape(-1, 2)
        assert sig.data_ptr() % 16 == 0
        if c["mode"] == "lookup":
            out = ctx.lookup(sig, mph["n"], E, values, mph["width"], sigbits, bool(c["check"]))
        else:
            out = ctx.sign(sig, E, values, mph["width"])
            assert out.numel() == c["words"]
        pending.append((c, out, sig))
    torch.cuda.synchronize()
    for c, out, _ in pending:
        if c["mode"] == "lookup":
            assert out.cpu().tolist() == L.lookup_expected(c), c["_name"]
        else:
            assert u64(out) == L.sign_expected(c), c["_name"]


def test_index_scatter(ctx):
    pending = []
    for c in L.scatter_valid():
        fill = int.from_bytes(bytes([c["fill"]]) * 8, "little")
        index = dev([fill] * (c["len"] + 1))   # one spare slot: the pointer is not null when the window is empty
        args = [dev(c["rank"], np.int64), dev(c["addr"]), c["start"], c["len"], index]
        index_a = None
        if c["approx"]:
            index_a = torch.full((8 * c["len"] + 8,), c["fill"], dtype=torch.uint8, device="cuda")
            args += [dev(c["value8"]), dev(c["value_len"], np.uint8), index_a]
        ctx.index_scatter(*args)
        pending.append((c, index, index_a, args))
    torch.cuda.synchronize()
    for c, index, index_a, _ in pending:
        want, want_a = L.scatter_expected(c)
        spare = bytes([c["fill"]]) * 8
        assert u64(index) == want + [int.from_bytes(spare, "little")], c["_name"]
        if c["approx"]:
            assert index_a.cpu().numpy().tobytes() == want_a + spare, c["_name"]


def test_verify(ctx):
    cases, pending, tensors = L.verify_valid(), [], {}
    for c in cases:
        mph = c["_mph"]
        if id(mph) not in tensors:
            tensors[id(mph)] = mph_tensors(mph)
        E, values, sigbits = tensors[id(mph)]
        out = ctx.verify_out("cuda")
        keys = dev_keys(c["keys"], c["kmis"])
        approx = "index_a" in c
        kw = dict(start=c["start"], length=c["len"], width=mph["width"], sigbits=sigbits, addr=dev(c["addr"]) if "addr" in c else None,
                  addr_base=c["addr_base"], addr_stride=c["addr_stride"], first=c["first"],
                  value8=dev(c["value8"]) if approx else None, vlen=dev(c["vlen"], np.uint8) if approx else None,
                  index_a=dev(c["index_a"]) if approx else None, out=out)
        if "off" in c:
            ctx.verify_var(keys, dev(c["off"]), mph["n"], E, values, dev(c["index"]), **kw)
        else:
            ctx.verify_fixed(keys, c["key_len"], mph["n"], E, values, dev(c["index"]), **kw)
        pending.append((c, out))
    torch.cuda.synchronize()
    for c, out in pending:
        assert u64(out) == L.verify_expected(c), c["_name"]


def test_these_are_the_host_cases():
    """What runs above is what tests/test_locate_host_cpu.py runs as its valid cases, and none of its hostile ones."""
    import test_locate_host_cpu as H
    valid = {id(c) for f in (L.locate_valid, L.mph_valid, L.scatter_valid, L.verify_valid) for c in f()}
    hostile = {id(c) for c in H.hostile_all() + L.accepted_offset_cases() + H.refused_cases()}
    assert valid and not valid & hostile
    assert all(L.structure_valid(c["_mph"]["E"], c["n"]) for f in (L.locate_valid, L.mph_valid, L.verify_valid) for c in f())
