"""GPU: the gather's valid cases of tests/piece_cases.py through
bsdb_dev_db_gather -- the cases tests/test_piece_host_cpu.py runs on the host
emulation, on the hardware: every misalignment x every sequence of one, two or
three value lengths of 0, 1, 8, 15, 16, 17, 33, the wave and workgroup edges,
the runs of empty values.  This ties the emulation to the real kernel: the two
must agree on every one of them.

The sources lie inside the image of one tiny one-partition compact database,
and the truth is the bytes of its kv file at those positions, read back in
Python.  Every output is a view at its misalignment between 0xA5 guards inside
one buffer; a group of cases is launched back to back, then one
synchronisation, one copy back and one check of the whole buffer.  Only valid
scans and sources inside the image run here: nothing hostile goes to the
device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import piece_cases as P  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD = 0xA5
FENCE = 32


@pytest.fixture(scope="module")
def opened(tmp_path_factory):
    """ctx, the open database and its kv file's bytes: 60 records of 100 value bytes, about 6 KB."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from bsdb_amd import Context, kvfiles
    d = tmp_path_factory.mktemp("piece_cases")
    rng = np.random.default_rng(19)
    keys = [b"k%02d" % i for i in range(60)]
    vals = [rng.integers(0, 256, 100, dtype=np.uint8).tobytes() for _ in keys]
    kv, ip = str(d / "kv.db"), str(d / "index.db")
    kblob, koff = kvfiles.pack_values(keys)
    with Context(0) as ctx:
        addr = kvfiles.write_compact(kv, 1, kblob, koff, *kvfiles.pack_values(vals))
        with ctx.mph_build_index_var(kblob, koff, 4, addr, ip) as mph, mph.open_db(kv, 1, ip) as db:
            data = open(kv + ".0", "rb").read()
            assert len(data) == 60 * (3 + 3 + 100) and db.info()["image_bytes"] >= len(data)
            yield ctx, db, data


def gather_all(opened, cases):
    ctx, db, data = opened
    file = np.frombuffer(data, np.uint8)
    srcs, voffs, slots, at = [], [], [], 0
    for c in cases:
        assert c["scale"] == 1 and c["voff"][0] == 0 and c["voff"][-1] == c["value_bytes"] > 0
        src, _ = P.place(c["_vlens"], 1, image_bytes=len(data))
        assert all(s + l <= len(data) for s, l in zip(src, c["_vlens"]))
        srcs.append(src)
        voffs.append(c["voff"])
        slots.append(at + FENCE + c["mis"])                  # the output: FENCE + mis past a 16-byte aligned address
        at += -(-(FENCE + c["mis"] + c["value_bytes"] + FENCE) // 16) * 16
    d_src = torch.from_numpy(np.concatenate(srcs).astype(np.int64)).cuda()
    d_voff = torch.from_numpy(np.concatenate(voffs).astype(np.int64)).cuda()
    big = torch.full((at,), GUARD, dtype=torch.uint8, device="cuda")
    assert big.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    s0 = v0 = 0
    for c, o in zip(cases, slots):
        nq, total = len(c["src"]), c["value_bytes"]
        ctx.db_gather(db, d_src[s0:s0 + nq], d_voff[v0:v0 + nq + 1], values=big[o:o + total], value_bytes=total)
        s0 += nq
        v0 += nq + 1
    torch.cuda.synchronize()
    got = big.cpu().numpy()
    want = np.full(at, GUARD, np.uint8)                      # the guards, and every output where it belongs
    for c, o, src in zip(cases, slots, srcs):
        for s, l, v in zip(src, c["_vlens"], c["voff"]):
            want[o + v:o + v + l] = file[s:s + l]
    bad = np.flatnonzero(got != want)
    if bad.size:
        i = int(np.searchsorted(np.array(slots) - FENCE - 15, bad[0], side="right")) - 1
        raise AssertionError((cases[i]["mis"], cases[i]["_vlens"][:8], "buffer byte", int(bad[0]) - slots[i], "of the output",
                              int(got[bad[0]]), int(want[bad[0]])))


def test_enumeration(opened):
    cases = P.gather_enumeration()
    assert len(cases) == 16 * 396
    gather_all(opened, cases)


def test_wave_and_workgroup_edges(opened):
    cases = P.gather_edges()
    assert {c["value_bytes"] for c in cases} == {1023, 1024, 1025, 4095, 4096, 4097}
    gather_all(opened, cases)


def test_empty_runs(opened):
    gather_all(opened, P.gather_empty_runs())


def test_these_are_the_host_cases():
    """The cases above are, one for one, among those the host emulation runs."""
    host = {(c["mis"], c["scale"], tuple(c["_vlens"])) for c in P.gather_valid()}
    gpu = P.gather_valid_gpu()
    assert len(gpu) == len(P.gather_enumeration()) + len(P.gather_edges()) + len(P.gather_empty_runs())
    assert all((c["mis"], 1, tuple(c["_vlens"])) in host and c["cus"] != 1 for c in gpu)
