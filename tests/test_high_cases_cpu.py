"""CPU: tests/high_cases.py pinned without a device.  A small directory written
with locate_cases' helpers is relocated by small shifts, and every word of the
new index.db is decoded with locate_cases.decode and read with record_rule over
np.memmaps of the new files: it names a record with the same key and the same
value as before.  straddle_shift is pinned against a worked example, and a
relocated file of 2^32 + 1 MiB bytes must have that size and cost no time."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import high_cases as H  # noqa: E402
import locate_cases as L  # noqa: E402

LAYOUTS = {"compact3": (3, 0, 4096, (777, 0, 5)), "blocked4096": (2, 1, 4096, (3 * 4096, 4096)),
           "blocked8192": (2, 1, 8192, (3 * 4096, 4096))}


def small_dir(d, parts, fmt, block, n=300):
    """n records (a few larger than a block) written with write_files, index.db by the oracle's MPHF, and two
    files that stand for hash.dump and the config.  Returns (keys, values, rank of every key)."""
    rng = np.random.default_rng(7 + parts + block)
    keys = L.distinct_keys(rng, n, list(range(1, 41)) + [255])
    lens = rng.integers(0, 200, n)
    lens[::37] = rng.integers(5000, 20000, lens[::37].size)
    vals = [L.rand_bytes(rng, l) for l in lens]
    os.makedirs(d)
    addr = L.write_files(os.path.join(d, "kv.db"), keys, vals, parts, fmt, block)
    mph = L.mph_of(L.sigs_of(keys), 4)
    rank = L.ranks(mph, L.sigs_of(keys))
    assert sorted(rank.tolist()) == list(range(n))
    index = [0] * n
    for i in range(n):
        index[rank[i]] = int(addr[i])
    np.array(L.be(index), np.uint64).tofile(os.path.join(d, "index.db"))
    assert np.fromfile(os.path.join(d, "index.db"), ">u8").tolist() == index
    with open(os.path.join(d, "hash.dump"), "wb") as f:
        f.write(L.rand_bytes(rng, 999))
    with open(os.path.join(d, "config.properties"), "w") as f:
        f.write("kv.count = %d\n" % n)
    return keys, vals, rank


def read_all(d, parts, fmt, keys, rank):
    """(status, value) per key through the directory's index.db, the decode and the record's rule."""
    files = [np.memmap(os.path.join(d, f"kv.db.{p}"), np.uint8, "r") for p in range(parts)]
    sizes = [f.size for f in files]
    index = np.fromfile(os.path.join(d, "index.db"), ">u8").tolist()
    out = []
    for key, r in zip(keys, rank.tolist()):
        dec = L.decode(index[r], fmt, sizes)
        assert dec is not None
        part, pos, limit = dec
        st, vpos, vlen = L.record_rule(files[part], limit, pos, key)
        out.append((st, bytes(files[part][vpos: vpos + vlen])))
    return out, sizes


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_relocated_records_are_the_same_records(tmp_path, layout):
    parts, fmt, block, shifts = LAYOUTS[layout]
    src, dst = str(tmp_path / "src"), str(tmp_path / "dst")
    keys, vals, rank = small_dir(src, parts, fmt, block)
    before, old_sizes = read_all(src, parts, fmt, keys, rank)
    assert before == [(L.FOUND, v) for v in vals]
    new_sizes = H.relocate(src, dst, parts, fmt, block, shifts)
    assert new_sizes == [s + o for s, o in zip(shifts, old_sizes)]
    after, sizes = read_all(dst, parts, fmt, keys, rank)
    assert sizes == new_sizes and after == before
    for p in range(parts):                                            # a hole of zeros, then the original bytes
        f = open(os.path.join(dst, f"kv.db.{p}"), "rb").read()
        assert f[:shifts[p]] == bytes(shifts[p]) and f[shifts[p]:] == open(os.path.join(src, f"kv.db.{p}"), "rb").read()
    old, new = (np.fromfile(os.path.join(d, "index.db"), ">u8").astype(np.uint64) for d in (src, dst))
    part = (old >> np.uint64(56)).astype(np.int64)
    step = np.array([s if fmt == 0 else (s // 4096) << 16 for s in shifts], np.uint64)
    assert np.array_equal(new - old, step[part]) and np.array_equal(new >> np.uint64(56), old >> np.uint64(56))
    assert len(set(part.tolist())) == parts
    for name in ("hash.dump", "config.properties"):
        assert open(os.path.join(dst, name), "rb").read() == open(os.path.join(src, name), "rb").read()
    assert sorted(os.listdir(dst)) == sorted(os.listdir(src))


def test_blocked_shift_must_be_whole_pages(tmp_path):
    src = str(tmp_path / "src")
    small_dir(src, 2, 1, 4096, n=20)
    with pytest.raises(AssertionError):
        H.relocate(src, str(tmp_path / "dst"), 2, 1, 4096, (4096, 100))


def test_straddle_shift_worked_example():
    """A record at file offset 1000 with a 20-byte key: its header's second byte (x = 1) lands on 2^32 with a shift
    of 4 294 966 295; byte 10 of its key is record byte 3 + 10."""
    assert H.straddle_shift(1000, 1) == 4_294_966_295
    assert 1000 + 1 + H.straddle_shift(1000, 1) == 1 << 32
    assert H.straddle_shift(1000, 3 + 10) == 4_294_966_283
    assert H.straddle_shift(0, 0) == 1 << 32
    base, _ = L.layout([H.straddle_shift(1000, 1) + 5000, 70])       # partition 0 lies at image position 0
    assert base[0] == 0 and base[1] >= 1 << 32


def test_a_file_beyond_4_gib_costs_nothing(tmp_path):
    src, dst = str(tmp_path / "src"), str(tmp_path / "dst")
    keys, vals, rank = small_dir(src, 1, 0, 4096, n=50)
    size = os.path.getsize(os.path.join(src, "kv.db.0"))
    want = (1 << 32) + (1 << 20)
    t0 = time.perf_counter()
    sizes = H.relocate(src, dst, 1, 0, 4096, (want - size,))
    dt = time.perf_counter() - t0
    assert sizes == [want] and os.stat(os.path.join(dst, "kv.db.0")).st_size == want
    assert dt < 1.0, dt
    after, _ = read_all(dst, 1, 0, keys, rank)                        # every address is >= 2^32 - (the file's bytes)
    assert after == [(L.FOUND, v) for v in vals]
    index = np.fromfile(os.path.join(dst, "index.db"), ">u8")
    assert int(index.min()) >= want - size and int(index.max()) >= 1 << 32
