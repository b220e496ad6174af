"""GPU: which keys are duplicates (bsdb_*find_duplicates*).

The expected groups are computed here by grouping the key bytes (a dict): no
oracle.  A group of r equal keys is r - 1 pairs (smallest position, other);
where the anchor is unspecified (the builder and kv.db forms, which report
record addresses) groups are compared as sets of sets."""
import os
from collections import defaultdict

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from bsdb_amd import Context
    c = Context(0)
    yield c
    c.close()
    torch.cuda.empty_cache()


# ---- inputs and expectations ---------------------------------------------------
def groups_of(keys):
    """positions grouped by key bytes: the groups of more than one key"""
    d = defaultdict(list)
    for i, k in enumerate(keys):
        d[k].append(i)
    return [g for g in d.values() if len(g) > 1]


def expected_pairs(keys):
    p = sorted((g[0], x) for g in groups_of(keys) for x in g[1:])
    return np.array(p, np.uint64).reshape(len(p), 2)


def pair_groups(pairs):
    """the groups a pair list describes, as a set of frozensets (any anchor)"""
    d = defaultdict(set)
    for a, b in np.asarray(pairs).tolist():
        d[a] |= {a, b}
    return {frozenset(g) for g in d.values()}


def plant(keys, rng):
    """three pairs, one triple, one run of 40, and position 0 again at n - 1:
    copies keys[src] over keys[dst] for disjoint random positions"""
    n = len(keys)
    pos = [int(x) for x in rng.permutation(np.arange(1, n - 1))[: 3 * 2 + 3 + 40]]
    cuts = [pos[0:2], pos[2:4], pos[4:6], pos[6:9], pos[9:49], [0, n - 1]]
    for g in cuts:
        for x in g[1:]:
            keys[x] = keys[g[0]]
    return keys


def fixed_keys(n, key_len, seed):
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 256, (n, key_len), dtype=np.uint8)
    return plant([r.tobytes() for r in raw], rng)


def var_keys(n, seed):
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 65, n)
    keys = plant([rng.integers(0, 256, int(l), dtype=np.uint8).tobytes() for l in lens], rng)
    # near misses: a key that is a prefix of another, two keys differing in the last byte only
    keys[7] = b"near-miss key of some length"
    keys[8] = keys[7][:-3]
    keys[9] = keys[7][:-1] + bytes([keys[7][-1] ^ 1])
    return keys


def dev_fixed(keys):
    a = np.frombuffer(b"".join(keys), np.uint8)
    t = torch.zeros(a.size + 16, dtype=torch.uint8, device="cuda")
    t[: a.size] = torch.from_numpy(a.copy())
    return t[: a.size]


def blob_off(keys):
    off = np.zeros(len(keys) + 1, np.uint64)
    off[1:] = np.cumsum([len(k) for k in keys])
    return np.frombuffer(b"".join(keys), np.uint8).copy(), off


def dev_var(keys):
    blob, off = blob_off(keys)
    t = torch.zeros(blob.size + 16, dtype=torch.uint8, device="cuda")
    t[: blob.size] = torch.from_numpy(blob)
    return t[: blob.size], torch.from_numpy(off.astype(np.int64)).cuda()


@pytest.fixture(scope="module")
def planted_fixed():
    keys = fixed_keys(5000, 13, 1)
    return keys, expected_pairs(keys)


@pytest.fixture(scope="module")
def planted_var():
    keys = var_keys(5000, 2)
    return keys, expected_pairs(keys)


def check_exact(rep, want, n, kind=0):
    assert rep["found"] == len(want) and rep["keys"] == n
    assert not rep["list_full"] and not rep["partial"]
    assert np.array_equal(rep["pairs"], want)
    assert rep["kinds"].tolist() == [kind] * len(want)
    assert rep["collisions"] == (len(want) if kind == 1 else 0)


# ---- the device forms ---------------------------------------------------------
@pytest.mark.parametrize("keys,found", [([], 0), ([b"k" * 13], 0), ([b"k" * 13] * 2, 1), ([b"k" * 13, b"j" * 13], 0)])
@pytest.mark.parametrize("cap", [0, 8])
def test_degenerate(ctx, keys, found, cap):
    t = dev_fixed(keys) if keys else torch.zeros(16, dtype=torch.uint8, device="cuda")[:0]
    rep = ctx.find_duplicates_fixed(t, 13, n=len(keys), cap=cap)
    assert rep["found"] == found and rep["keys"] == len(keys) and not rep["partial"]  # cap = 0 still counts
    assert rep["list_full"] == (found > cap)
    assert rep["pairs"].tolist() == ([[0, 1]] if found and cap else [])


def test_planted_fixed(ctx, planted_fixed):
    keys, want = planted_fixed
    assert len(want) == 3 + 2 + 39 + 1 and [0, len(keys) - 1] in want.tolist()
    check_exact(ctx.find_duplicates_fixed(dev_fixed(keys), 13), want, len(keys))


@pytest.mark.parametrize("key_len", [1, 255])
def test_planted_fixed_shortest_and_longest_keys(ctx, key_len):
    keys = fixed_keys(600, key_len, 3 + key_len)  # (1-byte keys: 256 values, most of the 600 are duplicates)
    check_exact(ctx.find_duplicates_fixed(dev_fixed(keys), key_len), expected_pairs(keys), 600)


def test_planted_var(ctx, planted_var):
    keys, want = planted_var
    blob, off = dev_var(keys)
    rep = ctx.find_duplicates_var(blob, off)
    check_exact(rep, want, len(keys))
    listed = set(rep["pairs"].reshape(-1).tolist())
    assert not listed & {7, 8, 9}  # the prefix and the last-byte near misses are not reported


@pytest.fixture(scope="module")
def ten_thousand():
    keys = fixed_keys(10_000, 13, 5)
    return keys, expected_pairs(keys)


@pytest.mark.parametrize("passes", [1, 3, 7])
def test_multi_pass(ctx, ten_thousand, passes):
    keys, want = ten_thousand  # 7 buckets: one, some, one bucket a pass
    check_exact(ctx.find_duplicates_fixed(dev_fixed(keys), 13, passes=passes), want, len(keys))


@pytest.mark.parametrize("var", [False, True])
def test_above_the_histogram_threshold(ctx, var):
    """from 65 536 keys on the buckets' counts come once from the histogram stage, as in the build"""
    n = 70_000
    if var:
        rng = np.random.default_rng(21)
        raw = rng.integers(0, 256, (n, 40), dtype=np.uint8)
        keys = plant([raw[i, :l].tobytes() for i, l in enumerate(rng.integers(8, 41, n).tolist())], rng)
        rep = ctx.find_duplicates_var(*dev_var(keys), passes=2)
    else:
        keys = fixed_keys(n, 13, 20)
        rep = ctx.find_duplicates_fixed(dev_fixed(keys), 13, passes=2)
    check_exact(rep, expected_pairs(keys), n)


def heavy_keys(copies, distinct, seed):
    rng = np.random.default_rng(seed)
    keys = [r.tobytes() for r in rng.integers(0, 256, (distinct, 13), dtype=np.uint8)] + [b"the same key."] * copies
    order = rng.permutation(len(keys))
    return [keys[i] for i in order]


def test_big_sort_path(ctx):
    """one bucket of 1 665 .. 16 384 keys: k_bucket_sort_big, not partial"""
    keys = heavy_keys(3000, 2000, 6)
    want = expected_pairs(keys)
    assert len(want) == 2999
    check_exact(ctx.find_duplicates_fixed(dev_fixed(keys), 13), want, len(keys))


def test_oversize_bucket(ctx):
    """a bucket over GB_CMAX keys: chunks of GB_CMAX, each losing at most one link"""
    keys = heavy_keys(40_000, 2000, 7)
    same = {i for i, k in enumerate(keys) if k == b"the same key."}
    rep = ctx.find_duplicates_fixed(dev_fixed(keys), 13, cap=64)
    assert rep["list_full"] and rep["keys"] == len(keys)
    assert rep["pairs"].shape == (64, 2) and len({tuple(p) for p in rep["pairs"].tolist()}) == 64
    for a, b in rep["pairs"].tolist():
        assert a in same and b in same and a < b
    assert rep["kinds"].tolist() == [0] * 64
    if rep["partial"]:
        assert 39_997 <= rep["found"] <= 39_999
    else:
        assert rep["found"] == 39_999


def test_list_full(ctx):
    rng = np.random.default_rng(8)
    keys = [r.tobytes() for r in rng.integers(0, 256, (3000, 13), dtype=np.uint8)]
    for j in range(10):
        keys[2000 + j] = keys[j]
    want = {tuple(p) for p in expected_pairs(keys).tolist()}
    rep = ctx.find_duplicates_fixed(dev_fixed(keys), 13, cap=4)
    assert rep["found"] == 10 and rep["list_full"] and not rep["partial"]
    got = {tuple(p) for p in rep["pairs"].tolist()}
    assert len(got) == 4 and got <= want


def test_no_false_positive(ctx):
    n = 1_000_000
    rep = ctx.find_duplicates_fixed(ctx.gen_keys13(0, n), 13)
    assert rep["found"] == 0 and rep["keys"] == n and not rep["list_full"] and not rep["partial"]
    assert rep["pairs"].shape == (0, 2)


def test_signature_form(ctx):
    rng = np.random.default_rng(9)
    sig = rng.integers(-2**63, 2**63 - 1, (4000, 2), dtype=np.int64)
    src, dst = [3, 500, 1999, 2500, 3998], [3999, 7, 2000, 100, 0]
    sig[dst] = sig[src]
    rep = ctx.find_duplicates_sig(torch.from_numpy(sig).cuda())
    want = sorted((min(a, b), max(a, b)) for a, b in zip(src, dst))
    assert rep["found"] == 5 and rep["kinds"] is None and rep["keys"] == 4000
    assert rep["pairs"].tolist() == [list(p) for p in want]


def test_classify(ctx, planted_fixed, planted_var):
    keys, want = planted_fixed
    t = dev_fixed(keys)
    equal = torch.from_numpy(want.astype(np.int64)).cuda()
    assert ctx.classify_pairs_fixed(t, 13, equal).cpu().tolist() == [0] * len(want)
    grouped = {i for g in groups_of(keys) for i in g}
    s = [i for i in range(len(keys)) if i not in grouped][:4]  # keys with one copy
    a0, a1 = sorted({int(p[0]) for p in want})[:2]               # the anchors of two groups
    distinct = np.array([[s[0], s[1]], [s[1], s[0]], [s[2], s[3]], [a0, a1]], np.int64)
    assert ctx.classify_pairs_fixed(t, 13, torch.from_numpy(distinct).cuda()).cpu().tolist() == [1] * 4
    vkeys, vwant = planted_var
    blob, off = dev_var(vkeys)
    assert ctx.classify_pairs_var(blob, off, torch.from_numpy(vwant.astype(np.int64)).cuda()).cpu().tolist() == \
        [0] * len(vwant)
    # different lengths (a prefix), the same length with another last byte, a key against itself
    near = np.array([[7, 8], [8, 7], [7, 9], [7, 7]], np.int64)
    assert len(vkeys[7]) != len(vkeys[8]) and len(vkeys[7]) == len(vkeys[9])
    assert ctx.classify_pairs_var(blob, off, torch.from_numpy(near).cuda()).cpu().tolist() == [1, 1, 1, 0]


# ---- host buffers, the builder, kv.db files, the writer -------------------------
def same_report(a, b):
    return (np.array_equal(a["pairs"], b["pairs"]) and np.array_equal(a["kinds"], b["kinds"]) and
            all(a[k] == b[k] for k in ("found", "collisions", "list_full", "partial", "keys")))


def test_host_forms_equal_the_device_forms(ctx, planted_fixed, planted_var):
    keys, want = planted_fixed
    host = ctx.find_duplicates_fixed_host(np.frombuffer(b"".join(keys), np.uint8), 13)
    check_exact(host, want, len(keys))
    assert same_report(host, ctx.find_duplicates_fixed(dev_fixed(keys), 13))
    vkeys, vwant = planted_var
    vhost = ctx.find_duplicates_var_host(*blob_off(vkeys))
    check_exact(vhost, vwant, len(vkeys))
    assert same_report(vhost, ctx.find_duplicates_var(*dev_var(vkeys)))


@pytest.mark.parametrize("stride", [False, True])
def test_builder(ctx, planted_fixed, stride):
    from bsdb_amd.native import BsdbError
    keys, _ = planted_fixed
    n = len(keys)
    addr = (np.uint64(0x2000) + np.uint64(64) * np.arange(n, dtype=np.uint64) if stride
            else np.random.default_rng(10).permutation(n).astype(np.uint64) * np.uint64(3) + np.uint64(1 << 40))
    want = {frozenset(int(addr[i]) for i in g) for g in groups_of(keys)}
    raw = np.frombuffer(b"".join(keys), np.uint8)
    b = ctx.builder(13, key_capacity=n, **(dict(addr_base=0x2000, addr_stride=64) if stride else {}))
    for lo, hi in ((0, 1000), (1000, 1001), (1001, n)):
        b.add_fixed(raw[13 * lo: 13 * hi], 13, None if stride else addr[lo:hi])
    rep = b.find_duplicates()
    assert pair_groups(rep["pairs"]) == want and rep["found"] == sum(len(g) - 1 for g in want)
    assert rep["kinds"].tolist() == [0] * rep["found"] and rep["keys"] == n and not rep["partial"]
    assert same_report(rep, b.find_duplicates())  # a query: the builder is as it was
    with pytest.raises(BsdbError) as e:
        b.finish(4)
    assert e.value.code == -17  # the build says what it always said
    with pytest.raises(BsdbError) as e:
        b.find_duplicates()
    assert e.value.code == -22
    b.close()


def test_builder_spill(ctx):
    """keys past the device key area: pairs from the spilled (signature, position) segments, no key bytes"""
    n = 200_000
    rng = np.random.default_rng(11)
    raw = rng.integers(0, 256, (n, 13), dtype=np.uint8)
    plants = [(5, 150_000), (70_000, 70_001), (199_999, 3)]
    for a, c in plants:
        raw[c] = raw[a]
    keys = [r.tobytes() for r in raw]
    addr = np.arange(n, dtype=np.uint64) * np.uint64(16) + np.uint64(7)
    want = {frozenset(int(addr[i]) for i in g) for g in groups_of(keys)}
    assert len(want) == 3
    os.environ["BSDB_BUILDER_DEVICE_KEY_BYTES"] = "1000000"
    try:
        b = ctx.builder(13, key_capacity=n // 8)
    finally:
        os.environ.pop("BSDB_BUILDER_DEVICE_KEY_BYTES", None)
    flat = raw.reshape(-1)
    for lo in range(0, n, 50_000):
        b.add_fixed(flat[13 * lo: 13 * (lo + 50_000)], 13, addr[lo: lo + 50_000])
    rep = b.find_duplicates()
    assert rep["found"] == 3 and rep["keys"] == n and pair_groups(rep["pairs"]) == want
    assert rep["kinds"].tolist() == [2, 2, 2] and rep["collisions"] == 0
    b.close()


@pytest.mark.parametrize("fmt", [0, 1])
def test_kv_files(ctx, tmp_path, fmt):
    from bsdb_amd import kvfiles
    from bsdb_amd.native import kv_scan
    n = 20_000
    rng = np.random.default_rng(12 + fmt)
    raw = rng.integers(0, 256, (n, 13), dtype=np.uint8)
    for a, c in ((10, 11), (200, 15_001), (19_999, 0), (7000, 7003)):  # record i lies in partition i % 2
        raw[c] = raw[a]
    keys = [r.tobytes() for r in raw]
    kb, ko = blob_off(keys)
    vb, vo = kvfiles.pack_values([b"v%d" % i for i in range(n)])
    base = str(tmp_path / "kv.db")
    (kvfiles.write_blocked(base, 2, kb, ko, vb, vo, 4096) if fmt else kvfiles.write_compact(base, 2, kb, ko, vb, vo))
    scan = kv_scan(base, 2, fmt, 4096)
    so = scan["offsets"].astype(np.int64)
    scanned = [scan["blob"][so[i]: so[i + 1]].tobytes() for i in range(n)]
    want = {frozenset(int(scan["addr"][i]) for i in g) for g in groups_of(scanned)}
    assert len(want) == 4
    rep = ctx.kv_find_duplicates(base, 2, fmt, 4096)
    assert rep["found"] == 4 and rep["keys"] == n and pair_groups(rep["pairs"]) == want
    assert rep["kinds"].tolist() == [0] * 4


@pytest.mark.parametrize("from_files", [False, True])
def test_writer_raises_duplicate_key_error(tmp_path, from_files):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from bsdb_amd.native import BsdbError, DuplicateKeyError
    from bsdb_amd.writer import BSDBWriter
    w = BSDBWriter(str(tmp_path), partitions=2, from_files=from_files)
    try:
        for i in range(500):
            w.put(b"key-%05d" % i, b"value-%d" % i)
        w.put(b"key-00123", b"again")
        with pytest.raises(BsdbError) as e:  # (code that catches BsdbError and checks .code keeps working)
            w.build()
        assert isinstance(e.value, DuplicateKeyError) and e.value.code == -17
        assert e.value.keys == [b"key-00123"] and e.value.report["found"] == 1
        assert "key-00123" in str(e.value)
    finally:
        w.close()
