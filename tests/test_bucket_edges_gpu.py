"""Signatures on bucket boundaries.  bucket = hi64((sig0 >>> 1) * 2m) is computed
from 32-bit halves by bucket_of_w and its copies (the grouping kernels of the
SMALL, MID and LARGE classes, mph_rank, owner_of's callers); an off-by-one at an
exact boundary has probability about m / 2^63 per random key, so random
signatures never see one.  Here the signatures sit on the boundaries: for m
buckets the first value of sig0 >>> 1 in bucket b is x_b = ceil(b * 2^63 / m),
and sig0 takes 2 x_b - 1 (the last of bucket b - 1), 2 x_b and 2 x_b + 1 (the
first two of bucket b).  The reference arithmetic is exact Python integers; the
oracle is pinned to it first.  Every comparison is exact."""
import functools

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

THREADS = O.cpu_threads()
EXTREMES = [0, 1, 2**63 - 1, 2**63, 2**64 - 2, 2**64 - 1]


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from bsdb_amd import Context
    c = Context(0)
    yield c
    c.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def bucket_int(sig0, m):
    """multiplyHigh(sig0 >>> 1, 2m) in exact integers."""
    return ((int(sig0) >> 1) * (2 * m)) >> 64


def buckets_int(sig, m):
    return np.array([bucket_int(s, m) for s in sig[:, 0]], np.int64)


def boundary_sig0(m, bs):
    out = []
    for b in bs:
        x = -((-b << 63) // m)  # ceil(b * 2^63 / m)
        assert bucket_int(2 * x - 1, m) == b - 1 and bucket_int(2 * x, m) == b == bucket_int(2 * x + 1, m)
        out += [2 * x - 1, 2 * x, 2 * x + 1]
    return out


def boundaries_of(m):
    """Every b when m is small, else 2000 values spread over [1, m) and m - 1."""
    if m <= 4000:
        return list(range(1, m))
    return sorted(set(int(b) for b in np.linspace(1, m - 1, 2000).astype(np.int64)) | {m - 1})


def crafted(m, n, seed, bs=None):
    """n distinct signatures: sig0 on the boundaries `bs` of m buckets and on
    the extremes of its range, random sig1, random fill (shuffled).  Returns
    (sig, a mask of the crafted ones)."""
    rng = np.random.default_rng(seed)
    s0 = sorted(set(boundary_sig0(m, boundaries_of(m) if bs is None else bs) + EXTREMES))
    assert len(s0) <= n
    fill = rng.integers(0, 1 << 64, 2 * (n - len(s0)) + 16, dtype=np.uint64)
    fill = fill[~np.isin(fill, np.array(s0, np.uint64))]
    fill = fill[np.sort(np.unique(fill, return_index=True)[1])][: n - len(s0)]
    sig = np.empty((n, 2), np.uint64)
    sig[:, 0] = np.concatenate([np.array(s0, np.uint64), fill])
    sig[:, 1] = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    perm = rng.permutation(n)
    sig = np.ascontiguousarray(sig[perm])
    is_crafted = perm < len(s0)
    # the oracle agrees with the integer formula on these signatures
    np.testing.assert_array_equal(O.buckets(sig, m).astype(np.int64), buckets_int(sig, m))
    return sig, is_crafted


# ---- SMALL class: the whole build ------------------------------------------------

@pytest.mark.parametrize("n", [3001, 20_000])
def test_gov_build_small_class(ctx, n):
    m, width = n // 1500 + 1, 5
    assert m == O.num_buckets(n)
    sig, is_crafted = crafted(m, n, n)
    rc, E, values, sigbits = O.gov_build(sig, width)
    assert rc == 0
    # E is the histogram of the integer formula's buckets
    np.testing.assert_array_equal(E[1:] & np.uint64((1 << 56) - 1), np.cumsum(np.bincount(buckets_int(sig, m), minlength=m)))
    dsig = dev(sig.view(np.int64))
    dE, dv, dsb = ctx.gov_build(dsig, width)
    np.testing.assert_array_equal(u64(dE), E)
    np.testing.assert_array_equal(u64(dv), values)
    np.testing.assert_array_equal(u64(dsb), sigbits)
    got = ctx.lookup(dsig, n, dE, dv, width, dsb, check=False).cpu().numpy()
    np.testing.assert_array_equal(got, O.lookup_batch(sig, n, E, values, width, sigbits, False))
    np.testing.assert_array_equal(np.sort(got), np.arange(n))
    checked = ctx.lookup(dsig, n, dE, dv, width, dsb, check=True).cpu().numpy()
    np.testing.assert_array_equal(checked[is_crafted], got[is_crafted])


# ---- MID and LARGE classes: range builds -----------------------------------------

# the interior range of each structure; its edges join the crafted boundaries
INTERIOR = {7_000_000: (200, 4_500), 121_500_000: (500, 80_600)}


@functools.lru_cache(maxsize=None)
def range_set(n_global):
    """300 000 local signatures of a structure on n_global keys, the crafted ones among them."""
    m = O.num_buckets(n_global)
    bs = sorted(set(boundaries_of(m)) | set(INTERIOR[n_global]))
    sig, is_crafted = crafted(m, 300_000, n_global % 1000, bs)
    return m, sig, is_crafted, buckets_int(sig, m)


# MID: 4 096 < buckets <= 80 000 (k_bucket_count_mid); LARGE: more (per-key atomics).
# The interior ranges put signatures on b_lo's and b_hi's boundaries on both sides.
@pytest.mark.parametrize("n_global,b_lo,b_hi", [(7_000_000, 0, 4_667), (7_000_000, 200, 4_500),
                                                (121_500_000, 0, 81_001), (121_500_000, 500, 80_600)])
def test_range_build_mid_and_large_class(ctx, n_global, b_lo, b_hi):
    m, sig, is_crafted, b_of = range_set(n_global)
    assert b_hi <= m and (b_hi == m) == (b_lo == 0)
    nb = b_hi - b_lo
    assert 4096 < nb <= 80_000 if n_global == 7_000_000 else nb > 80_000
    width = 4
    keep = (b_of >= b_lo) & (b_of < b_hi)  # by the integer formula
    part = np.ascontiguousarray(sig[keep])
    e_lo = int((b_of < b_lo).sum())
    if b_lo:
        # the range's edges are among the crafted boundaries: keys on both sides of each
        assert (b_lo, b_hi) == INTERIOR[n_global]
        for b in (b_lo, b_hi):
            assert (b_of == b - 1).sum() >= 1 and (b_of == b).sum() >= 2
    vw, sw = int(O.lib().bo_values_words(n_global)), (n_global * width + 63) // 64 + 1
    E, vals, sb = np.zeros(m + 1, np.uint64), np.zeros(vw, np.uint64), np.zeros(sw, np.uint64)
    assert O.gov_build_range(part, n_global, b_lo, b_hi, e_lo, width, E, vals, sb, THREADS) == 0
    dE = torch.zeros(m + 1, dtype=torch.int64, device="cuda")
    dv = torch.zeros(vw, dtype=torch.int64, device="cuda")
    ds = torch.zeros(sw, dtype=torch.int64, device="cuda")
    rk = torch.zeros(part.shape[0], dtype=torch.int64, device="cuda")
    dpart = dev(part.view(np.int64))
    ctx.gov_build_range(dpart, n_global, b_lo, b_hi, e_lo, width, dE, dv, ds, rank=rk)
    np.testing.assert_array_equal(u64(dE), E)
    np.testing.assert_array_equal(u64(dv), vals)
    np.testing.assert_array_equal(u64(ds), sb)
    E_look = E.copy()
    E_look[b_hi] = max(int(E_look[b_hi]), e_lo + part.shape[0])  # (an interior range leaves E[b_hi] to the next one)
    want = O.lookup_batch(part, n_global, E_look, vals, width, sb, False)
    np.testing.assert_array_equal(rk.cpu().numpy(), want)
    np.testing.assert_array_equal(np.sort(want), e_lo + np.arange(part.shape[0]))
    # the lookup kernel on the same structure, the crafted signatures among the queries
    assert is_crafted[keep].sum() > 5000
    got = ctx.lookup(dpart, n_global, dev(E_look.view(np.int64)), dv, width, ds, check=False).cpu().numpy()
    np.testing.assert_array_equal(got, want)


# ---- ownership ---------------------------------------------------------------------

# m = 2^31 - 1 is the largest the ABI accepts: mult = 2m is near 2^32
@pytest.mark.parametrize("G", [2, 3, 64])
@pytest.mark.parametrize("m", [2, 667, 81_001, 2**31 - 1])
def test_partition_owners(ctx, m, G):
    firsts = sorted({g * m // G for g in range(1, G)} - {0})  # the owners' first buckets
    bs = sorted(set(firsts) | set(boundaries_of(m)[:: 40 if m > 4000 else 1]))
    n = 20_000
    sig, _ = crafted(m, n, m % 997 + G, bs)
    b_of = buckets_int(sig, m)
    own = ((b_of + 1) * G - 1) // m
    for g in range(1, G):  # rank g owns [g m / G, (g + 1) m / G)
        assert np.all((own >= g) == (b_of >= g * m // G))
    want_counts = [int((own == g).sum()) for g in range(G)]
    for b in firsts:
        assert (b_of == b - 1).sum() >= 1 and (b_of == b).sum() >= 2
    payload = torch.arange(n, dtype=torch.int64, device="cuda")
    out, pout, counts = ctx.partition_owners(dev(sig.view(np.int64)), m, G, payload=payload)
    assert counts == want_counts
    got, pay = u64(out), pout.cpu().numpy()
    np.testing.assert_array_equal(got, sig[pay])  # the payload travels with its signature
    start = 0
    for g in range(G):
        seg = got[start: start + counts[g]]
        mine = sig[own == g]
        np.testing.assert_array_equal(seg[np.lexsort((seg[:, 1], seg[:, 0]))], mine[np.lexsort((mine[:, 1], mine[:, 0]))])
        start += counts[g]
