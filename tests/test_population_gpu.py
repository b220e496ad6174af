"""GPU: bucket populations and signature ties random keys never produce (tests/population_cases.py; the table is
pinned on the CPU by tests/test_population_cases_cpu.py): buckets of exactly GS_CMAX, GM_CMAX and GB_CMAX keys
and one more, empty, one-key and tiny buckets between full ones, ties and clusters in sig0.  The oracle is the
specification of E, values, checksum bits and ranks; exact integers (the bincount of the bucket formula) and a
dict grouping are the specification of the rest.  Every comparison is exact."""
import functools
import time

import numpy as np
import pytest

import oracle as O
import population_cases as P
from bsdb_amd.native import BsdbError

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

E2BIG, EDUP = -7, -17


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from bsdb_amd import Context
    c = Context(0)
    yield c
    c.close()


def dev(a):
    """A signature set (uint64 [n, 2]) on the device, as the int64 tensor the calls take."""
    return torch.from_numpy(np.array(a, np.uint64).view(np.int64)).cuda()


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def offsets_of(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)


def sign_words(sig, ranks, width):
    """signatures[rank(sig)] = sig0 & mask as the packed width-bit list of (n width + 63) / 64 + 1 words."""
    words = (len(sig) * width + 63) // 64 + 1
    bits, mask = 0, (1 << width) - 1
    for s0, r in zip(sig[:, 0].tolist(), ranks.tolist()):
        bits |= (s0 & mask) << (r * width)
    assert bits >> (64 * words) == 0
    return np.array([(bits >> (64 * i)) & P.U64 for i in range(words)], np.uint64)


def check_structure(ctx, sig, dsig, counts, width, dE, dv, dsb, rank):
    """What holds of a build whatever the oracle says: E is the bincount's cumsum, the ranks are a bijection,
    the lookup kernel (with the checksum compare) finds them again, the checksum bits are sig0's at each rank."""
    n = len(sig)
    np.testing.assert_array_equal(u64(dE) & np.uint64(P.OFFSET_MASK), offsets_of(counts))
    np.testing.assert_array_equal(np.sort(rank), np.arange(n))
    got = ctx.lookup(dsig, n, dE, dv, width, dsb, check=True).cpu().numpy()
    np.testing.assert_array_equal(got, rank)
    if width:
        want = sign_words(sig, rank, width)
        np.testing.assert_array_equal(u64(dsb), want)
        np.testing.assert_array_equal(u64(ctx.sign(dsig, dE, dv, width)), want)


# ---- 1. build parity -----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def oracle_build(name, width):
    _, _, sig = P.case(name)
    rc, E, values, sigbits = O.gov_build(sig, width)
    assert rc == 0
    return E, values, sigbits, O.lookup_batch(sig, len(sig), E, values, width, sigbits, False)


WIDE = ("small_limit", "tiny_ladder", "ties8_4400")
BUILDS = [(name, w) for name in sorted(P.CASES) if name != "range_profile" for w in (0, 5)] + [(name, 64) for name in WIDE]


@pytest.mark.parametrize("name,width", BUILDS)
def test_build_matches_oracle(ctx, name, width):
    counts, _, sig = P.case(name)
    E, values, sigbits, ranks = oracle_build(name, width)
    dsig = dev(sig)
    dE, dv, dsb, drank = ctx.gov_build_ranks(dsig, width)
    np.testing.assert_array_equal(u64(dE), E)
    np.testing.assert_array_equal(u64(dv), values)
    if width:
        np.testing.assert_array_equal(u64(dsb), sigbits)
    rank = drank.cpu().numpy()
    np.testing.assert_array_equal(rank, ranks)
    check_structure(ctx, sig, dsig, counts, width, dE, dv, dsb, rank)


# ---- 2. the limit of the global-slab solver ------------------------------------------------------------------------

def test_bucket_over_the_limit_is_refused(ctx):
    """16 385 keys in one bucket: BSDB_E2BIG from both builds (the oracle has no limit and solves it)."""
    counts, _, sig = P.case("over_limit")
    assert counts[0] == P.GB_CMAX + 1
    dsig = dev(sig)
    for build in (ctx.gov_build, ctx.gov_build_ranks):
        with pytest.raises(BsdbError) as e:
            build(dsig, 5)
        assert e.value.code == E2BIG


def test_bucket_on_the_limit_builds(ctx):
    """16 384 keys in one bucket: the bitonic sort pads to the count itself, the solver's slab is full.  By the
    properties alone (the oracle needs 12 s of CPU for this set)."""
    counts, _, sig = P.case("big_limit")
    assert counts[0] == P.GB_CMAX
    dsig = dev(sig)
    t0 = time.perf_counter()
    dE, dv, dsb, drank = ctx.gov_build_ranks(dsig, 5)
    torch.cuda.synchronize()
    print(f"16384-key bucket: gov_build_ranks took {time.perf_counter() - t0:.2f} s")
    check_structure(ctx, sig, dsig, counts, 5, dE, dv, dsb, drank.cpu().numpy())
    dE2, dv2, dsb2 = ctx.gov_build(dsig, 5)       # the build without ranks gives the same structure
    assert torch.equal(dE2, dE) and torch.equal(dv2, dv) and torch.equal(dsb2, dsb)


# ---- 3. range and window builds over a profile with empty and tiny buckets ------------------------------------------

@pytest.mark.parametrize("b_lo,b_hi", [(1, 6), (2, 5), (0, 7)])
def test_range_and_window_builds(ctx, b_lo, b_hi):
    """[1, 6): an interior range whose first and last buckets are empty and whose others hold 11 .. 13 keys;
    [2, 5): the same without the empty ones, so a tiny bucket is first and another last; [0, 7): the full range.
    The range build into full-size arrays against the oracle's, then the window build between 64 sentinel words
    on both sides against the slices."""
    from bsdb_amd.native import range_windows
    counts, _, sig = P.case("range_profile")
    n, m, width, guard = len(sig), len(counts), 5, 64
    assert counts == [2, 0, 11, 12, 13, 0, 8962] and n // 1500 + 1 == m
    b_of = P.buckets_int(sig, m)
    part = np.ascontiguousarray(sig[(b_of >= b_lo) & (b_of < b_hi)])
    e_lo, n_local = sum(counts[:b_lo]), sum(counts[b_lo:b_hi])
    assert len(part) == n_local
    assert [counts[b_lo], counts[b_hi - 1]] == {1: [0, 0], 2: [11, 13], 0: [2, 8962]}[b_lo]
    vw_full, sw_full = int(O.lib().bo_values_words(n)), (n * width + 63) // 64 + 1
    E, vals, sb = np.zeros(m + 1, np.uint64), np.zeros(vw_full, np.uint64), np.zeros(sw_full, np.uint64)
    assert O.gov_build_range(part, n, b_lo, b_hi, e_lo, width, E, vals, sb, 1) == 0
    off = offsets_of(counts)
    owned = slice(b_lo, b_hi + 1 if b_hi == m else b_hi)   # (an interior range leaves E[b_hi] to the next one)
    np.testing.assert_array_equal(E[owned] & np.uint64(P.OFFSET_MASK), off[owned])
    dpart = dev(part)
    full = [torch.zeros(k, dtype=torch.int64, device="cuda") for k in (m + 1, vw_full, sw_full)]
    rk = torch.zeros(max(n_local, 1), dtype=torch.int64, device="cuda")[:n_local]
    ctx.gov_build_range(dpart, n, b_lo, b_hi, e_lo, width, *full, rank=rk)
    for got, want in zip(full, (E, vals, sb)):
        np.testing.assert_array_equal(u64(got), want)
    E_look = E.copy()
    E_look[b_hi] = max(int(E_look[b_hi]), e_lo + n_local)
    want_rank = O.lookup_batch(part, n, E_look, vals, width, sb, False)
    np.testing.assert_array_equal(rk.cpu().numpy(), want_rank)
    np.testing.assert_array_equal(np.sort(want_rank), e_lo + np.arange(n_local))
    # the windows
    v0, vw, s0, sw = range_windows(n, width, e_lo, n_local)
    sentinel = 0x5A5A5A5A5A5A5A5A
    bufs, wins = [], []
    for words in (b_hi - b_lo + 1, vw, sw):
        buf = torch.full((guard + words + guard,), sentinel, dtype=torch.int64, device="cuda")
        buf[guard: guard + words] = 0
        bufs.append(buf)
        wins.append(buf[guard: guard + words])
    rkw = torch.zeros(max(n_local, 1), dtype=torch.int64, device="cuda")[:n_local]
    ctx.gov_build_window(dpart, n, b_lo, b_hi, e_lo, width, wins[0], wins[1], v0, wins[2], s0, rank=rkw)
    torch.cuda.synchronize()
    for buf, win, whole, first in zip(bufs, wins, (E, vals, sb), (b_lo, v0, s0)):
        assert torch.all(buf[:guard] == sentinel) and torch.all(buf[-guard:] == sentinel)
        np.testing.assert_array_equal(u64(win), whole[first: first + win.numel()])
        assert np.count_nonzero(whole) == int(torch.count_nonzero(win))   # (the windows hold every word the range wrote)
    np.testing.assert_array_equal(np.sort(rkw.cpu().numpy()), e_lo + np.arange(n_local))
    assert torch.equal(rkw, rk)


# ---- 4. duplicates among ties --------------------------------------------------------------------------------------

def check_pairs(rep, want, n):
    assert rep["found"] == len(want) and rep["keys"] == n and rep["kinds"] is None
    assert not rep["partial"] and not rep["list_full"]
    assert rep["pairs"].tolist() == want


@pytest.mark.parametrize("name,bucket", [("ties8_4400", 1), ("tied_mid_2000", 0)])
def test_duplicates_among_ties(ctx, name, bucket):
    """A tie in sig0 is no duplicate; planted ones (inside a tie group, across groups, a run of 3) are refused
    by the build and listed exactly by the finder."""
    _, _, sig = P.case(name)
    dsig = dev(sig)
    check_pairs(ctx.find_duplicates_sig(dsig), [], len(sig))
    ctx.gov_build(dsig, 0)                                # no BSDB_EDUP
    dup, plants = P.plant_in_bucket(sig, bucket, 7)
    want = P.expected_pairs(dup)
    assert len(want) == 4 and len(plants) == 4
    ddup = dev(dup)
    with pytest.raises(BsdbError, match="EDUP") as e:
        ctx.gov_build(ddup, 0)
    assert e.value.code == EDUP
    check_pairs(ctx.find_duplicates_sig(ddup), want, len(sig))


# ---- 5. the duplicate finder's chunk limit -------------------------------------------------------------------------

def planted_big(name):
    """Duplicates among the keys of the big bucket, and one pair in the last bucket."""
    counts, _, sig = P.case(name)
    dup, _ = P.plant_in_bucket(sig, 0, 11)
    last = np.flatnonzero(P.buckets_int(sig, len(counts)) == len(counts) - 1)
    dup[last[5]] = dup[last[70]]
    return dup, sorted([int(last[5]), int(last[70])])


def test_finder_on_the_chunk_limit(ctx):
    """A bucket of exactly GB_CMAX keys is sorted whole: the exact list, not partial."""
    dup, last_pair = planted_big("big_limit")
    want = P.expected_pairs(dup)
    assert len(want) == 5 and last_pair in want
    check_pairs(ctx.find_duplicates_sig(dev(dup)), want, len(dup))


def test_finder_over_the_chunk_limit(ctx):
    """GB_CMAX + 1 keys: two chunks, of GB_CMAX keys and of one key, each sorted on its own.  The one key belongs to
    at most one run, so at most one pair is lost; what is reported are true pairs, and the report says partial.
    The other buckets are not cut: the last bucket's pair is reported as it is."""
    dup, last_pair = planted_big("over_limit")
    want = P.expected_pairs(dup)
    assert len(want) == 5
    rep = ctx.find_duplicates_sig(dev(dup))
    assert rep["partial"] and not rep["list_full"] and rep["keys"] == len(dup)
    got = rep["pairs"].tolist()
    assert len(want) - 1 <= rep["found"] == len(got) <= len(want)
    assert len({tuple(p) for p in got}) == len(got) and last_pair in got
    for a, b in got:
        assert a < b and dup[a].tolist() == dup[b].tolist()
