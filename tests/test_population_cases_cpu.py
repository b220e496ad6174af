"""The table of tests/population_cases.py pinned on the CPU, before any GPU sees it: every set has the
populations, ties and clusters it claims (exact integers), and the oracle builds a bijection over it."""
import numpy as np
import pytest

import oracle as O
import population_cases as P


def by_bucket(sig, m):
    b_of = P.buckets_int(sig, m)
    rows = sig.tolist()
    return [[rows[i] for i in np.flatnonzero(b_of == b)] for b in range(m)]


def check_population(name):
    counts, shapes, sig = P.case(name)
    m, n = len(counts), sum(counts)
    assert sig.shape == (n, 2) and sig.dtype == np.uint64 and n // 1500 + 1 == m == O.num_buckets(n)
    b_of = P.buckets_int(sig, m)
    np.testing.assert_array_equal(O.buckets(sig, m).astype(np.int64), b_of)       # the oracle agrees with the integers
    assert np.bincount(b_of, minlength=m).tolist() == counts
    assert len({tuple(r) for r in sig.tolist()}) == n
    for b, rows in enumerate(by_bucket(sig, m)):
        lo, hi = P.bucket_range(b, m)
        s0, s1 = [r[0] for r in rows], {r[1] for r in rows}
        assert all(lo <= x <= hi for x in s0)
        if b:
            assert P.bucket_int(lo - 1, m) == b - 1 and P.bucket_int(lo, m) == b
        assert set(P.SIG1_EDGES[: len(rows)]) <= s1
        if len(rows) >= 2 and shapes[b] not in ("span0", "pow2"):
            assert lo in s0 and hi in s0
    return counts, shapes, sig


@pytest.mark.parametrize("name", sorted(P.CASES))
def test_case(name):
    counts, shapes, sig = check_population(name)
    m, n = len(counts), sum(counts)
    rc, E, values, sigbits = O.gov_build(sig, 5)
    assert rc == 0
    assert int(E[0]) & P.OFFSET_MASK == 0
    np.testing.assert_array_equal(E[1:] & np.uint64(P.OFFSET_MASK), np.cumsum(counts))
    for check in (False, True):
        got = O.lookup_batch(sig, n, E, values, 5, sigbits, check)
        np.testing.assert_array_equal(np.sort(got), np.arange(n))
    for b, rows in enumerate(by_bucket(sig, m)):
        s0 = [r[0] for r in rows]
        if len(s0) < 2:
            continue
        mn, shift = P.sort_shift(s0)
        bins = [(x - mn) >> shift for x in s0]
        assert max(bins) < 2048
        if shapes[b] in P.TIE_SHAPES:
            assert len(set(s0)) < len(s0)                       # a pair shares sig0: sig_less's second clause decides
            first = next(r[0] for r in rows if r[1] == 0)       # the group that took SIG1_EDGES
            group = [r[1] for r in rows if r[0] == first]
            assert {0, 2**63 - 1, 2**63} <= set(group)          # unsigned and signed order of sig1 differ in a tie
        else:
            assert len(set(s0)) == len(s0)
        if shapes[b] == "span0":
            assert len(set(s0)) == 1 and shift == 0 and set(bins) == {0}
        if shapes[b] in ("onebin", "onebin_desc"):
            inner = sorted(bins)[1:-1]
            assert len(set(inner)) == 1 and bins.count(inner[0]) == len(s0) - 2 and shift > 0
        if shapes[b] == "pow2":
            span = max(s0) - mn
            assert span == (1 << 40) - 1 + (b & 1) and shift == 29 + (b & 1) and max(bins) == (2047 if b % 2 == 0 else 1024)


def test_onebin_desc_is_descending_in_the_input():
    for n in P.SHAPE_NS:
        counts, _, sig = P.case(f"onebin_desc_{n}")
        for rows in by_bucket(sig, len(counts)):
            s0 = [r[0] for r in rows]
            assert s0 == sorted(s0, reverse=True)


def test_every_profile_and_shape_is_in_the_table():
    have = {tuple(c) for c, _, _ in list(P.CASES.values()) + list(P.BIG_CASES.values())}
    for counts in ([1664, 1665, 0, 1, 2700], [2048, 2049, 13, 1500], [12, 1663, 1664], [0, 0, 3000], [1, 1, 2998],
                   [2, 3, 11, 12, 13, 14, 8945], [16384] + [0] * 9 + [100], [16385] + [0] * 9 + [99],
                   [2, 0, 11, 12, 13, 0, 8962], [2000, 501, 500], [5000, 400, 400, 400, 400]):
        assert tuple(counts) in have
    for shape in ("random", "span0", "ties8", "onebin", "onebin_desc", "pow2"):
        for n in (3001, 4400):
            counts, case_shape, _ = P.CASES[f"{shape}_{n}"]
            assert sum(counts) == n and len(counts) == 3 and max(counts) - min(counts) <= 1 and case_shape == shape
    assert P.CASES["tied_mid_2000"][1][0] == P.CASES["tied_big_5000"][1][0] == "ties4"


@pytest.mark.parametrize("name", sorted(P.BIG_CASES))
def test_big_case_population(name):
    """The 16 384 / 16 385-key buckets: population only (the oracle needs 12 s for either)."""
    counts, _, _ = check_population(name)
    assert counts[0] == P.GB_CMAX + (name == "over_limit")


@pytest.mark.parametrize("name,bucket", [("ties8_4400", 1), ("tied_mid_2000", 0), ("big_limit", 0)])
def test_planted_duplicates(name, bucket):
    counts, shapes, sig = P.case(name)
    m = len(counts)
    assert P.expected_pairs(sig) == []
    dup, plants = P.plant_in_bucket(sig, bucket, 7)
    assert np.bincount(P.buckets_int(dup, m), minlength=m).tolist() == counts     # the populations stay
    (a, same), (c, other), (t, t1), (t_, t2) = plants
    assert t == t_ and len({a, same, c, other, t, t1, t2}) == 7
    assert all(P.bucket_int(sig[p, 0], m) == bucket for p in (a, same, c, other, t, t1, t2))
    if shapes[bucket] in P.TIE_SHAPES:
        assert sig[a, 0] == sig[same, 0]                    # inside a tie group
    assert sig[c, 0] != sig[other, 0]                       # across groups
    want = P.expected_pairs(dup)
    assert want == sorted([sorted([a, same]), sorted([c, other])] + [[min(t, t1, t2), x] for x in sorted((t, t1, t2))[1:]])
    if name != "big_limit":
        assert O.gov_build(dup, 0)[0] != 0                  # the oracle refuses the set
