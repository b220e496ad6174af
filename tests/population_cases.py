"""The cases of what lies inside a bucket: populations on the exact limits of the
bucket classes (gov_geometry.hpp: GS_CMAX = 1664, GM_CMAX = 2048, GB_CMAX =
16384), empty, one-key and tiny buckets between full ones (GS_TINY = 12), and
ties and clusters in sig0 (sig_less's second clause, k_bucket_sort's sub-bin
arithmetic, the neighbour duplicate compare).  Random keys give none of them:
every bucket then holds 1500 +- 40 keys and no sig0 repeats.

Not a test module: pure functions over numpy, pinned by
tests/test_population_cases_cpu.py and run on the GPU by
tests/test_population_gpu.py.  Everything starts at signatures (the builds,
lookup, sign and find_duplicates_sig take them directly), so no hash preimage
is needed.

The bucket arithmetic is exact Python integers, as in test_bucket_edges_gpu.py:
bucket = hi64((sig0 >>> 1) * 2m), so bucket b of m starts at
sig0 = 2 ceil(b 2^63 / m) and ends one before bucket b + 1's start (2^64 - 1 for
the last bucket)."""
import numpy as np

U64 = (1 << 64) - 1
OFFSET_MASK = (1 << 56) - 1
GS_TINY, GS_CMAX, GM_CMAX, GB_CMAX = 12, 1664, 2048, 16384     # gov_kernels.hip, gov_geometry.hpp
NBIN_BITS = 11                                                 # k_bucket_sort: 2 048 sub-bins
# unsigned against signed order of sig1: every bucket of 7 or more keys holds all of these
SIG1_EDGES = (0, 1, 2**63 - 1, 2**63, 2**63 + 1, 2**64 - 2, 2**64 - 1)
TIE_SHAPES = ("span0", "ties8", "ties4")
SHAPES = ("random", "span0", "ties8", "onebin", "onebin_desc", "pow2")


# ---- buckets in exact integers -------------------------------------------------------------------------------------

def bucket_int(sig0, m):
    """multiplyHigh(sig0 >>> 1, 2m)."""
    return ((int(sig0) >> 1) * (2 * m)) >> 64


def buckets_int(sig, m):
    return np.array([bucket_int(s, m) for s in sig[:, 0].tolist()], np.int64)


def bucket_start(b, m):
    return 2 * -((-b << 63) // m)            # 2 ceil(b 2^63 / m)


def bucket_range(b, m):
    """[first, last] sig0 of bucket b of m."""
    return bucket_start(b, m), (bucket_start(b + 1, m) - 1 if b + 1 < m else U64)


def sort_shift(sig0s):
    """k_bucket_sort's sub-bin rule for one bucket's sig0: (min, shift) with bits = the bit length of the span
    and shift = max(bits - 11, 0); a key's sub-bin is (sig0 - min) >> shift."""
    mn, mx = min(sig0s), max(sig0s)
    bits = (mx - mn).bit_length()
    return mn, max(bits - NBIN_BITS, 0)


# ---- the signature sets --------------------------------------------------------------------------------------------

def _rand_int(rng, lo, hi):
    """A uniform integer of [lo, hi], any width."""
    span = hi - lo + 1
    r = int.from_bytes(rng.bytes(12), "little")          # 96 bits: the bias is below 2^-32
    return lo + r % span


def _distinct(rng, lo, hi, k, taken=()):
    """k distinct integers of [lo, hi], none of them in `taken`, in the order drawn."""
    assert hi - lo + 1 >= k + len(taken)
    seen, out = set(taken), []
    while len(out) < k:
        x = _rand_int(rng, lo, hi)
        if x not in seen:
            seen.add(x)
            out.append(x)
    return out


def _sig0_of_bucket(rng, shape, b, m, c):
    """The c values of sig0 of bucket b, in the order they take in the bucket's list (before any shuffle)."""
    lo, hi = bucket_range(b, m)
    if c == 0:
        return []
    if c == 1:
        return [_rand_int(rng, lo, hi)]
    if shape == "random":                    # both ends of the bucket's range, distinct values between them
        return [lo, hi] + _distinct(rng, lo + 1, hi - 1, c - 2)
    if shape == "span0":                     # one value: the sort's span is 0
        return [_rand_int(rng, lo, hi)] * c
    if shape.startswith("ties"):             # groups of k share a value; the first two groups sit on the range's ends
        k = int(shape[4:])
        groups = -(-c // k)
        vals = ([lo, hi] + _distinct(rng, lo + 1, hi - 1, groups - 2))[:groups]
        return [vals[i // k] for i in range(c)]
    if shape in ("onebin", "onebin_desc"):   # the range's ends, the rest 7 apart from its middle: one sub-bin
        mid = (lo + hi) // 2
        vals = [lo, hi] + [mid + 7 * i for i in range(c - 2)]
        assert mid + 7 * c < hi
        return sorted(vals, reverse=True) if shape == "onebin_desc" else vals
    if shape == "pow2":                      # the sort's span on a power of two: 2^40 - 1 (even b), 2^40 (odd b)
        span = (1 << 40) - 1 + (b & 1)
        first = _rand_int(rng, lo, hi - span)
        return [first, first + span] + _distinct(rng, first + 1, first + span - 1, c - 2)
    raise ValueError(shape)


def populate(counts, shape, seed):
    """A signature set (uint64 [n, 2]) with exactly counts[b] signatures in bucket b of m = len(counts).

    sig0 lies inside each bucket as `shape` says -- one name for every bucket, or a list of one name a bucket:
      random       both ends of the bucket's sig0 range, distinct values between them
      span0        every sig0 of the bucket equal
      ties8/ties4  groups of 8 / 4 share a sig0; the range's two ends are among the groups' values
      onebin       the range's two ends, the rest at mid + 7 i: all but two keys in one sub-bin of k_bucket_sort
      onebin_desc  the same, a bucket's keys in descending order of sig0 in the input
      pow2         the bucket's sig0 span is exactly 2^40 - 1 (even buckets) or 2^40 (odd ones)
    (span0 and pow2 fix the span, so only the other shapes hold both ends of the bucket's range; a one-key
    bucket holds one value of its range.)  sig1: the first seven keys of a bucket's list -- for the tie shapes
    they share a sig0 -- take SIG1_EDGES, the rest random values.  The buckets are interleaved at random and,
    but for onebin_desc, each bucket's keys are shuffled.  All signatures are distinct."""
    m, n = len(counts), int(sum(counts))
    assert n // 1500 + 1 == m, (n, m)
    shapes = [shape] * m if isinstance(shape, str) else list(shape)
    assert len(shapes) == m
    rng = np.random.default_rng(seed)
    per_bucket = []
    for b, c in enumerate(counts):
        s0 = _sig0_of_bucket(rng, shapes[b], b, m, c)
        edges = list(SIG1_EDGES[: min(c, len(SIG1_EDGES))])
        s1 = edges + _distinct(rng, 0, U64, c - len(edges), edges)
        rows = list(zip(s0, s1))
        if shapes[b] != "onebin_desc":
            rows = [rows[i] for i in rng.permutation(c)]
        per_bucket.append(rows)
    owner = np.repeat(np.arange(m), counts)
    rng.shuffle(owner)
    nxt, rows = [0] * m, []
    for b in owner.tolist():
        rows.append(per_bucket[b][nxt[b]])
        nxt[b] += 1
    assert len(set(rows)) == n
    return np.array(rows, dtype=np.uint64).reshape(n, 2)


# ---- the table -----------------------------------------------------------------------------------------------------

def even(n, m=3):
    """n keys spread evenly over m buckets."""
    return [n // m + (b < n % m) for b in range(m)]


# populations on the class limits, and empty, one-key and tiny buckets between full ones (random shape)
PROFILES = {
    "small_limit": [GS_CMAX, GS_CMAX + 1, 0, 1, 2700],
    "mid_limit": [GM_CMAX, GM_CMAX + 1, GS_TINY + 1, 1500],
    "tiny_small_limit": [GS_TINY, GS_CMAX - 1, GS_CMAX],
    "empty_first": [0, 0, 3000],
    "one_key_first": [1, 1, 2998],
    "tiny_ladder": [2, 3, 11, 12, 13, 14, 8945],
}
# the global-slab solver's limit: built (and refused) on the device only -- the oracle needs 12 s for either
BIG_PROFILES = {
    "big_limit": [GB_CMAX] + [0] * 9 + [100],
    "over_limit": [GB_CMAX + 1] + [0] * 9 + [99],
}
# tiny_ladder with two more empty buckets: [1, 6) is an interior range whose first and last buckets are empty
RANGE_PROFILE = [2, 0, 11, 12, 13, 0, 8962]
SHAPE_NS = (3001, 4400)

CASES = {name: (counts, "random", 100 + i) for i, (name, counts) in enumerate(PROFILES.items())}
CASES.update({f"{shape}_{n}": (even(n), shape, 200 + 10 * i + j)
              for i, shape in enumerate(SHAPES) if shape != "random" for j, n in enumerate(SHAPE_NS)})
CASES.update({f"random_{n}": (even(n), "random", 300 + j) for j, n in enumerate(SHAPE_NS)})
# an oversized bucket (k_bucket_sort_big's bitonic sort) with groups of 4 sharing sig0, the others random
CASES["tied_mid_2000"] = ([2000, 501, 500], ["ties4", "random", "random"], 400)
CASES["tied_big_5000"] = ([5000, 400, 400, 400, 400], ["ties4"] + ["random"] * 4, 401)
CASES["range_profile"] = (RANGE_PROFILE, "random", 402)
BIG_CASES = {name: (counts, "random", 500 + i) for i, (name, counts) in enumerate(BIG_PROFILES.items())}

_memo = {}


def case(name):
    """(counts, shapes a bucket, the signature set) of a case of CASES or BIG_CASES; the set is made once."""
    if name not in _memo:
        counts, shape, seed = (CASES.get(name) or BIG_CASES[name])
        sig = populate(counts, shape, seed)
        sig.setflags(write=False)
        _memo[name] = (list(counts), [shape] * len(counts) if isinstance(shape, str) else list(shape), sig)
    return _memo[name]


# ---- duplicates ----------------------------------------------------------------------------------------------------

def plant_in_bucket(sig, bucket, seed):
    """A copy of `sig` with duplicates planted among the keys of `bucket` (counts stay as they are): one
    signature copied over another of the same sig0 where the bucket has a tie (else over any other), one over a
    key of another sig0, and one over two more keys (a run of 3).  Returns (the copy, the [src, dst] lists)."""
    m = len(sig) // 1500 + 1
    rng = np.random.default_rng(seed)
    pos = [i for i, s in enumerate(sig[:, 0].tolist()) if bucket_int(s, m) == bucket]
    pos = [pos[i] for i in rng.permutation(len(pos))]
    assert len(pos) >= 8
    s0 = sig[:, 0].tolist()
    a = pos[0]
    same = next((p for p in pos[1:] if s0[p] == s0[a]), pos[1])
    rest = [p for p in pos[1:] if p != same]
    other = next((p for p in rest if s0[p] != s0[a]), rest[0])
    rest = [p for p in rest if p != other]
    plants = [[a, same], [rest[0], other], [rest[1], rest[2]], [rest[1], rest[3]]]
    out = np.array(sig)
    for src, dst in plants:
        out[dst] = sig[src]
    return out, plants


def expected_pairs(sig):
    """The finder's list by a dict grouping: a run of r equal signatures is r - 1 pairs (smallest position,
    other), the rows sorted."""
    groups = {}
    for i, s in enumerate(map(tuple, sig.tolist())):
        groups.setdefault(s, []).append(i)
    return sorted([g[0], x] for g in groups.values() for x in g[1:])
