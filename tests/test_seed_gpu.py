"""A non-zero store seed through every histogram and hash kernel.  The reference
reseeds its store when it meets duplicates (CBHS), and pass1_kernel() picks a
different kernel instantiation when seed != 0: k_pass1_d13e<*, false, *> (lengths
8, 12, 16, and 13 in both cursor variants), k_pass1_vare<*, false>, the sort
kernel, the one-tile kernels, the fallback, the pipelined path and the
single-pass kernel all take the seed from their arguments.  Every case states
on the host that its expected result differs from the seed-0 result (a kernel
that ignored the seed fails), and every case not meant to overflow checks that
the fallback counter did not move (a recount with direct atomics would hide a
wrong pass 1).  Integer work: every comparison is bit-exact against the oracle."""
import contextlib
import functools
import os

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

THREADS = O.cpu_threads()
ROUND = 256 * 16384  # keys of one super-tile round of the single-pass kernel
TILE = 16384         # D13E_TILE (VARE_TILE is 8192)
# the persistent kernel runs whole tiles, the bounds-checked kernel the tail
N = 3 * TILE + 777
S_MIXED, S_TOP, S_LOW32, S_ONES = 0x0123456789ABCDEF, 1 << 63, 0x00000000FFFFFFFF, 2**64 - 1
# S_LOW32: seed + 8 L carries out of the low word in the W64 pair arithmetic
SEEDS = [S_MIXED, S_TOP, S_LOW32, S_ONES]
M_SMALL, M_C4 = 667, 8_795_859
M_SORT = 9_437_185          # just past k_pass1_d13e's 288 bins: the sort kernel
M_VARE = [5_000, 144 * 32768]  # a small shift; k_pass1_vare's 144-bin limit


def cross(ms):
    """Two bucket counts x two seeds, and the other seeds with the second one."""
    a, b = ms
    return [(a, S_MIXED), (a, S_TOP), (b, S_MIXED), (b, S_TOP), (b, S_LOW32), (b, S_ONES)]


@contextlib.contextmanager
def env(name, value):
    old = os.environ.get(name)
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = str(value)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = old


@pytest.fixture(scope="module")
def ctx_of():
    """A context per BSDB_D13_VARIANT (None: the default), opened on first use."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from bsdb_amd import Context
    open_ctx = {}

    def get(variant=None):
        if variant not in open_ctx:
            with env("BSDB_D13_VARIANT", variant):
                open_ctx[variant] = Context(0)
        return open_ctx[variant]

    yield get
    for c in open_ctx.values():
        c.close()


@pytest.fixture(scope="module")
def ctx(ctx_of):
    return ctx_of(None)


@functools.lru_cache(maxsize=None)
def keys_of(n, L):
    """n random distinct keys of L bytes (the 13-byte recipe's byte stream, cut
    every L bytes; L = 1: 256 distinct keys)."""
    k = O.gen_keys13_mt(5151, (n * L + 12) // 13, THREADS)[: n * L]
    k.setflags(write=False)
    return k


@functools.lru_cache(maxsize=None)
def expect(n, L, m, seed):
    c = O.histogram_fixed_mt(keys_of(n, L), L, m, THREADS, seed)[0]
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def c5_set(n):
    blob, off = O.gen_keys_var(7, n)
    return blob, off


@functools.lru_cache(maxsize=None)
def ragged_set():
    """Keys of 0..255 bytes: empty keys at the start and across a tile boundary,
    2.5-4 KiB groups, groups over the 4352-byte stage (the recipe of
    test_var_binned_ragged_groups).  Fewer empty keys than there: they are one
    key repeated, and at k_pass1_vare's 144 bins a bin holds 128 ids for a mean
    fill of 57 +- 7.5 a tile; 32 copies in a tile leave it 5 sigma of room, so
    the fallback counter can be held still."""
    rng = np.random.default_rng(23)
    n = 3 * 8192 + 777
    lens = rng.integers(8, 30, n)
    lens[0:24] = 0
    lens[8192 - 8:8192 + 8] = 0
    lens[9000:9640] = rng.integers(40, 65, 640)
    lens[12000:12700] = rng.integers(70, 256, 700)
    lens[20000:20064] = 64
    lens[-50:] = rng.integers(0, 256, 50)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    return rng.integers(0, 256, int(off[-1]), dtype=np.uint8), off


VAR_SETS = {"c5": lambda: c5_set(N), "ragged": ragged_set}


@functools.lru_cache(maxsize=None)
def expect_var(name, m, seed):
    blob, off = VAR_SETS[name]()
    return O.histogram_var(blob, off, m, seed)


def exact(a):
    """The array in a device buffer that ends exactly at its last byte."""
    t = torch.from_numpy(np.array(a)).cuda()
    assert t.numel() == a.size
    return t


def dev_var(name):
    blob, off = VAR_SETS[name]()
    return exact(blob), exact(off.view(np.int64))


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def seeded(want, want0):
    """The expected result differs from the seed-0 result, so a kernel that
    ignored the seed fails the comparison that follows."""
    assert want.shape == want0.shape and not np.array_equal(want, want0)


def check_counts(ctx, run, want, want0, overflows=False):
    seeded(want, want0)
    before = ctx.fallback_count()
    got = u32(run())
    np.testing.assert_array_equal(got, want)
    if not overflows:
        assert ctx.fallback_count() == before
    return got


# ---- the persistent windowed kernel k_pass1_d13e and the sort kernel ----------

@pytest.mark.parametrize("m,seed", cross([M_SMALL, M_C4]))
@pytest.mark.parametrize("L", [8, 12, 13, 16])
def test_windowed_kernel(ctx, L, m, seed):
    keys = exact(keys_of(N, L))
    check_counts(ctx, lambda: ctx.histogram_fixed(keys, L, m, seed=seed), expect(N, L, m, seed), expect(N, L, m, 0))


@pytest.mark.parametrize("m,seed", cross([M_SMALL, M_C4]))
@pytest.mark.parametrize("variant", [0, 2])
def test_13_byte_cursor_variants(ctx_of, variant, m, seed):
    """BSDB_D13_VARIANT=0: k_pass1_d13e<0> (flat cursor atomic); =2: k_pass1_d13."""
    c = ctx_of(variant)
    keys = exact(keys_of(N, 13))
    check_counts(c, lambda: c.histogram_fixed(keys, 13, m, seed=seed), expect(N, 13, m, seed), expect(N, 13, m, 0))


@pytest.mark.parametrize("seed", SEEDS)
def test_sort_kernel_past_the_bins(ctx, seed):
    keys = exact(keys_of(N, 13))
    check_counts(ctx, lambda: ctx.histogram_fixed(keys, 13, M_SORT, seed=seed), expect(N, 13, M_SORT, seed),
                 expect(N, 13, M_SORT, 0))


# ---- k_pass1_vare ---------------------------------------------------------------

@pytest.mark.parametrize("m,seed", cross(M_VARE))
@pytest.mark.parametrize("L", [1, 5, 20, 32])
def test_vare_fixed_lengths(ctx, L, m, seed):
    # L = 1: 256 distinct keys, ~195 copies of each, up to 8 of them in one LDS
    # bin: a bin may overflow by right, so there the counter is not held still
    keys = exact(keys_of(N, L))
    check_counts(ctx, lambda: ctx.histogram_fixed(keys, L, m, seed=seed), expect(N, L, m, seed), expect(N, L, m, 0),
                 overflows=L == 1)


@pytest.mark.parametrize("m,seed", cross(M_VARE))
@pytest.mark.parametrize("name", ["c5", "ragged"])
def test_vare_variable_length(ctx, name, m, seed):
    blob, off = dev_var(name)
    check_counts(ctx, lambda: ctx.histogram_var(blob, off, m, seed=seed), expect_var(name, m, seed),
                 expect_var(name, m, 0))


# ---- the one-tile kernels (set_frontend) and direct atomics (mode 2) ------------

@contextlib.contextmanager
def knobs(ctx, frontend=0, mode=0):
    ctx.set_frontend(frontend)
    ctx.set_histogram_mode(mode)
    try:
        yield
    finally:
        ctx.set_frontend(0)
        ctx.set_histogram_mode(0)


# 13: STAGED13 / DIRECT13; 5, 20, 40: STAGED with 4 / 2 / 1 keys per thread; 80: FIXED_DIRECT
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("L", [13, 5, 20, 40, 80])
@pytest.mark.parametrize("frontend", [1, 2])
def test_one_tile_kernels_fixed(ctx, frontend, L, seed):
    keys = exact(keys_of(N, L))
    with knobs(ctx, frontend):
        check_counts(ctx, lambda: ctx.histogram_fixed(keys, L, M_C4, seed=seed), expect(N, L, M_C4, seed),
                     expect(N, L, M_C4, 0))


# 1: VARSTAGED; 2: VAR
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", ["c5", "ragged"])
@pytest.mark.parametrize("frontend", [1, 2])
def test_one_tile_kernels_variable_length(ctx, frontend, name, seed):
    blob, off = dev_var(name)
    with knobs(ctx, frontend):
        check_counts(ctx, lambda: ctx.histogram_var(blob, off, M_C4, seed=seed), expect_var(name, M_C4, seed),
                     expect_var(name, M_C4, 0))


@pytest.mark.parametrize("m,seed", cross([M_SMALL, M_C4]))
def test_direct_atomics(ctx, m, seed):
    keys = exact(keys_of(N, 13))
    blob, off = dev_var("ragged")
    with knobs(ctx, mode=2):
        check_counts(ctx, lambda: ctx.histogram_fixed(keys, 13, m, seed=seed), expect(N, 13, m, seed),
                     expect(N, 13, m, 0))
        check_counts(ctx, lambda: ctx.histogram_var(blob, off, m, seed=seed), expect_var("ragged", m, seed),
                     expect_var("ragged", m, 0))


# ---- pipelined, single pass, overflow, accumulation ----------------------------

@pytest.mark.parametrize("seed", SEEDS)
def test_pipelined(ctx, seed):
    n = 3_000_017  # ragged: chunk ends mid-tile, the last tile bounds-checked
    keys = exact(keys_of(n, 13))
    ctx.set_pipeline(1, 4, 32)
    try:
        check_counts(ctx, lambda: ctx.histogram_fixed(keys, 13, M_C4, seed=seed), expect(n, 13, M_C4, seed),
                     expect(n, 13, M_C4, 0))
    finally:
        ctx.set_pipeline(-1)


N_FUSED = 4 * ROUND + 12_345  # four rounds of the single-pass kernel and a two-pass tail


@pytest.fixture(scope="module")
def fused_keys():
    return exact(keys_of(N_FUSED, 13))


@pytest.mark.parametrize("seed", SEEDS)
def test_single_pass_with_a_ragged_tail(ctx, fused_keys, seed):
    launches = ctx.fused_status()[0]
    with knobs(ctx, mode=3):
        check_counts(ctx, lambda: ctx.histogram_fixed(fused_keys, 13, M_C4, seed=seed), expect(N_FUSED, 13, M_C4, seed),
                     expect(N_FUSED, 13, M_C4, 0))
    now, timeouts = ctx.fused_status()
    assert now > launches and timeouts == 0


@pytest.mark.parametrize("seed", SEEDS)
def test_overflow_recount(ctx, seed):
    """One key repeated: the regions overflow and k_overflow_fallback recounts with the seed."""
    n, key = 600_000, b"abcdefghijklm"
    keys = exact(np.tile(np.frombuffer(key, np.uint8), n))
    b, b0 = O.bucket(O.spooky_short(key, seed)[0], M_C4), O.bucket(O.spooky_short(key)[0], M_C4)
    assert b != b0
    before = ctx.fallback_count()
    counts = u32(ctx.histogram_fixed(keys, 13, M_C4, seed=seed))
    assert counts[b] == n and int(counts.sum(dtype=np.uint64)) == n
    assert ctx.fallback_count() > before


@pytest.mark.parametrize("seed", SEEDS)
def test_accumulates_over_chunks(ctx, seed):
    keys = exact(keys_of(N, 13))
    want = 2 * expect(N, 13, M_C4, seed)

    def twice():
        ctx.set_chunk_keys(3 * 8192)
        try:
            c = ctx.histogram_fixed(keys, 13, M_C4, seed=seed)
            return ctx.histogram_fixed(keys, 13, M_C4, counts=c, seed=seed)
        finally:
            ctx.set_chunk_keys(0)
    check_counts(ctx, twice, want, 2 * expect(N, 13, M_C4, 0))


# ---- signatures ------------------------------------------------------------------

@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("L", [1, 8, 12, 16, 20, 40, 80, 255])
def test_hash_fixed(ctx, L, seed):
    n = 20_001  # two whole tiles and a partial one
    k = keys_of(n, L)
    want = O.hash_fixed(k, L, seed)
    seeded(want, O.hash_fixed(k, L, 0))
    np.testing.assert_array_equal(u64(ctx.hash_fixed(exact(k), L, seed=seed)), want)


@functools.lru_cache(maxsize=None)
def every_length_set():
    """40 keys of every length 0..255, shuffled: more than one tile."""
    rng = np.random.default_rng(77)
    lens = rng.permutation(np.repeat(np.arange(256), 40))
    off = np.zeros(lens.size + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    return rng.integers(0, 256, int(off[-1]), dtype=np.uint8), off


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("frontend", [0, 2])
def test_hash_var_every_length(ctx, frontend, seed):
    blob, off = every_length_set()
    want = O.hash_var(blob, off, seed)
    seeded(want, O.hash_var(blob, off, 0))
    with knobs(ctx, frontend):
        got = u64(ctx.hash_var(exact(blob), exact(off.view(np.int64)), seed=seed))
    np.testing.assert_array_equal(got, want)


# ---- host forms and the multi-device context ---------------------------------------

@pytest.mark.parametrize("seed", SEEDS)
def test_host_forms(ctx, seed):
    k = keys_of(N, 13)
    blob, off = ragged_set()
    before = ctx.fallback_count()
    seeded(expect(N, 13, M_SMALL, seed), expect(N, 13, M_SMALL, 0))
    np.testing.assert_array_equal(ctx.histogram_fixed_host(k, 13, M_SMALL, seed=seed), expect(N, 13, M_SMALL, seed))
    seeded(expect_var("ragged", M_SMALL, seed), expect_var("ragged", M_SMALL, 0))
    np.testing.assert_array_equal(ctx.histogram_var_host(blob, off, M_SMALL, seed=seed),
                                  expect_var("ragged", M_SMALL, seed))
    assert ctx.fallback_count() == before
    want = O.hash_fixed(k, 13, seed)
    seeded(want, O.hash_fixed(k, 13, 0))
    np.testing.assert_array_equal(ctx.hash_fixed_host(k, 13, seed=seed), want)
    want = O.hash_var(blob, off, seed)
    seeded(want, O.hash_var(blob, off, 0))
    np.testing.assert_array_equal(ctx.hash_var_host(blob, off, seed=seed), want)


@pytest.mark.parametrize("seed", [S_MIXED, S_LOW32])
def test_multi_device_context(seed):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from bsdb_amd.native import Multi
    k = keys_of(N, 13)
    blob, off = c5_set(N)
    m = O.num_buckets(N)
    want, want_var = expect(N, 13, m, seed), expect_var("c5", m, seed)
    seeded(want, expect(N, 13, m, 0))
    seeded(want_var, expect_var("c5", m, 0))
    with Multi(1) as mc:
        np.testing.assert_array_equal(mc.histogram_fixed(k, 13, seed=seed), O.edge_offsets(want))
        np.testing.assert_array_equal(mc.histogram_var(blob, off, seed=seed), O.edge_offsets(want_var))


# ---- BSDB_NO_SEED0: the generic instantiation on seed 0 (the A/B switch of the measurements) ----

@pytest.mark.parametrize("L", [8, 13])
def test_generic_instantiation_on_seed_0(ctx, L):
    keys = exact(keys_of(N, L))
    before = ctx.fallback_count()
    with env("BSDB_NO_SEED0", 1):
        got = u32(ctx.histogram_fixed(keys, L, M_C4))
    np.testing.assert_array_equal(got, expect(N, L, M_C4, 0))
    assert ctx.fallback_count() == before


def test_generic_instantiation_on_seed_0_variable_length(ctx):
    blob, off = dev_var("ragged")
    before = ctx.fallback_count()
    with env("BSDB_NO_SEED0", 1):
        got = u32(ctx.histogram_var(blob, off, M_VARE[0]))
    np.testing.assert_array_equal(got, expect_var("ragged", M_VARE[0], 0))
    assert ctx.fallback_count() == before


def test_generic_instantiation_on_seed_0_single_pass(ctx, fused_keys):
    launches = ctx.fused_status()[0]
    before = ctx.fallback_count()
    with env("BSDB_NO_SEED0", 1), knobs(ctx, mode=3):
        got = u32(ctx.histogram_fixed(fused_keys, 13, M_C4))
    np.testing.assert_array_equal(got, expect(N_FUSED, 13, M_C4, 0))
    now, timeouts = ctx.fused_status()
    assert now > launches and timeouts == 0 and ctx.fallback_count() == before
