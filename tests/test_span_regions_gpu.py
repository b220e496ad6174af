"""One region set per span of the two-pass histogram: every pass-1 launch of a
span appends to the same id regions and cursors (sized for the span), and one
pass 2 reads them.  The launch length is set_chunk_keys and no longer bounds
the launches of a span: a one-tile launch length gives 15 whole launches and a
bounds-checked tail in ONE span (BSDB_SPAN_MAX unset).  BSDB_D13_GRID=2 makes
a workgroup run several tiles of a launch and carry remainders; launches of
fewer tiles than region copies fill the low copies only, which the region
capacity has to allow for.
Integer work: every comparison is bit-exact against the CPU oracle."""
import contextlib
import functools
import os

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TILE = 16384
LAUNCHES = [TILE, 3 * TILE]
# 15 whole tiles and a ragged rest for the bounds-checked tail kernel
N = 15 * TILE + 777
# one owner lane; a small shift; P = 269; P = 288 (test_pass1_requests_gpu.py)
BUCKETS = [1, 667, 8_795_859, 9_437_184]
M_C4 = 8_795_859
# k_pass1_vare holds 144 bins: the largest m that still runs it, and M_C4
# (the one-tile-per-workgroup kernel)
M_VARE = 144 * 32768
UNLIMITED = None
SPAN_LIMITS = [1, 2, UNLIMITED]


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
    """A context per span limit (1, 2 or UNLIMITED), opened on first use."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from bsdb_amd import Context
    open_ctx = {}

    def get(span_max):
        if span_max not in open_ctx:
            with env("BSDB_SPAN_MAX", span_max):
                open_ctx[span_max] = Context(0)
        return open_ctx[span_max]

    yield get
    for c in open_ctx.values():
        c.close()


@contextlib.contextmanager
def launches_of(ctx, keys, grid=2):
    ctx.set_chunk_keys(keys)
    try:
        with env("BSDB_D13_GRID", grid):
            yield
    finally:
        ctx.set_chunk_keys(0)


@functools.lru_cache(maxsize=None)
def keys_of(n, L):
    """n random distinct keys of L bytes (the 13-byte recipe's byte stream, cut
    every L bytes)."""
    k = O.gen_keys13(977, (n * L + 12) // 13)[: n * L]
    k.setflags(write=False)
    return k


@functools.lru_cache(maxsize=None)
def expect(n, L, m):
    c = O.histogram_fixed(keys_of(n, L), L, m)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def var_set(n):
    """n keys of 8..29 bytes, the last 50 of 0..255: (blob, offsets)."""
    rng = np.random.default_rng(47)
    lens = rng.integers(8, 30, n)
    lens[-50:] = rng.integers(0, 256, 50)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    blob = rng.integers(0, 256, int(off[-1]), dtype=np.uint8)
    return blob, off


@functools.lru_cache(maxsize=None)
def expect_var(n, m):
    blob, off = var_set(n)
    return O.histogram_var(blob, off, m)


def exact(a):
    """The array in a device buffer that ends exactly at its last byte."""
    t = torch.from_numpy(np.array(a)).cuda()
    assert t.numel() == a.size
    return t


def u32(t):
    return t.cpu().numpy().view(np.uint32)


@functools.lru_cache(maxsize=None)
def counts13(get, m, span_max, launch):
    ctx = get(span_max)
    before = ctx.fallback_count()
    with launches_of(ctx, launch):
        c = u32(ctx.histogram_fixed(exact(keys_of(N, 13)), 13, m))
    # random distinct keys never take the fallback (its recount would hide a
    # corrupted reservation or a region sized too small)
    assert ctx.fallback_count() == before
    return c


@pytest.mark.parametrize("launch", LAUNCHES)
@pytest.mark.parametrize("span_max", SPAN_LIMITS)
@pytest.mark.parametrize("m", BUCKETS)
def test_launches_append_to_one_region_set(ctx_of, m, span_max, launch):
    np.testing.assert_array_equal(counts13(ctx_of, m, span_max, launch), expect(N, 13, m))


@pytest.mark.parametrize("m", BUCKETS)
def test_span_limits_and_launch_lengths_agree(ctx_of, m):
    one = counts13(ctx_of, m, 1, TILE)
    for span_max in SPAN_LIMITS:
        for launch in LAUNCHES:
            np.testing.assert_array_equal(counts13(ctx_of, m, span_max, launch), one)


@pytest.mark.parametrize("span_max,spans", [(1, 16), (2, 8), (UNLIMITED, 1)])
def test_sixteen_launches_in_one_span(ctx_of, span_max, spans):
    """The context's live profile at a one-tile launch length: 15 whole
    launches and the tail's, one pass-2 bracket per span -- with no limit set,
    one span, past the eight launches a span once held."""
    ctx = ctx_of(span_max)
    keys = exact(keys_of(N, 13))
    ctx.profile_read(ctx.PASS1), ctx.profile_read(ctx.PASS2)
    with launches_of(ctx, TILE):
        ctx.set_profiling(True)
        try:
            ctx.histogram_fixed(keys, 13, M_C4)
        finally:
            ctx.set_profiling(False)
    _, p1_launches, p1_keys = ctx.profile_read(ctx.PASS1)
    _, p2_launches, _ = ctx.profile_read(ctx.PASS2)
    assert (p1_launches, p1_keys, p2_launches) == (16, N, spans)


@pytest.mark.parametrize("launch", LAUNCHES)
def test_accumulates_over_calls(ctx_of, launch):
    ctx = ctx_of(UNLIMITED)
    keys = exact(keys_of(N, 13))
    before = ctx.fallback_count()
    with launches_of(ctx, launch):
        c = ctx.histogram_fixed(keys, 13, M_C4)
        assert int(u32(c).sum()) == N  # (non-zero counts go into the second call)
        c = ctx.histogram_fixed(keys, 13, M_C4, counts=c)
    np.testing.assert_array_equal(u32(c), 2 * expect(N, 13, M_C4))
    assert ctx.fallback_count() == before


@pytest.mark.parametrize("launch", LAUNCHES)
@pytest.mark.parametrize("L", [8, 12, 16])
def test_other_fixed_lengths(ctx_of, L, launch):
    ctx = ctx_of(UNLIMITED)
    before = ctx.fallback_count()
    with launches_of(ctx, launch):
        c = u32(ctx.histogram_fixed(exact(keys_of(N, L)), L, M_C4))
    np.testing.assert_array_equal(c, expect(N, L, M_C4))
    assert ctx.fallback_count() == before


# k_pass1_vare has tiles of 8192 keys: launches of 2 and 6 of them
@pytest.mark.parametrize("launch", LAUNCHES)
@pytest.mark.parametrize("m", [M_VARE, M_C4])
def test_variable_length(ctx_of, m, launch):
    ctx = ctx_of(UNLIMITED)
    blob, off = var_set(N)
    before = ctx.fallback_count()
    with launches_of(ctx, launch):
        c = u32(ctx.histogram_var(exact(blob), exact(off.view(np.int64)), m))
    np.testing.assert_array_equal(c, expect_var(N, m))
    assert ctx.fallback_count() == before


@pytest.mark.parametrize("launch", LAUNCHES)
def test_overflow_recounts_the_span_once(ctx_of, launch):
    """Every key identical: one bin takes everything and overflows.  Pass 2
    skips the span and the fallback recounts all of it, once; the next,
    ordinary call on the same context starts from cleared cursors."""
    ctx = ctx_of(UNLIMITED)
    keys = np.tile(keys_of(1, 13), N)
    before = ctx.fallback_count()
    with launches_of(ctx, launch):
        c = u32(ctx.histogram_fixed(exact(keys), 13, M_C4))
    np.testing.assert_array_equal(c, O.histogram_fixed(keys, 13, M_C4))
    assert int(c.sum()) == N
    assert ctx.fallback_count() == before + 1
    with launches_of(ctx, launch):
        c = u32(ctx.histogram_fixed(exact(keys_of(N, 13)), 13, M_C4))
    np.testing.assert_array_equal(c, expect(N, 13, M_C4))
    assert ctx.fallback_count() == before + 1
