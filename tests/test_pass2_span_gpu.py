"""Spans of the two-pass histogram: several pass-1 launches (each into a region
set of its own), then one pass 2 over all of them.  The launch length is
set_chunk_keys, the launches per span at most BSDB_SPAN_MAX (read when a
context opens; unset = the library's own limit).  BSDB_D13_GRID=2 makes a
workgroup run several tiles of a launch and carry remainders.
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
LAUNCH = 3 * TILE
# five whole launches and a ragged sixth with a bounds-checked tail
N_MANY = 2 * 7 * TILE + TILE + 777
# one owner lane; a small shift; P = 269; P = 288 (test_pass1_requests_gpu.py)
BUCKETS = [1, 667, 8_795_859, 9_437_184]
M_C4 = 8_795_859
# k_pass1_vare holds 144 bins: the largest m that still runs it, and M_C4
# (the one-tile-per-workgroup kernel)
M_VARE = 144 * 32768
UNLIMITED = None


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
    """A context per span limit (1, 2, ... or UNLIMITED), opened on first use."""
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
    k = O.gen_keys13(4242, (n * L + 12) // 13)[: n * L]
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
    rng = np.random.default_rng(31)
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
def counts_many(get, m, span_max):
    ctx = get(span_max)
    before = ctx.fallback_count()
    with launches_of(ctx, LAUNCH):
        c = u32(ctx.histogram_fixed(exact(keys_of(N_MANY, 13)), 13, m))
    # random distinct keys never take the fallback (its recount would hide a
    # corrupted reservation)
    assert ctx.fallback_count() == before
    return c


@pytest.mark.parametrize("span_max", [1, 2, UNLIMITED])
@pytest.mark.parametrize("m", BUCKETS)
def test_spans_of_several_launches(ctx_of, m, span_max):
    np.testing.assert_array_equal(counts_many(ctx_of, m, span_max), expect(N_MANY, 13, m))


@pytest.mark.parametrize("m", BUCKETS)
def test_span_limits_give_identical_counts(ctx_of, m):
    one = counts_many(ctx_of, m, 1)
    np.testing.assert_array_equal(counts_many(ctx_of, m, 2), one)
    np.testing.assert_array_equal(counts_many(ctx_of, m, UNLIMITED), one)


@pytest.mark.parametrize("span_max,spans", [(1, 6), (2, 3), (UNLIMITED, 1)])
def test_pass2_runs_once_per_span(ctx_of, span_max, spans):
    """The context's live profile: six pass-1 brackets, one pass-2 bracket per span."""
    ctx = ctx_of(span_max)
    keys = exact(keys_of(N_MANY, 13))
    ctx.profile_read(ctx.PASS1), ctx.profile_read(ctx.PASS2)
    with launches_of(ctx, LAUNCH):
        ctx.set_profiling(True)
        try:
            ctx.histogram_fixed(keys, 13, M_C4)
        finally:
            ctx.set_profiling(False)
    _, p1_launches, p1_keys = ctx.profile_read(ctx.PASS1)
    _, p2_launches, _ = ctx.profile_read(ctx.PASS2)
    assert (p1_launches, p1_keys, p2_launches) == (6, N_MANY, spans)


@pytest.mark.parametrize("m", BUCKETS)
def test_flat_cursor_atomic_in_spans(m):
    """BSDB_D13_VARIANT=0: the 13-byte kernel with its cursor atomic as a flat
    atomic (the default is the buffer atomic), every launch with cursors of
    its own."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from bsdb_amd import Context
    with env("BSDB_D13_VARIANT", 0), env("BSDB_SPAN_MAX", None):
        ctx = Context(0)
    try:
        before = ctx.fallback_count()
        with launches_of(ctx, LAUNCH):
            c = u32(ctx.histogram_fixed(exact(keys_of(N_MANY, 13)), 13, m))
        np.testing.assert_array_equal(c, expect(N_MANY, 13, m))
        assert ctx.fallback_count() == before
    finally:
        ctx.close()


@pytest.mark.parametrize("L", [8, 16])
def test_other_fixed_lengths(ctx_of, L):
    ctx = ctx_of(UNLIMITED)
    before = ctx.fallback_count()
    with launches_of(ctx, LAUNCH):
        c = u32(ctx.histogram_fixed(exact(keys_of(N_MANY, L)), L, M_C4))
    np.testing.assert_array_equal(c, expect(N_MANY, L, M_C4))
    assert ctx.fallback_count() == before


@pytest.mark.parametrize("m", [M_VARE, M_C4])
def test_variable_length(ctx_of, m):
    ctx = ctx_of(UNLIMITED)
    blob, off = var_set(N_MANY)
    before = ctx.fallback_count()
    with launches_of(ctx, LAUNCH):
        c = u32(ctx.histogram_var(exact(blob), exact(off.view(np.int64)), m))
    np.testing.assert_array_equal(c, expect_var(N_MANY, m))
    assert ctx.fallback_count() == before


# five launches under a limit of two: spans of 2, 2 and 1 launches; the last
# launch ragged (a tail), or whole (n a multiple of the launch length)
@pytest.mark.parametrize("n", [4 * LAUNCH + TILE + 777, 5 * LAUNCH])
def test_span_ends_inside_the_call(ctx_of, n):
    ctx = ctx_of(2)
    before = ctx.fallback_count()
    with launches_of(ctx, LAUNCH):
        c = u32(ctx.histogram_fixed(exact(keys_of(n, 13)), 13, M_C4))
    np.testing.assert_array_equal(c, expect(n, 13, M_C4))
    assert ctx.fallback_count() == before


def test_accumulates_over_calls(ctx_of):
    ctx = ctx_of(UNLIMITED)
    keys = exact(keys_of(N_MANY, 13))
    before = ctx.fallback_count()
    with launches_of(ctx, LAUNCH):
        c = ctx.histogram_fixed(keys, 13, M_C4)
        c = ctx.histogram_fixed(keys, 13, M_C4, counts=c)
    np.testing.assert_array_equal(u32(c), 2 * expect(N_MANY, 13, M_C4))
    assert ctx.fallback_count() == before


# a launch's windows read past its end into the next launch's keys, never past
# the blob: launches of one tile, the buffer ending at the last key's byte
@pytest.mark.parametrize("L", [13, 8, 16])
@pytest.mark.parametrize("n", [4 * TILE, 4 * TILE + TILE - 1])
def test_buffer_ends_at_last_key(ctx_of, n, L):
    ctx = ctx_of(UNLIMITED)
    before = ctx.fallback_count()
    with launches_of(ctx, TILE):
        c = u32(ctx.histogram_fixed(exact(keys_of(n, L)), L, M_C4))
    np.testing.assert_array_equal(c, expect(n, L, M_C4))
    assert ctx.fallback_count() == before


def test_overflow_recounts_the_whole_span(ctx_of):
    """Every key identical: one bin overflows its regions in every launch.
    Pass 2 skips the span and the fallback recounts all of it, once."""
    ctx = ctx_of(UNLIMITED)
    n = 6 * LAUNCH
    keys = np.tile(keys_of(1, 13), n)
    before = ctx.fallback_count()
    with launches_of(ctx, LAUNCH):
        c = u32(ctx.histogram_fixed(exact(keys), 13, M_C4))
    np.testing.assert_array_equal(c, O.histogram_fixed(keys, 13, M_C4))
    assert int(c.sum()) == n
    assert ctx.fallback_count() > before
