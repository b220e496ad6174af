"""Pass 1's memory requests (k_pass1_d13e): the cursor reservation chain, the
remainder carry and the key-window addresses, with one workgroup running many
tiles (BSDB_D13_GRID=2; the parity tests give every workgroup one tile).
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
# two workgroups of seven or eight tiles each, and a ragged tail for the
# bounds-checked kernel
N_MANY = 2 * 7 * TILE + TILE + 777
# one owner lane; a small shift; P = 269 (the last wave owns fewer partitions
# than the others); P = 288 (every owner slot in use)
BUCKETS = [1, 667, 8_795_859, 9_437_184]


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from bsdb_amd import Context
    c = Context(0)
    yield c
    c.close()


@contextlib.contextmanager
def grid_limit(g):
    """BSDB_D13_GRID (read by the library at plan time) for the calls inside."""
    old = os.environ.get("BSDB_D13_GRID")
    os.environ["BSDB_D13_GRID"] = str(g)
    try:
        yield
    finally:
        if old is None:
            del os.environ["BSDB_D13_GRID"]
        else:
            os.environ["BSDB_D13_GRID"] = old


@functools.lru_cache(maxsize=None)
def keys_of(n, L):
    """n random distinct keys of L bytes: the 13-byte recipe's byte stream
    (bytes 0-7 of a 13-byte key are a bijection of its index, the rest random),
    cut every L bytes."""
    k = O.gen_keys13(911, (n * L + 12) // 13)[: n * L]
    k.setflags(write=False)
    return k


@functools.lru_cache(maxsize=None)
def expect(n, L, m):
    c = O.histogram_fixed(keys_of(n, L), L, m)
    c.setflags(write=False)
    return c


def exact(keys):
    """The keys in a device buffer that ends exactly at their last byte."""
    t = torch.from_numpy(np.array(keys)).cuda()
    assert t.numel() == keys.size
    return t


@pytest.mark.parametrize("L", [13, 8, 16])
@pytest.mark.parametrize("m", BUCKETS)
def test_many_tiles_per_workgroup(ctx, m, L):
    keys = exact(keys_of(N_MANY, L))
    before = ctx.fallback_count()
    with grid_limit(2):
        counts = ctx.histogram_fixed(keys, L, m).cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(counts, expect(N_MANY, L, m))
    # a corrupted reservation overflows a region, and the fallback's recount
    # would hide it: random distinct keys never take the fallback
    assert ctx.fallback_count() == before


@pytest.mark.parametrize("L", [13, 8, 16])
@pytest.mark.parametrize("n", [4 * TILE, 4 * TILE + TILE - 1])
def test_buffer_ends_at_last_key(ctx, n, L):
    m = 8_795_859
    keys = exact(keys_of(n, L))
    before = ctx.fallback_count()
    counts = ctx.histogram_fixed(keys, L, m).cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(counts, expect(n, L, m))
    assert ctx.fallback_count() == before


def test_accumulates_over_chunks(ctx):
    m = 8_795_859
    keys = exact(keys_of(N_MANY, 13))
    before = ctx.fallback_count()
    ctx.set_chunk_keys(TILE * 3)
    try:
        with grid_limit(2):
            c = ctx.histogram_fixed(keys, 13, m)
            c = ctx.histogram_fixed(keys, 13, m, counts=c)
    finally:
        ctx.set_chunk_keys(0)
    np.testing.assert_array_equal(c.cpu().numpy().view(np.uint32), 2 * expect(N_MANY, 13, m))
    assert ctx.fallback_count() == before
