"""Pass 1's bin insert and write-out (k_pass1_d13e): odd and even tile counts
per workgroup, a bin filled exactly to its capacity and one id past it (the
first bin, and the last, whose overflow is the one that could leave the LDS
buffer), a tile whose keys all fall into one bin, accumulation and a non-zero
seed.  Integer work: every comparison is bit-exact against the CPU oracle,
and every test checks the fallback counter."""
import contextlib
import functools
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle as O

gpu = pytest.mark.gpu

TILE = 16384
TAIL = 777
# one owner lane; a small shift; P = 269 (the last wave owns fewer bins than
# the others); P = 288 (every owner slot in use)
BUCKETS = [1, 667, 8_795_859, 9_437_184]
LENGTHS = [13, 8, 12, 16]
# (workgroups, whole tiles): two workgroups run 1+2, 2+2, 3+2 and 3+3 tiles,
# one workgroup 1, 2 and 3.  The ragged tail goes to the bounds-checked
# kernel, and keeps the last whole tile's 16-byte windows inside the buffer,
# so the persistent kernel runs exactly these tiles.
SPLITS = [(2, 3), (2, 4), (2, 5), (2, 6), (1, 1), (1, 2), (1, 3)]
# m = 8 795 859: 269 bins of 32768 buckets, 136 ids each (test_bins_of_c4)
C4_M, C4_BINS, C4_CAPB, BIN_SHIFT = 8_795_859, 269, 136, 15
POOL = 40 * TILE  # keys to pick from: ~2400 of bin 0, ~1000 of the short bin 268


def test_bins_of_c4(tmp_path):
    """The bin geometry the capacity tests rely on, from hist_plan.hpp itself."""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler on this machine")
    exe = str(tmp_path / "hist_plan_check")
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hist_plan_check.cpp")
    subprocess.run([cxx, "-std=c++17", "-O1", "-o", exe, src], check=True)
    case = f"var=0 key_len=13 n={2 * TILE + TAIL} m={C4_M} blob_bytes={13 * (2 * TILE + TAIL)} seed0=1 wg_per_cu=1 " \
           f"free_bytes={256 * 10**9}\n"
    r = subprocess.run([exe], input=case, capture_output=True, text=True, check=True)
    p = json.loads(r.stdout)
    assert (p["kind"], p["nparts"], p["bin_shift"], p["capb"]) == ("d13e", C4_BINS, BIN_SHIFT, C4_CAPB)
    assert (p["launches"], p["spans"]) == (1, 1)  # one overflow: one span recounted


def test_kernel_registers_and_scratch(tmp_path):
    """Every form of k_pass1_d13e the library launches, compiled for gfx950 with
    the library's flags and warnings as errors: at most 128 VGPRs (1024 threads
    a workgroup), nothing spilled, no scratch, LDS within the CU's 160 KiB."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc"))
                  if c and os.path.exists(c)), None)
    if hipcc is None:
        pytest.skip("no hipcc on this machine")
    forms = [(13, s, 13) for s in ("true", "false")] + [(0, s, L) for s in ("true", "false") for L in (13, 8, 12, 16)]
    src = tmp_path / "forms.hip"
    src.write_text('#include "hash_kernels.hip"\nnamespace bsdb {\n' + "".join(
        f"template __global__ void k_pass1_d13e<{v}, {s}, {L}>(P1Args, uint64_t);\n" for v, s, L in forms) + "}\n")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fgpu-flush-denormals-to-zero", "-Wall",
                        "-Werror", "-Wno-unused-function", "--cuda-device-only", "-c",
                        "-Rpass-analysis=kernel-resource-usage", "-I", os.path.join(root, "bsdb_amd", "csrc"),
                        "-o", str(tmp_path / "forms.o"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    seen, name = {}, None
    for line in r.stderr.splitlines():
        if "remark:" not in line:
            continue
        key, _, val = line.split("remark:", 1)[1].rsplit("[-Rpass", 1)[0].strip().partition(":")
        if key == "Function Name":
            name = val.strip()
            seen[name] = {}
        elif name is not None:
            seen[name][key.strip()] = val.strip()
    mine = {n: u for n, u in seen.items() if "k_pass1_d13eIL" in n}
    assert len(mine) == len(forms), sorted(seen)
    for n, u in mine.items():
        assert int(u["VGPRs"]) <= 128 and int(u["AGPRs"]) == 0, (n, u)
        assert int(u["ScratchSize [bytes/lane]"]) == 0 and int(u["VGPRs Spill"]) == 0 and int(u["SGPRs Spill"]) == 0, (n, u)
        assert int(u["LDS Size [bytes/block]"]) <= 160 * 1024, (n, u)


@pytest.fixture(scope="module")
def ctx():
    torch = pytest.importorskip("torch")
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
def expect(n, L, m, seed=0):
    c = O.histogram_fixed(keys_of(n, L), L, m, seed)
    c.setflags(write=False)
    return c


def exact(keys):
    """The keys in a device buffer that ends exactly at their last byte."""
    import torch
    t = torch.from_numpy(np.array(keys)).cuda()
    assert t.numel() == keys.size
    return t


def run(ctx, keys, L, m, grid, **kw):
    with grid_limit(grid):
        return ctx.histogram_fixed(exact(keys), L, m, **kw).cpu().numpy().view(np.uint32)


@gpu
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("m", BUCKETS)
@pytest.mark.parametrize("grid,tiles", SPLITS)
def test_odd_and_even_tiles_per_workgroup(ctx, grid, tiles, m, L):
    n = tiles * TILE + TAIL
    before = ctx.fallback_count()
    counts = run(ctx, keys_of(n, L), L, m, grid)
    np.testing.assert_array_equal(counts, expect(n, L, m))
    # (a corrupted reservation or carry overflows, and the fallback's recount
    # would hide it: random distinct keys never take the fallback)
    assert ctx.fallback_count() == before


@functools.lru_cache(maxsize=None)
def pool():
    """POOL distinct 13-byte keys as rows, and each key's bin at m = C4_M."""
    k = keys_of(POOL, 13).reshape(POOL, 13)
    b = O.buckets(O.hash_fixed(keys_of(POOL, 13), 13), C4_M) >> BIN_SHIFT
    assert int(b.max()) == C4_BINS - 1
    return k, b


@functools.lru_cache(maxsize=None)
def filled(target, fill):
    """Two tiles and a tail of distinct keys whose first tile puts exactly
    `fill` ids into bin `target`, at scattered places of the tile; every other
    key, of all three parts, belongs to another bin."""
    k, b = pool()
    mine, other = np.flatnonzero(b == target), np.flatnonzero(b != target)
    n = 2 * TILE + TAIL
    assert mine.size >= fill and other.size >= n - fill
    idx = other[: n - fill].copy()
    at = np.sort(np.random.default_rng(5).choice(TILE, fill, replace=False))
    idx = np.insert(idx, at - np.arange(fill), mine[:fill])  # mine[i] ends up at position at[i]
    assert idx.size == n and np.array_equal(np.flatnonzero(b[idx] == target), at)
    # the bins of the first tile: the target at `fill`, no other over its capacity
    per_bin = np.bincount(b[idx[:TILE]], minlength=C4_BINS)
    assert per_bin[target] == fill and np.delete(per_bin, target).max() <= C4_CAPB
    assert np.bincount(b[idx[TILE:2 * TILE]], minlength=C4_BINS).max() <= C4_CAPB
    keys = np.ascontiguousarray(k[idx]).reshape(-1)
    keys.setflags(write=False)
    want = O.histogram_fixed(keys, 13, C4_M)
    want.setflags(write=False)
    return keys, want


@gpu
@pytest.mark.parametrize("target", [0, C4_BINS - 1])
@pytest.mark.parametrize("fill,recounts", [(C4_CAPB, 0), (C4_CAPB + 1, 1)])
def test_bin_at_capacity_and_one_past(ctx, fill, recounts, target):
    keys, want = filled(target, fill)
    before = ctx.fallback_count()
    counts = run(ctx, keys, 13, C4_M, 2)
    np.testing.assert_array_equal(counts, want)
    # a full bin is no overflow; one id more recounts the call's one span, once
    assert ctx.fallback_count() == before + recounts


@gpu
@pytest.mark.parametrize("target", [0, C4_BINS - 1])
def test_every_key_of_a_tile_in_one_bin(ctx, target):
    k, b = pool()
    n = 2 * TILE + TAIL
    keys = np.tile(k[np.flatnonzero(b == target)[0]], n)
    want = O.histogram_fixed(keys, 13, C4_M)
    assert np.count_nonzero(want) == 1 and int(want.sum()) == n
    before = ctx.fallback_count()
    counts = run(ctx, keys, 13, C4_M, 2)
    np.testing.assert_array_equal(counts, want)  # (every other bucket, of this bin and its neighbours, stays 0)
    assert ctx.fallback_count() == before + 1


@gpu
def test_accumulates_with_a_seed(ctx):
    """The kernel without the folded seed, adding into counts that are not zero."""
    n, seed = 5 * TILE + TAIL, 0x5EED0123456789AB
    before = ctx.fallback_count()
    with grid_limit(2):
        c = ctx.histogram_fixed(exact(keys_of(n, 13)), 13, C4_M, seed=seed)
        first = c.cpu().numpy().view(np.uint32).copy()
        c = ctx.histogram_fixed(exact(keys_of(n, 13)), 13, C4_M, counts=c, seed=seed)
    np.testing.assert_array_equal(first, expect(n, 13, C4_M, seed))
    assert not np.array_equal(first, expect(n, 13, C4_M))
    np.testing.assert_array_equal(c.cpu().numpy().view(np.uint32), 2 * expect(n, 13, C4_M, seed))
    assert ctx.fallback_count() == before
