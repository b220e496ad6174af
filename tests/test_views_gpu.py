"""Inputs and outputs as views into larger buffers.  A fresh allocation starts on
a 256-byte boundary and is followed by allocator slack, so four things go
unnoticed: a kernel whose result depends on bytes outside the key range, a
kernel that writes a word before or after its output, a var-len blob whose base
is not 16-byte aligned (the header asks no alignment of it), and fixed keys at a
16-byte but not 256-byte aligned address.

 * embedded(): the input sits at byte `lead` of a buffer filled with 0x00 or
   0xFF and ends exactly at its last key, 64 bytes of the fill behind it.  Every
   input case runs with both fills and must equal the oracle's result.
 * guarded(): the output is a window between two bands of 64 sentinel words;
   bands_untouched() synchronises and checks both bands of every buffer.

Integer and byte work: every comparison is exact."""
import contextlib
import functools

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

THREADS = O.cpu_threads()
NONE = 2**64 - 1
EINVAL = -22
ROUND = 256 * 16384
GUARD = 64
SENTINEL = {torch.int64: 0x5A5A5A5A5A5A5A5A, torch.int32: 0x5A5A5A5A, torch.uint8: 0x5A}
FILLS = [0x00, 0xFF]
TAIL = 64
M_C4 = 8_795_859
ADDR_BASE, ADDR_STRIDE = 1 << 33, 24


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from bsdb_amd import Context
    c = Context(0)
    yield c
    c.close()


@contextlib.contextmanager
def knobs(ctx, frontend=0, mode=0):
    ctx.set_frontend(frontend)
    ctx.set_histogram_mode(mode)
    try:
        yield
    finally:
        ctx.set_frontend(0)
        ctx.set_histogram_mode(0)


# ---- the two helpers ---------------------------------------------------------------

def embedded(data, lead, tail=TAIL, fill=0):
    """`data`'s bytes at byte `lead` of a device buffer of lead + size + tail
    bytes filled with `fill`: the view of exactly those bytes (numel() is
    exact, data_ptr() is offset, the view ends at the last key)."""
    data = np.array(data, order="C").view(np.uint8).reshape(-1)
    buf = torch.full((lead + data.size + tail,), fill, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    view = buf[lead: lead + data.size]
    view.copy_(torch.from_numpy(data))
    assert view.numel() == data.size and view.data_ptr() == buf.data_ptr() + lead
    return view


def guarded(words, dtype, inside=0):
    """(buf, window): `words` elements set to `inside` between two bands of GUARD sentinel elements."""
    buf = torch.full((GUARD + words + GUARD,), SENTINEL[dtype], dtype=dtype, device="cuda")
    window = buf[GUARD: GUARD + words]
    window.fill_(inside)
    return buf, window


def bands_untouched(*bufs):
    torch.cuda.synchronize()
    for buf in bufs:
        s = SENTINEL[buf.dtype]
        assert bool(torch.all(buf[:GUARD] == s)) and bool(torch.all(buf[-GUARD:] == s))


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def u64(t):
    return t.cpu().numpy().view(np.uint64)


# ---- key sets -----------------------------------------------------------------------

N_VAR = 3 * 8192 + 777
GROUP = 8192 + 1024  # the first key of a 128-key group of wave 0


@functools.lru_cache(maxsize=None)
def var_set(distinct=False):
    """Keys of 0..64 bytes, a zero-length key first and (unless `distinct`, for
    the builds: a one-byte key then) a zero-length key last, so the first and
    the last read sit at the view's edges; one key of each length 1..7; one
    128-key group over k_pass1_vare's 4352-byte stage.  The keys of 8 bytes
    and more are random, hence distinct.  (blob, offsets)."""
    rng = np.random.default_rng(41)
    lens = rng.integers(8, 65, N_VAR)
    lens[0:8] = np.arange(8)
    lens[GROUP: GROUP + 128] = rng.integers(40, 65, 128)
    assert lens[GROUP: GROUP + 128].sum() > 4352
    lens[-1] = 1 if distinct else 0
    off = np.zeros(N_VAR + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    blob = rng.integers(0, 256, int(off[-1]), dtype=np.uint8)
    if distinct:
        blob[-1] = blob[0] ^ 0xFF  # (key 1 is blob[0:1])
    blob.setflags(write=False)
    off.setflags(write=False)
    return blob, off


def var_key(i, distinct=False):
    blob, off = var_set(distinct)
    return blob[int(off[i]): int(off[i + 1])].tobytes()


@functools.lru_cache(maxsize=None)
def var_sig():
    return O.hash_var(*var_set())


@functools.lru_cache(maxsize=None)
def var_counts(m):
    return O.histogram_var(*var_set(), m)


@functools.lru_cache(maxsize=None)
def keys_of(n, L):
    """n random distinct keys of L bytes (the 13-byte recipe's byte stream, cut every L bytes)."""
    k = O.gen_keys13_mt(6262, (n * L + 12) // 13, THREADS)[: n * L]
    k.setflags(write=False)
    return k


@functools.lru_cache(maxsize=None)
def fixed_counts(n, L, m):
    return O.histogram_fixed_mt(keys_of(n, L), L, m, THREADS)[0]


def dev_off(off):
    return dev(off.view(np.int64))


# ================================================================= inputs: a var-len blob at any base

VAR_LEADS = [1, 3, 4, 8, 15]


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("lead", VAR_LEADS)
def test_hash_var_blob_base(ctx, lead, fill):
    blob, off = var_set()
    view, doff = embedded(blob, lead, fill=fill), dev_off(off)
    for frontend in (0, 2):  # VARSTAGED, VAR
        with knobs(ctx, frontend):
            np.testing.assert_array_equal(u64(ctx.hash_var(view, doff)), var_sig())


# mode 0: k_pass1_vare (it rounds blob + first down to 16 bytes) and the tail's
# SRC_VAR; front end 1: SRC_VARSTAGED (it rounds the offset down); 2: SRC_VAR
@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("lead", VAR_LEADS)
@pytest.mark.parametrize("frontend,mode", [(0, 0), (1, 0), (2, 0), (0, 2)])
def test_histogram_var_blob_base(ctx, frontend, mode, lead, fill):
    blob, off = var_set()
    view, doff = embedded(blob, lead, fill=fill), dev_off(off)
    before = ctx.fallback_count()
    with knobs(ctx, frontend, mode):
        for m in (40_000, 144 * 32768):
            np.testing.assert_array_equal(u32(ctx.histogram_var(view, doff, m)), var_counts(m))
    assert ctx.fallback_count() == before  # (a recount would hide a wrong pass 1)


@pytest.fixture(scope="module")
def var_db(ctx):
    """A small database on the distinct var-len set, built from an aligned blob:
    (E, values, sigbits, index, width), equal to the oracle's build."""
    blob, off = var_set(True)
    width = 4
    index = torch.zeros(N_VAR, dtype=torch.int64, device="cuda")
    E, values, sigbits, _ = ctx.mph_build_index_passes(dev(blob), 0, N_VAR, width, offsets=dev_off(off),
                                                       addr_base=ADDR_BASE, addr_stride=ADDR_STRIDE, index=index)
    return E, values, sigbits, index, width


@functools.lru_cache(maxsize=None)
def var_build(width):
    sig = O.hash_var(*var_set(True))
    rc, E, values, sigbits = O.gov_build(sig, width)
    assert rc == 0
    rank = O.lookup_batch(sig, N_VAR, E, values, width, sigbits, False)
    addr = (ADDR_BASE + ADDR_STRIDE * np.arange(N_VAR, dtype=np.uint64))
    index = np.zeros(N_VAR, np.uint64)
    index[rank] = addr.byteswap()
    return E, values, sigbits, index


def check_var_build(E, values, sigbits, index, width):
    wE, wv, ws, wi = var_build(width)
    np.testing.assert_array_equal(u64(E), wE)
    np.testing.assert_array_equal(u64(values), wv)
    np.testing.assert_array_equal(u64(sigbits)[: ws.size], ws)
    np.testing.assert_array_equal(u64(index), wi)


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("lead", VAR_LEADS)
def test_verify_var_blob_base(ctx, var_db, lead, fill):
    E, values, sigbits, index, width = var_db
    check_var_build(E, values, sigbits, index, width)
    blob, off = var_set(True)
    got = ctx.verify_var(embedded(blob, lead, fill=fill), dev_off(off), N_VAR, E, values, index, width=width,
                         sigbits=sigbits, addr_base=ADDR_BASE, addr_stride=ADDR_STRIDE)
    assert got == (N_VAR, 0, N_VAR, 0, 0, NONE)


@functools.lru_cache(maxsize=None)
def var_pairs():
    """Pairs of positions of var_set() with their kinds: the two empty keys, keys
    at the view's edges, a key against itself, random pairs."""
    rng = np.random.default_rng(43)
    n = N_VAR
    pairs = [(0, n - 1), (n - 1, 0), (0, 1), (1, 2), (5, 5), (n - 2, n - 1), (n - 2, n - 2), (GROUP, GROUP + 127)]
    pairs += [tuple(p) for p in rng.integers(0, n, (300, 2)).tolist()]
    pairs += [(int(i), int(i)) for i in rng.integers(0, n, 50)]
    kinds = [0 if var_key(a) == var_key(b) else 1 for a, b in pairs]
    assert kinds[:7] == [0, 0, 1, 1, 0, 1, 0]
    return np.array(pairs, np.int64), np.array(kinds, np.uint8)


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("lead", VAR_LEADS)
def test_classify_pairs_var_blob_base(ctx, lead, fill):
    blob, off = var_set()
    pairs, kinds = var_pairs()
    got = ctx.classify_pairs_var(embedded(blob, lead, fill=fill), dev_off(off), dev(pairs))
    np.testing.assert_array_equal(got.cpu().numpy(), kinds)


DWORD_LEADS = [4, 8, 12]


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("lead", DWORD_LEADS)
def test_find_duplicates_var_blob_base(ctx, lead, fill):
    blob, off = var_set()
    rep = ctx.find_duplicates_var(embedded(blob, lead, fill=fill), dev_off(off))
    assert rep["found"] == 1 and rep["keys"] == N_VAR and not rep["list_full"] and not rep["partial"]
    assert rep["pairs"].tolist() == [[0, N_VAR - 1]] and rep["kinds"].tolist() == [0] and rep["collisions"] == 0


def test_find_duplicates_var_refuses_an_odd_base(ctx):
    from bsdb_amd.native import BsdbError
    blob, off = var_set()
    with pytest.raises(BsdbError) as e:  # the header: d_blob 4-byte aligned
        ctx.find_duplicates_var(embedded(blob, 1), dev_off(off))
    assert e.value.code == EINVAL


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("lead", DWORD_LEADS)
def test_passes_build_var_blob_base(ctx, lead, fill):
    """bsdb_dev_mph_build_index_passes_var (k_sel KIND 2) in two passes."""
    blob, off = var_set(True)
    width = 7
    index = torch.zeros(N_VAR, dtype=torch.int64, device="cuda")
    E, values, sigbits, used = ctx.mph_build_index_passes(embedded(blob, lead, fill=fill), 0, N_VAR, width, passes=2,
                                                          offsets=dev_off(off), addr_base=ADDR_BASE,
                                                          addr_stride=ADDR_STRIDE, index=index)
    assert used >= 1
    check_var_build(E, values, sigbits, index, width)


# ================================================================= inputs: fixed keys at 16-byte addresses

FIXED_LEADS = [16, 48]
FIXED_L = [5, 8, 13, 16, 40]
N_FIXED = 3 * 16384 + 777  # whole tiles for the persistent kernels and a bounds-checked tail


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("lead", FIXED_LEADS)
@pytest.mark.parametrize("L", FIXED_L)
def test_hash_fixed_in_a_view(ctx, L, lead, fill):
    n = 20_001
    k = keys_of(n, L)
    np.testing.assert_array_equal(u64(ctx.hash_fixed(embedded(k, lead, fill=fill), L)), O.hash_fixed(k, L))


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("lead", FIXED_LEADS)
@pytest.mark.parametrize("L", FIXED_L)
@pytest.mark.parametrize("frontend", [0, 1])
def test_histogram_fixed_in_a_view(ctx, frontend, L, lead, fill):
    view = embedded(keys_of(N_FIXED, L), lead, fill=fill)
    before = ctx.fallback_count()
    with knobs(ctx, frontend):
        got = u32(ctx.histogram_fixed(view, L, M_C4))
    np.testing.assert_array_equal(got, fixed_counts(N_FIXED, L, M_C4))
    assert ctx.fallback_count() == before


N_DB = 20_011


@pytest.fixture(scope="module")
def fixed_db(ctx):
    """A small database per key length, built from aligned keys, opened on first use."""
    made = {}

    def get(L):
        if L not in made:
            index = torch.zeros(N_DB, dtype=torch.int64, device="cuda")
            E, values, sigbits, _ = ctx.mph_build_index_passes(dev(keys_of(N_DB, L)), L, N_DB, 4, addr_base=ADDR_BASE,
                                                               addr_stride=ADDR_STRIDE, index=index)
            sig = O.hash_fixed(keys_of(N_DB, L), L)
            rc, wE, wv, ws = O.gov_build(sig, 4)
            assert rc == 0
            np.testing.assert_array_equal(u64(E), wE)
            np.testing.assert_array_equal(u64(values), wv)
            made[L] = (E, values, sigbits, index)
        return made[L]
    return get


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("lead", FIXED_LEADS)
@pytest.mark.parametrize("L", FIXED_L)
def test_verify_fixed_in_a_view(ctx, fixed_db, L, lead, fill):
    E, values, sigbits, index = fixed_db(L)
    got = ctx.verify_fixed(embedded(keys_of(N_DB, L), lead, fill=fill), L, N_DB, E, values, index, width=4,
                           sigbits=sigbits, addr_base=ADDR_BASE, addr_stride=ADDR_STRIDE)
    assert got == (N_DB, 0, N_DB, 0, 0, NONE)


@functools.lru_cache(maxsize=None)
def planted(L):
    """5 000 keys of L bytes with ten copies planted, the last key among them: (keys, pairs)."""
    n = 5000
    k = keys_of(n, L).reshape(n, L).copy()
    src = np.arange(10) * 97 + 3
    dst = np.arange(10) * 211 + 2000
    dst[-1] = n - 1
    k[dst] = k[src]
    return k.reshape(-1), np.stack([src, dst], 1).astype(np.uint64)


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("lead", FIXED_LEADS)
@pytest.mark.parametrize("L", FIXED_L)
def test_find_duplicates_fixed_in_a_view(ctx, L, lead, fill):
    k, want = planted(L)
    rep = ctx.find_duplicates_fixed(embedded(k, lead, fill=fill), L)
    assert rep["found"] == 10 and rep["keys"] == 5000 and not rep["list_full"] and not rep["partial"]
    np.testing.assert_array_equal(rep["pairs"], want)
    assert rep["kinds"].tolist() == [0] * 10


@pytest.mark.parametrize("L", [8, 13])
def test_fixed_keys_at_a_dword_address_are_refused(ctx, L):
    from bsdb_amd.native import BsdbError
    view = embedded(keys_of(20_001, L), 4)
    for call in (lambda: ctx.hash_fixed(view, L), lambda: ctx.histogram_fixed(view, L, 667)):
        with pytest.raises(BsdbError) as e:
            call()
        assert e.value.code == EINVAL


# ================================================================= outputs between guard bands

@pytest.mark.parametrize("L", [13, 40])
def test_hash_fixed_output(ctx, L):
    n = 20_001
    k = keys_of(n, L)
    buf, out = guarded(2 * n, torch.int64)
    ctx.hash_fixed(dev(k), L, out=out)
    bands_untouched(buf)
    np.testing.assert_array_equal(u64(out).reshape(n, 2), O.hash_fixed(k, L))


def test_hash_var_output(ctx):
    blob, off = var_set()
    buf, out = guarded(2 * N_VAR, torch.int64)
    ctx.hash_var(dev(blob), dev_off(off), out=out)
    bands_untouched(buf)
    np.testing.assert_array_equal(u64(out).reshape(N_VAR, 2), var_sig())


# m = 1; a last partition of 667 buckets; of one bucket (32 769 = 32 768 + 1); of 13 907 (C4, m odd)
BUCKETS = [1, 667, 32_769, M_C4]


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("m", BUCKETS)
def test_histogram_counts_output(ctx, m, mode):
    blob, off = var_set()
    fixed, dblob, doff = dev(keys_of(N_FIXED, 13)), dev(blob), dev_off(off)
    with knobs(ctx, mode=mode):
        buf, counts = guarded(m, torch.int32)
        ctx.histogram_fixed(fixed, 13, m, counts=counts)
        bands_untouched(buf)
        np.testing.assert_array_equal(u32(counts), fixed_counts(N_FIXED, 13, m))
        buf, counts = guarded(m, torch.int32)
        ctx.histogram_var(dblob, doff, m, counts=counts)
        bands_untouched(buf)
        np.testing.assert_array_equal(u32(counts), var_counts(m))


N_FUSED = 4 * ROUND + 5


@pytest.fixture(scope="module")
def fused_keys():
    return dev(keys_of(N_FUSED, 13))


@pytest.mark.parametrize("m", BUCKETS)
def test_single_pass_counts_output(ctx, fused_keys, m):
    """Mode 3: the single-pass kernel where it qualifies (<= 16 384 keys a bucket), and its five-key two-pass tail."""
    launches = ctx.fused_status()[0]
    buf, counts = guarded(m, torch.int32)
    with knobs(ctx, mode=3):
        ctx.histogram_fixed(fused_keys, 13, m, counts=counts)
    bands_untouched(buf)
    np.testing.assert_array_equal(u32(counts), fixed_counts(N_FUSED, 13, m))
    now, timeouts = ctx.fused_status()
    assert timeouts == 0 and (now > launches) == (N_FUSED // m <= 16384)


@pytest.mark.parametrize("m", [1, 8192, 8193])
def test_edge_offsets_output(ctx, m):
    c = np.random.default_rng(m).integers(0, 3000, m).astype(np.uint32)
    buf, out = guarded(m + 1, torch.int64)
    ctx.edge_offsets(dev(c.view(np.int32)), out=out)
    bands_untouched(buf)
    np.testing.assert_array_equal(u64(out), O.edge_offsets(c))


def rand_sigs(n, seed):
    return np.random.default_rng(seed).integers(0, 1 << 64, (n, 2), dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def gov_set(n, width):
    sig = rand_sigs(n, 1000 * n + width)
    rc, E, values, sigbits = O.gov_build(sig, width)
    assert rc == 0
    return sig, E, values, sigbits


def test_lookup_output(ctx):
    n, width = 20_000, 5
    sig, E, values, sigbits = gov_set(n, width)
    queries = np.concatenate([sig, rand_sigs(5_001, 9)])  # present and absent keys
    dE, dv, ds = dev(E.view(np.int64)), dev(values.view(np.int64)), dev(sigbits.view(np.int64))
    for check in (False, True):
        buf, out = guarded(queries.shape[0], torch.int64, inside=-7)
        ctx.lookup(dev(queries.view(np.int64)), n, dE, dv, width, ds, check=check, out=out)
        bands_untouched(buf)
        np.testing.assert_array_equal(out.cpu().numpy(), O.lookup_batch(queries, n, E, values, width, sigbits, check))


@pytest.mark.parametrize("width", [3, 64])
def test_sign_output(ctx, width):
    n = 20_000
    sig, E, values, sigbits = gov_set(n, width)
    words = (n * width + 63) // 64 + 1
    assert sigbits.size == words
    buf, out = guarded(words, torch.int64)
    ctx.sign(dev(sig.view(np.int64)), dev(E.view(np.int64)), dev(values.view(np.int64)), width, out=out)
    bands_untouched(buf)
    np.testing.assert_array_equal(u64(out), sigbits)


def test_index_scatter_output(ctx):
    rng = np.random.default_rng(11)
    n, start, length = 30_000, 5_000, 7_000
    rank = rng.permutation(n).astype(np.int64)
    rejected = np.arange(0, n, 97)  # rejected lookups (rank -1) are skipped; not the window's two end slots
    rank[rejected[~np.isin(rank[rejected], (start, start + length - 1))]] = -1
    addr = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    v8 = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    vlen = rng.integers(0, 41, n).astype(np.uint8)
    inside = np.flatnonzero((rank >= start) & (rank < start + length))
    vlen[inside[:4]] = [0, 40, 0, 40]
    # the window's first and last slots are written
    assert {start, start + length - 1} <= set(rank[inside].tolist())
    buf_i, index = guarded(length, torch.int64)
    buf_a, index_a = guarded(8 * length, torch.uint8)
    ctx.index_scatter(dev(rank), dev(addr.view(np.int64)), start, length, index, dev(v8.view(np.int64)), dev(vlen), index_a)
    bands_untouched(buf_i, buf_a)
    want = np.zeros(length, np.uint64)
    want_a = np.zeros((length, 8), np.uint8)
    want[rank[inside] - start] = addr[inside].byteswap()
    vb = v8[inside].view(np.uint8).reshape(-1, 8)  # little-endian bytes of value8
    keep = np.arange(8)[None, :] < np.minimum(vlen[inside], 8)[:, None]  # zeros past min(vlen, 8)
    want_a[rank[inside] - start] = np.where(keep, vb, 0)
    np.testing.assert_array_equal(u64(index), want)
    np.testing.assert_array_equal(index_a.cpu().numpy(), want_a.reshape(-1))


@pytest.mark.parametrize("width", [0, 5, 64])
@pytest.mark.parametrize("n", [1, 3001, 20_000])
@pytest.mark.parametrize("ranks", [False, True])
def test_gov_build_outputs(ctx, ranks, n, width):
    from bsdb_amd.native import num_buckets
    sig, E, values, sigbits = gov_set(n, width)
    assert E.size == num_buckets(n) + 1
    bE, wE = guarded(E.size, torch.int64, inside=-1)
    bv, wv = guarded(values.size, torch.int64, inside=-1)
    bs, ws = guarded(sigbits.size, torch.int64, inside=-1) if width else (None, None)
    br, wr = guarded(n, torch.int64, inside=-1)
    dsig = dev(sig.view(np.int64))
    if ranks:
        got = ctx.gov_build_ranks(dsig, width, E=wE, values=wv, sigbits=ws, rank=wr)
        assert got[3] is wr
        bands_untouched(br)
        np.testing.assert_array_equal(wr.cpu().numpy(), O.lookup_batch(sig, n, E, values, width, sigbits, False))
    else:
        got = ctx.gov_build(dsig, width, E=wE, values=wv, sigbits=ws)
    assert got[0] is wE and got[1] is wv and got[2] is ws
    bands_untouched(*(b for b in (bE, bv, bs) if b is not None))
    np.testing.assert_array_equal(u64(wE), E)
    np.testing.assert_array_equal(u64(wv), values)
    if width:
        np.testing.assert_array_equal(u64(ws), sigbits)


def test_gov_build_allocates_its_outputs_by_default(ctx):
    sig, E, values, sigbits = gov_set(3001, 5)
    dE, dv, ds = ctx.gov_build(dev(sig.view(np.int64)), 5)
    assert (dE.numel(), dv.numel(), ds.numel()) == (E.size, values.size, sigbits.size)
    np.testing.assert_array_equal(u64(dE), E)
    assert ctx.gov_build(dev(sig.view(np.int64)), 0)[2] is None
    with pytest.raises(ValueError):
        ctx.gov_build(dev(sig.view(np.int64)), 5, E=dE[:-1])


# G = 5 > m = 2: ranks that own no bucket
@pytest.mark.parametrize("m,G", [(667, 1), (667, 3), (667, 64), (2, 5)])
def test_partition_owners_outputs(ctx, m, G):
    n = 20_000
    sig = rand_sigs(n, 17 * G + m)
    own = ((O.buckets(sig, m).astype(np.int64) + 1) * G - 1) // m
    want_counts = [int((own == g).sum()) for g in range(G)]
    bo, out = guarded(2 * n, torch.int64)
    bp, pout = guarded(n, torch.int64)
    got, gotp, counts = ctx.partition_owners(dev(sig.view(np.int64)), m, G,
                                             payload=torch.arange(n, dtype=torch.int64, device="cuda"),
                                             out=out.view(n, 2), payload_out=pout)
    bands_untouched(bo, bp)
    assert counts == want_counts and sum(counts) == n
    if (m, G) == (2, 5):
        assert counts[0] == counts[1] == counts[3] == 0 and counts[2] and counts[4]
    pay = pout.cpu().numpy()
    np.testing.assert_array_equal(np.sort(pay), np.arange(n))
    np.testing.assert_array_equal(u64(out).reshape(n, 2), sig[pay])  # the payload travels with its signature
    np.testing.assert_array_equal(own[pay], np.repeat(np.arange(G), counts))  # rank 0's first


def test_find_duplicates_list_full_output(ctx):
    """found > cap: `pairs` has exactly cap rows, `kinds` exactly cap bytes."""
    k, want = planted(13)
    cap = 4
    bp, pairs = guarded(2 * cap, torch.int64)
    bk, kinds = guarded(cap, torch.uint8, inside=9)
    br, report = guarded(4, torch.int64)
    rep = ctx.find_duplicates_fixed(dev(k), 13, cap=cap, pairs=pairs.view(cap, 2), kinds=kinds, report=report)
    bands_untouched(bp, bk, br)
    assert rep["found"] == 10 and rep["list_full"] and not rep["partial"] and rep["keys"] == 5000
    listed = {tuple(p) for p in rep["pairs"].tolist()}
    assert len(listed) == cap and listed <= {tuple(p) for p in want.tolist()}
    assert kinds.cpu().tolist() == [0] * cap and rep["collisions"] == 0


def test_classify_pairs_outputs(ctx):
    blob, off = var_set()
    pairs, kinds = var_pairs()
    buf, out = guarded(pairs.shape[0], torch.uint8, inside=9)
    ctx.classify_pairs_var(dev(blob), dev_off(off), dev(pairs), kinds=out)
    bands_untouched(buf)
    np.testing.assert_array_equal(out.cpu().numpy(), kinds)
    k, want = planted(13)
    fpairs = np.concatenate([want.astype(np.int64), np.array([[0, 1], [4999, 4998], [7, 7]], np.int64)])
    buf, out = guarded(fpairs.shape[0], torch.uint8, inside=9)
    ctx.classify_pairs_fixed(dev(k), 13, dev(fpairs), kinds=out)
    bands_untouched(buf)
    assert out.cpu().tolist() == [0] * 10 + [1, 1, 0]


def test_verify_report_output(ctx, var_db, fixed_db):
    E, values, sigbits, index, width = var_db
    blob, off = var_set(True)
    buf, out = guarded(8, torch.int64)
    out[5] = -1
    got = ctx.verify_var(dev(blob), dev_off(off), N_VAR, E, values, index, width=width, sigbits=sigbits,
                         addr_base=ADDR_BASE, addr_stride=ADDR_STRIDE, out=out)
    bands_untouched(buf)
    assert got == (N_VAR, 0, N_VAR, 0, 0, NONE) and u64(out)[6:].tolist() == [0, 0]
    E, values, sigbits, index = fixed_db(13)
    spoiled = index.clone()
    spoiled[100] = 7
    buf, out = guarded(8, torch.int64)
    out[5] = -1
    got = ctx.verify_fixed(dev(keys_of(N_DB, 13)), 13, N_DB, E, values, spoiled, width=4, sigbits=sigbits,
                           addr_base=ADDR_BASE, addr_stride=ADDR_STRIDE, out=out)
    bands_untouched(buf)
    assert got[:5] == (N_DB, 0, N_DB, 1, 0) and got[5] != NONE and u64(out)[6:].tolist() == [0, 0]


# the generator stores dwords per block of 256 keys, bytes at the end
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_key_generator_outputs(ctx, n):
    first = 123_456_789_000
    buf, out = guarded(13 * n, torch.uint8)
    ctx.gen_keys13(first, n, out=out)
    bands_untouched(buf)
    np.testing.assert_array_equal(out.cpu().numpy(), O.gen_keys13(first, n))
    wblob, woff = O.gen_keys_var(first, n)
    bo, offsets = guarded(n + 1, torch.int64, inside=-1)
    bb, blob = guarded(wblob.size, torch.uint8)
    ctx.gen_keys_var(first, n, offsets=offsets, blob=blob)
    bands_untouched(bo, bb)
    np.testing.assert_array_equal(u64(offsets), woff)
    np.testing.assert_array_equal(blob.cpu().numpy(), wblob)
