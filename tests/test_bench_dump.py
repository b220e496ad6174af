"""bench.py --dump-outputs: what is written for the headline's outputs (bucket
counts and edge offsets at C4's bucket count) -- float arrays that hold the
integers exactly, the same sample positions on every call, 64 MB at most."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import bench  # noqa: E402

M_C4 = bench.README_N // 1500 + 1


@pytest.fixture(scope="module")
def outputs():
    g = torch.Generator().manual_seed(1)
    counts = torch.randint(1200, 1800, (M_C4,), dtype=torch.int32, generator=g)
    E = torch.zeros(M_C4 + 1, dtype=torch.int64)
    torch.cumsum(counts, 0, out=E[1:])
    return counts, E


def test_dump_outputs_writes_exact_float_arrays_within_the_limit(outputs, tmp_path):
    counts, E = outputs
    d = str(tmp_path / "a")
    bench.dump_outputs(d, {"counts": (counts, "float32"), "edge_offsets": (E, "float64")})
    assert sorted(os.listdir(d)) == ["counts.npy", "edge_offsets.npy"]
    assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 64_000_000
    c = np.load(os.path.join(d, "counts.npy"))
    assert c.dtype == np.float32 and np.array_equal(c.astype(np.int64), counts.numpy())  # written whole
    e = np.load(os.path.join(d, "edge_offsets.npy"))
    assert e.dtype == np.float64 and e.size == bench.DUMP_SAMPLE_ELEMS
    assert np.all(np.diff(e) > 0) and e[-1] == float(E[-1])                             # sorted positions, last kept
    assert np.isin(e.astype(np.int64), E.numpy()).all()


def test_dump_outputs_samples_the_same_positions_every_time(outputs, tmp_path):
    counts, E = outputs
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, {"edge_offsets": (E, "float64")})
    bench.dump_outputs(b, {"edge_offsets": (E + 7, "float64")})
    assert np.array_equal(np.load(os.path.join(a, "edge_offsets.npy")) + 7, np.load(os.path.join(b, "edge_offsets.npy")))
