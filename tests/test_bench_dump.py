"""bench.py --dump-outputs without a GPU: the row sample of a tall factor is fixed and bounded, the per-rank gathers add
up to the whole factor, and what is written is float32 / float64 within the size limit."""

import numpy as np
import pytest

import bench


def test_sample_rows_fixed_and_bounded():
    assert np.array_equal(bench.sample_rows(1000, 200, 24 << 20), np.arange(1000))
    r = bench.sample_rows(1036800, 200, 24 << 20)
    assert r.size == bench.DUMP_MAX_ROWS and np.all(np.diff(r) > 0) and r[0] >= 0 and r[-1] < 1036800
    assert np.array_equal(r, bench.sample_rows(1036800, 200, 24 << 20))
    assert bench.sample_rows(10 ** 6, 4000, 1 << 20).size == (1 << 20) // 4000


def test_gather_rows_over_shards_and_complex():
    torch = pytest.importorskip("torch")
    A = torch.randn(5000, 7)
    rows = bench.sample_rows(5000, 28, 28 * 600)
    whole = bench.gather_rows(A, 0, rows, 1, "cpu")
    assert np.array_equal(whole, A.numpy()[rows])
    parts = bench.gather_rows(A[:1234], 0, rows, 1, "cpu") + bench.gather_rows(A[1234:], 1234, rows, 1, "cpu")
    assert np.array_equal(parts, whole)
    outs = {}
    C = (np.arange(60) + 1j * np.arange(60)[::-1]).astype(np.complex64).reshape(20, 3)
    bench.factor_outputs(outs, "C", C, 0, 20, 1, "cpu", 1 << 20, itemsize=8)
    assert set(outs) == {"C_re", "C_im"} and np.array_equal(outs["C_re"] + 1j * outs["C_im"], C)


def test_write_outputs_dtypes_and_limit(tmp_path):
    bench.write_outputs(str(tmp_path / "d"), {"a": np.ones(3, np.float16), "b": np.arange(4), "c": np.zeros(2)})
    got = {f: np.load(tmp_path / "d" / f) for f in ("a.npy", "b.npy", "c.npy")}
    assert got["a.npy"].dtype == np.float32 and got["b.npy"].dtype == np.float64 and got["c.npy"].dtype == np.float64
    with pytest.raises(SystemExit):
        bench.write_outputs(str(tmp_path / "e"), {"big": np.zeros(bench.DUMP_MAX_BYTES // 4 + 1, np.float32)})
    assert not (tmp_path / "e").exists()
