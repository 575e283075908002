"""CPU: bench.py's options -- a plain run asks for the headline only, --full for every other leg; --dump-outputs writes float64 .npy
files of at most 64 MB, a fixed seeded sample of the starts when the outputs are larger."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_plain_run_has_no_extra_legs_and_full_has_them():
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and not a.full and not a.extras and a.dump_outputs is None
    assert (a.sweep_starts, a.sweep_large_starts, a.sweep_xl_starts, a.sweep_c5_starts) == (0, 0, 0, 0)
    f = bench.parse_args(["--full"])
    assert f.full and f.extras
    assert (f.sweep_starts, f.sweep_large_starts, f.sweep_xl_starts, f.sweep_c5_starts) == (65536, 8 * 65536, 64 * 65536, 16384)
    lean = bench.parse_args(["--full", "--lean", "--sweep-starts", "200"])
    assert lean.full and not lean.extras and lean.sweep_starts == 200 and lean.sweep_large_starts == 0
    assert bench.parse_args(["--dump-outputs", "out"]).dump_outputs == "out"
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


def test_dump_outputs_writes_everything_when_it_fits(tmp_path):
    import torch
    import bench
    rows = torch.arange(8 * 15 * 14, dtype=torch.float64).reshape(8, 15, 14)
    jac = -torch.arange(8 * 14 * 14, dtype=torch.float64).reshape(8, 14, 14)
    (tmp_path / "sample_starts.npy").write_bytes(b"stale")
    bench.dump_outputs(torch, str(tmp_path), rows, jac)
    assert sorted(os.listdir(tmp_path)) == ["jacobians.npy", "residual_rows.npy"]
    assert np.array_equal(np.load(tmp_path / "residual_rows.npy"), rows.numpy())
    assert np.array_equal(np.load(tmp_path / "jacobians.npy"), jac.numpy())


def test_dump_outputs_samples_the_same_starts_under_the_limit(tmp_path):
    import torch
    import bench
    P = 24000                                                       # 24000 x 3248 B = 78 MB of outputs
    rows = torch.arange(P, dtype=torch.float64)[:, None, None].expand(P, 15, 14).contiguous()
    jac = (torch.arange(P, dtype=torch.float64)[:, None, None] + 0.5).expand(P, 14, 14).contiguous()
    for d in ("a", "b"):
        bench.dump_outputs(torch, str(tmp_path / d), rows, jac)
    files = ("jacobians.npy", "residual_rows.npy", "sample_starts.npy")
    assert sorted(os.listdir(tmp_path / "a")) == list(files)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= bench.DUMP_LIMIT_BYTES
    idx = np.load(tmp_path / "a" / "sample_starts.npy")
    assert idx.dtype == np.float64 and np.all(np.diff(idx) > 0) and 0 <= idx[0] and idx[-1] < P and len(idx) > 0.7 * P
    r, j = np.load(tmp_path / "a" / "residual_rows.npy"), np.load(tmp_path / "a" / "jacobians.npy")
    assert r.dtype == np.float64 and r.shape == (len(idx), 15, 14) and np.array_equal(r[:, 0, 0], idx)
    assert j.dtype == np.float64 and j.shape == (len(idx), 14, 14) and np.array_equal(j[:, 0, 0], idx + 0.5)
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f
