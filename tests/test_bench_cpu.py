"""Host-side checks of bench.py's command line (no GPU needed)."""
import os
import subprocess
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_refuses_a_rank_count_that_differs_from_gpus():
    repo = REPO
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"], env=env,
                       capture_output=True, text=True, timeout=300, cwd=repo)
    assert r.returncode != 0 and "WORLD_SIZE=1" in (r.stderr + r.stdout)


def test_bench_config_presets(monkeypatch):
    sys.path.insert(0, REPO)
    import bench

    for name, want in (("o96", ("o96", 5, "gt")), ("o96-res6", ("o96", 6, "gt")), ("n320", ("n320", 6, "gt")), ("gnn", ("o96", 5, "gnn"))):
        monkeypatch.setattr(sys, "argv", ["bench.py", "--config", name])
        a = bench.parse()
        assert (a.data_grid, a.hidden_res, a.kind) == want and a.gpus == 1 and a.layers == 16 and a.channels == 512
    monkeypatch.setattr(sys, "argv", ["bench.py", "--config", "n320", "--hidden-res", "5"])  # explicit flags win
    assert bench.parse().hidden_res == 5


def test_bench_refuses_zero_timed_steps(monkeypatch):
    sys.path.insert(0, REPO)
    import bench

    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "7", "--warmup", "0", "--dump-outputs", "out", "--full"])
    a = bench.parse()
    assert a.steps == 7 and a.warmup == 0 and a.dump_outputs == "out" and a.full


def test_dump_outputs_writes_float32_and_samples_large_outputs_the_same_way(tmp_path):
    """--dump-outputs: an output under the limit is written whole; a larger one as the same seeded, grid-ordered sample of grid
    points every time, under 64 MB."""
    import numpy as np

    sys.path.insert(0, REPO)
    import bench

    small = torch.randn(1, 1, 1, 100, 3, dtype=torch.bfloat16)
    bench.dump_outputs({"data": small}, str(tmp_path / "small"))
    a = np.load(tmp_path / "small" / "data.npy")
    assert a.dtype == np.float32 and np.array_equal(a, small.float().numpy())

    rows, V = bench.DUMP_LIMIT_BYTES // (4 * 84) + 1000, 84
    big = torch.arange(rows, dtype=torch.float32).view(1, 1, 1, rows, 1).expand(1, 1, 1, rows, V).contiguous()
    for d in ("big0", "big1"):
        bench.dump_outputs({"data": big}, str(tmp_path / d))
    b0, b1 = np.load(tmp_path / "big0" / "data.npy"), np.load(tmp_path / "big1" / "data.npy")
    assert np.array_equal(b0, b1) and b0.dtype == np.float32
    assert os.path.getsize(tmp_path / "big0" / "data.npy") < 64e6 and b0.shape[:3] == (1, 1, 1) and b0.shape[4] == V
    picked = b0[0, 0, 0, :, 0]
    assert 0 < len(picked) < rows and np.all(np.diff(picked) > 0) and np.all(b0[0, 0, 0] == picked[:, None])
