"""CPU: bench.py's command line and its --dump-outputs writer (the GPU side of both: tests/test_tools_gpu.py)."""
import os
import sys

import numpy as np
import pytest
import torch

import bench


def test_plain_run_is_the_default_and_steps_are_taken_as_given(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.gpus, a.steps, a.warmup, a.full, a.dump_outputs) == (1, 7, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "out"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()


def test_dump_outputs_float32_within_budget_and_a_fixed_sample(tmp_path):
    small = torch.arange(12, dtype=torch.float64).reshape(3, 4)
    big = torch.randn(17_000_000, generator=torch.Generator().manual_seed(3))          # 68 MB as float32: over the budget
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    assert sorted(os.listdir(tmp_path / "a")) == ["big_sample.npy", "small.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= bench.DUMP_BUDGET_BYTES
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float32 and s.shape == (3, 4) and np.array_equal(s, small.float().numpy())
    got = np.load(tmp_path / "a" / "big_sample.npy")
    assert got.dtype == np.float32 and got.ndim == 1 and got.size > 15_000_000
    assert np.array_equal(got, np.load(tmp_path / "b" / "big_sample.npy"))             # the same positions every run
    idx = torch.randint(0, big.numel(), (got.size,), generator=torch.Generator().manual_seed(0)).sort().values
    assert np.array_equal(got, big[idx].numpy())
