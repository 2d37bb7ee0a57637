"""bench.py's command line and output dump (CPU only): --full is off by default, --steps sets the timed steps, and
--dump-outputs writes float32 .npy files inside its byte budget, the same files for the same arrays."""
import os
import sys

import numpy as np
import torch

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    return bench.parse()


def test_plain_run_is_the_default(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "3")
    assert (a.full, a.dump_outputs, a.steps, a.warmup, a.config) == (False, None, 7, 3, 3)
    a = _parse(monkeypatch, "--full", "--dump-outputs", "somewhere")
    assert a.full and a.dump_outputs == "somewhere" and a.steps == bench.CONFIGS[3]["steps"]


def test_dump_outputs_small_arrays_whole(tmp_path):
    arrays = {"obs": torch.arange(24, dtype=torch.float32).reshape(2, 3, 4), "done": torch.tensor([True, False]),
              "nn_idx": torch.arange(6, dtype=torch.int64).reshape(2, 3), "loss": torch.tensor(0.5)}
    m = bench.dump_outputs(str(tmp_path), arrays)
    assert sorted(os.listdir(tmp_path)) == sorted(n + ".npy" for n in arrays)
    for n, t in arrays.items():
        a = np.load(tmp_path / (n + ".npy"))
        assert a.dtype == np.float32 and a.shape == tuple(t.shape) and m[n]["sampled"] is None
        np.testing.assert_array_equal(a, t.to(torch.float32).numpy())


def test_dump_outputs_budget_and_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4 * 1000)
    g = torch.Generator().manual_seed(0)
    arrays = {"small": torch.rand(100, generator=g), "big": torch.rand(70, 50, generator=g),
              "bigger": torch.rand(9001, generator=g), "mid": torch.rand(300, generator=g)}
    m1 = bench.dump_outputs(str(tmp_path / "a"), arrays)
    m2 = bench.dump_outputs(str(tmp_path / "b"), arrays)
    assert m1 == m2
    # water-filling: 100 + 300 whole, the two large arrays share the remaining 600 elements
    assert [m1[n]["sampled"] for n in ("small", "mid", "big", "bigger")] == [None, None, 300, 300]
    total = 0
    for n, t in arrays.items():
        a, b = np.load(tmp_path / "a" / (n + ".npy")), np.load(tmp_path / "b" / (n + ".npy"))
        np.testing.assert_array_equal(a, b)
        assert a.dtype == np.float32
        total += a.nbytes
        if m1[n]["sampled"] is not None:  # values of the source, in flat-index order
            src = t.reshape(-1).numpy()
            assert a.shape == (m1[n]["sampled"],) and np.isin(a, src).all()
    assert total <= 4 * 1000
