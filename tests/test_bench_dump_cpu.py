"""CPU: bench.py's bookkeeping of the timed steps and of --dump-outputs (no GPU: the arena is a host tensor here)."""
import types

import numpy as np
import torch

import bench


def test_window_sizes_add_up_to_steps():
    for steps in (1, 2, 3, 5, 20, 61):
        for windows in (1, 3, 7):
            w = bench.window_sizes(steps, windows)
            assert sum(w) == steps and len(w) == min(steps, windows) and min(w) >= 1 and max(w) - min(w) <= 1


def _fake_model(n):
    """An arena whose values are their own positions (exact in float32 below 2**24): the dump tells where it sampled."""
    pos = torch.arange(n, dtype=torch.float32)
    return types.SimpleNamespace(_engine=types.SimpleNamespace(params=pos, grads=-2.0 * pos))


def test_dump_outputs_is_a_fixed_float_sample(tmp_path):
    n = 3 * bench.DUMP_SAMPLE
    assert n < 1 << 24
    names = bench.dump_outputs(str(tmp_path / "a"), _fake_model(n), torch.tensor([2.5]))
    bench.dump_outputs(str(tmp_path / "b"), _fake_model(n), torch.tensor([2.5]))
    assert names == ["grads_sample", "loss", "params_sample"]
    total = 0
    for name in names:
        a, b = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b)   # same inputs -> same files
        total += a.nbytes
    assert total <= 64 << 20
    assert np.load(tmp_path / "a" / "loss.npy").tolist() == [2.5]
    p = np.load(tmp_path / "a" / "params_sample.npy")
    assert p.shape == (bench.DUMP_SAMPLE,) and p.min() >= 0 and p.max() < n
    assert np.all(np.diff(p) >= 0) and p.max() - p.min() > n * 0.9            # sorted positions over the whole arena
    # parameters and gradients are sampled at the same positions
    assert np.array_equal(np.load(tmp_path / "a" / "grads_sample.npy"), -2.0 * p)


def test_small_arena_is_sampled_within_bounds(tmp_path):
    bench.dump_outputs(str(tmp_path), _fake_model(1000), torch.tensor([1.0]))
    p = np.load(tmp_path / "params_sample.npy")
    assert p.shape == (1000,) and p.min() >= 0 and p.max() <= 999
