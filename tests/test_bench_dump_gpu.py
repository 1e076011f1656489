"""GPU: `bench.py --dump-outputs DIR` -- exactly --steps timed steps, and what the last one computed (loss, updated parameters,
gradients; float .npy files under 64 MB) comes out the same from two runs with the same arguments (the inputs and initial
weights are seeded; the step is bit-reproducible except the tied embedding gradient's fp32 atomics)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

ARGS = ["--gpus", "1", "--batch", "16", "--steps", "4", "--warmup", "1", "--no-extras", "--no-roofline", "--no-cpu-baseline",
        "--no-pcie"]


def _run(out_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + ARGS + ["--dump-outputs", out_dir], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _rel(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b) / (np.linalg.norm(b.astype(np.float64)) + 1e-30))


def test_dump_outputs_repeat(tmp_path):
    outs = [_run(str(tmp_path / d)) for d in ("a", "b")]
    for out in outs:
        assert out["steps"] == 4 and out["windows"] == 3 and out["ms_per_step"] > 0
        assert len(out["ms_per_step_windows"]) == 3 and out["dump_outputs"]["names"] == ["grads_sample", "loss", "params_sample"]
    arrays = [{n: np.load(tmp_path / d / (n + ".npy")) for n in outs[0]["dump_outputs"]["names"]} for d in ("a", "b")]
    total = sum(a.nbytes for a in arrays[0].values())
    assert total <= 64 << 20 and all(a.dtype in (np.float32, np.float64) for a in arrays[0].values())
    a, b = arrays
    assert a["loss"].shape == (1,) and abs(float(a["loss"][0]) - outs[0]["final_loss"]) < 1e-4   # the last timed step's loss
    assert np.isfinite(a["params_sample"]).all() and np.isfinite(a["grads_sample"]).all()
    assert np.abs(a["grads_sample"]).max() > 0
    dl = abs(float(a["loss"][0]) - float(b["loss"][0])) / abs(float(b["loss"][0]))
    dp, dg = _rel(a["params_sample"], b["params_sample"]), _rel(a["grads_sample"], b["grads_sample"])
    print("run-to-run: loss rel %.2e, params rel %.2e, grads rel %.2e" % (dl, dp, dg))
    assert dl < 1e-6 and dp < 1e-7 and dg < 1e-5   # measured: loss bit-equal, params 2e-14 (b = 16) / 6e-11 (b = 1024), grads 8e-10 / 2e-9
