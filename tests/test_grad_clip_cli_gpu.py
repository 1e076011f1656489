"""GPU: the fine-tuning driver with --max_grad_norm / --skip_nonfinite, end to end on synthetic batches."""
import json
import math
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_fine_tuning_driver_clips_and_logs_the_norm(tmp_path):
    """vcg_train.py --synthetic 3 --max_grad_norm 0.5 --skip_nonfinite on a two-layer d = 128 configuration (the synthetic batches carry the
    full vocabulary's ids): every logged loss is finite, each logged step is followed by ONE additional line with the gradient norm and
    the skipped-step count, and the existing loss line keeps its form."""
    cfg = dict(vocab_size=50320, d_model=128, encoder_layers=2, decoder_layers=2, encoder_attention_heads=2, decoder_attention_heads=2,
               encoder_ffn_dim=256, decoder_ffn_dim=256, max_position_embeddings=128, dropout=0.1, attention_dropout=0.0,
               activation_dropout=0.0, init_std=0.02)
    (tmp_path / "tiny.json").write_text(json.dumps(cfg))
    cmd = [sys.executable, os.path.join(ROOT, "km-bart_amd", "vcg_train.py"), "--model_config", str(tmp_path / "tiny.json"),
           "--checkpoint_dir", str(tmp_path / "ckpt"), "--synthetic", "3", "--epochs", "1", "--batch_size", "4",
           "--max_grad_norm", "0.5", "--skip_nonfinite"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    losses = [float(x) for x in re.findall(r"Epoch \[1/1\], Step \[\d/3\], Loss: ([-+.\w]+), ETA: ", r.stdout)]
    assert len(losses) == 3 and all(math.isfinite(x) and 0.0 < x < 20.0 for x in losses), r.stdout[-1500:]
    norms = re.findall(r"Epoch \[1/1\], Step \[(\d)/3\], Grad norm: ([-+.\w]+), Skipped steps: (\d+)", r.stdout)
    assert [int(s) for s, _, _ in norms] == [1, 2, 3], r.stdout[-1500:]
    assert all(math.isfinite(float(n)) and float(n) > 0.0 for _, n, _ in norms) and all(k == "0" for _, _, k in norms)
    # the checkpoint carries the device's count of applied steps
    import torch
    td = torch.load(str(tmp_path / "ckpt" / "epoch1" / "training_data.pt"), map_location="cpu", weights_only=False)
    assert td["optimizer"]["step"] == [3]
