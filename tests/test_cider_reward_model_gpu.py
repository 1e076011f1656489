"""GPU: the CIDEr-D reward on the device through src.training.self_critical_step on the trained tiny fixture -- info["rewards"] and
the greedy baseline equal the table-side restatement (tests/cider_ref.py) on info["sample_ids"] / info["greedy_ids"] within the
kernel's bound, the loss is finite and backward() runs -- and the fine-tuning driver with --self_critical on synthetic batches."""
import json
import math
import os
import random
import re
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "km-bart_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import goldenlib as G  # noqa: E402
import cider_ref as R  # noqa: E402
from src.rewards import CiderReward, reward_tokens  # noqa: E402
from src.training import self_critical_step  # noqa: E402
from test_model_gpu import build  # noqa: E402

DEV = "cuda:0"


def test_self_critical_step_with_the_device_reward(gold_dir):
    gen = json.load(open(os.path.join(gold_dir, "tiny_generate.json")))
    ocfg, sd = G.tiny_config(), G.trained_state_dict()
    pad, bos, eos = ocfg.pad_token_id, ocfg.bos_token_id, ocfg.eos_token_id
    model = build(ocfg, sd).eval()
    B = len(gen["input_ids"])
    # references: what the fixture's greedy decode says for the row, and two edited copies of it
    rng = random.Random(2)
    words = list(range(10, 80))
    groups = []
    for row in gen["cases"][0]["ids"]:
        t = reward_tokens(row, pad, bos, eos)
        assert len(t) >= 2
        groups.append([t, R.edit(t, rng, words), R.edit(R.edit(t, rng, words), rng, words)])
    assert len(groups) == B
    keys = [(50 + b, "intent") for b in range(B)]
    rew = CiderReward(groups, ocfg.vocab_size, pad, bos, eos, device=DEV, group_keys=keys)
    tab = R.TableReference(rew.tables)
    batch = dict(input_ids=torch.tensor(gen["input_ids"]), attention_mask=torch.tensor(gen["attention_mask"]),
                 image_features=G.golden_features(gen["regions"], seed=gen["seed"]), index=[k[0] for k in keys],
                 task_type=[k[1] for k in keys])
    torch.manual_seed(12)
    loss, info = self_critical_step(model, batch, rew.for_batch(batch), DEV, baseline="greedy",
                                    sample_kwargs=dict(max_length=12, min_length=0, temperature=1.5))
    for ids, got, what in ((info["sample_ids"], info["rewards"], "sample"), (info["greedy_ids"], info["baseline"], "greedy")):
        assert got.dtype == torch.float32 and got.device.type == "cuda" and got.shape == (B,)
        rows, got = ids.cpu().tolist(), got.double().cpu().tolist()
        for b in range(B):
            t = reward_tokens(rows[b], pad, bos, eos)
            want = tab.score(t, b, "D")
            assert abs(got[b] - want) <= R.bound(want, len(t), 3), (what, b, got[b], want)
        print("%s rewards: %s" % (what, ["%.4f" % x for x in got]))
        if what == "greedy":
            assert sum(1 for x in got if x > 1.0) >= B // 2, "the greedy decode of the trained fixture should resemble its references"
    assert torch.equal(info["advantages"], info["rewards"] - info["baseline"])
    assert math.isfinite(float(loss.detach()))
    loss.backward()
    torch.cuda.synchronize()
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert grads and all(bool(torch.isfinite(g).all()) for g in grads)


def test_fine_tuning_driver_self_critical(tmp_path):
    """vcg_train.py --synthetic 8 --self_critical --epochs 1 on a two-layer d = 128 configuration: exits 0, every step logs a finite loss,
    the batch's mean reward (>= 0) and its mean advantage in fine_tune's line."""
    cfg = dict(vocab_size=50320, d_model=128, encoder_layers=2, decoder_layers=2, encoder_attention_heads=2, decoder_attention_heads=2,
               encoder_ffn_dim=256, decoder_ffn_dim=256, max_position_embeddings=128, dropout=0.1, attention_dropout=0.0,
               activation_dropout=0.0, init_std=0.02)
    (tmp_path / "tiny.json").write_text(json.dumps(cfg))
    cmd = [sys.executable, os.path.join(ROOT, "km-bart_amd", "vcg_train.py"), "--model_config", str(tmp_path / "tiny.json"),
           "--checkpoint_dir", str(tmp_path / "ckpt"), "--synthetic", "8", "--self_critical", "--epochs", "1", "--batch_size", "4",
           "--sc_max_length", "12"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    lines = re.findall(r"Epoch \[1/1\], Step \[(\d)/8\], Loss: ([-+.\w]+), Reward: ([-+.\w]+), Advantage: ([-+.\w]+), ETA: ", r.stdout)
    assert [int(x[0]) for x in lines] == list(range(1, 9)), r.stdout[-1500:]
    assert all(math.isfinite(float(v)) for x in lines for v in x[1:]) and all(float(x[2]) >= 0.0 for x in lines)
    assert "Self-critical training: cider_d over token ids, 4 items, 32 references" in r.stdout
    assert os.path.isdir(str(tmp_path / "ckpt" / "epoch1"))
