"""GPU: activation dropout through the engine and the model classes (config.activation_dropout; a run-time setting of the handle).

1. Oracle parity of a training step: the masks the engine drew are read back per site (kmb_activation_dropout_site -> kmb_op_dropout_mask)
   and the oracle's F.dropout is replaced, inside the test, by one that applies them in call order (encoder layers, then decoder layers).
2. Determinism per (seed, step); eval forwards, generate() and score() do not depend on the value.
3. The existing dropout sites draw the masks they drew before: the attention sites report the same seeds and the embedding sites
   (numbers 1 and 2) the same zero pattern whether activation dropout is on or not.
4. dropout = attention_dropout = activation_dropout = 0.1 (facebook/bart-base): the conditional-generation, the pre-training and the
   bare model train; the fine-tuning driver runs with --activation_dropout.
"""
import json
import math
import os
import re
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import goldenlib as G  # noqa: E402
from oracle import kmbart_oracle as O  # noqa: E402
from oracle.make_golden import tiny_batch  # noqa: E402  (batch builder only)
from src.model import MultiModalBartForPreTraining, MultiModalBartModel  # noqa: E402
from kmbart.optim import AdamW  # noqa: E402
from gpu_util import dropout_mask  # noqa: E402
from test_attention_dropout_model_gpu import (DEV, GRAD_TOL, LOSS_TOL, RAGGED4, ROOT, _splitmix, build, cfg_from_oracle,  # noqa: E402
                                              grads_of, rel, run_fwd, same_gradients)
from test_attention_dropout_model_gpu import site_seeds as attn_site_seeds  # noqa: E402

P_ACT = 0.1
THR16 = int(round(P_ACT * 65536))
SCALE = 1.0 / (1.0 - THR16 / 65536.0)


def site_list(ocfg):
    """(kind, layer) in the order the oracle calls its activation dropout: encoder layers, then decoder layers"""
    return [(0, l) for l in range(ocfg.encoder_layers)] + [(1, l) for l in range(ocfg.decoder_layers)]


def site_seeds(eng, ocfg):
    return [eng.activation_dropout_site(kind, l) for kind, l in site_list(ocfg)]


def test_training_step_matches_the_oracle_under_the_exported_masks(monkeypatch):
    ocfg = G.tiny_config(activation_dropout=P_ACT)   # dropout = attention_dropout = 0: the activation masks are the only ones
    sd = G.golden_state_dict(ocfg, seed=21)
    b = tiny_batch(seed=31, **RAGGED4)
    model = build(ocfg, sd).train()
    eng = model._engine
    assert eng.activation_dropout == P_ACT
    eng.set_seed(777)
    loss = run_fwd(model, b)[0]
    loss.backward()
    got = grads_of(model)
    B, S = b["input_ids"].shape
    T = b["decoder_input_ids"].shape[1]
    masks = []
    for (kind, l), (thr, seed) in zip(site_list(ocfg), site_seeds(eng, ocfg)):
        assert thr == THR16, (kind, l, thr)
        rows, F_ = ((B * S, ocfg.encoder_ffn_dim), (B * T, ocfg.decoder_ffn_dim))[kind]
        masks.append(dropout_mask(seed, thr / 65536.0, rows, F_).view(B, rows // B, F_).cpu())
    assert len({seed for _, seed in site_seeds(eng, ocfg)}) == len(masks), "every site draws its own seed"
    pending = iter(masks)
    used = []

    def masked_dropout(x, p=0.5, training=True, inplace=False):
        if not training or p == 0.0:   # the hidden / attention dropout calls of this configuration
            return x
        m = next(pending)
        assert tuple(x.shape) == tuple(m.shape), (tuple(x.shape), tuple(m.shape))
        assert p == P_ACT
        used.append(m)
        return x * (m.to(x.dtype) * SCALE)

    monkeypatch.setattr(O.F, "dropout", masked_dropout)
    osd = {k: v.clone().requires_grad_(k != "final_logits_bias") for k, v in sd.items()}
    ref_loss = O.forward(osd, ocfg, b["input_ids"], b["image_features"], b["attention_mask"], b["decoder_input_ids"],
                         b["decoder_attention_mask"], b["labels"], training=True)[0]
    ref_loss.backward()
    monkeypatch.undo()
    assert len(used) == len(masks) and next(pending, None) is None
    d_loss = abs(float(loss) - float(ref_loss)) / float(ref_loss)
    print(f"activation dropout {P_ACT}: loss {float(loss):.6f} vs oracle {float(ref_loss):.6f} (rel {d_loss:.2e})")
    assert d_loss < LOSS_TOL
    worst = ("", 0.0)
    for n, g in got.items():
        r = osd[n].grad
        if float(r.norm()) < 1e-6:   # k_proj.bias: softmax is shift-invariant, the true gradient is zero
            assert float(g.norm()) < 1e-2, n
            continue
        e = rel(g, r)
        if e > worst[1]:
            worst = (n, e)
    print(f"activation dropout {P_ACT}: worst gradient error {worst[1]:.3e} ({worst[0]})")
    assert worst[1] < GRAD_TOL, worst
    # the loss really is a dropped one: the eval loss of the same weights differs
    assert float(run_fwd(model.eval(), b)[0]) != float(loss)


def test_determinism_per_seed_and_step_and_eval_independence():
    ocfg = G.tiny_config(activation_dropout=P_ACT)
    sd = G.trained_state_dict()
    b = tiny_batch(seed=41, **RAGGED4)
    model = build(ocfg, sd).train()
    eng = model._engine
    outs = []
    for _ in range(2):
        eng.set_seed(123)
        loss = run_fwd(model, b)[0]
        loss.backward()
        outs.append((loss.detach().clone(), grads_of(model), site_seeds(eng, ocfg)))
    assert torch.equal(outs[0][0], outs[1][0]) and outs[0][2] == outs[1][2]
    n_rows = b["input_ids"].numel() + b["decoder_input_ids"].numel()
    assert not same_gradients(outs[0][1], outs[1][1], n_rows)
    assert math.isfinite(float(outs[0][0])) and all(bool(torch.isfinite(g).all()) for g in outs[0][1].values())
    eng.set_seed(124)
    other = float(run_fwd(model, b)[0])
    assert other != float(outs[0][0]) and site_seeds(eng, ocfg) != outs[0][2]
    # the next step of the same seed draws new masks
    eng.set_seed(123)
    opt = AdamW(model.parameters(), lr=1e-4)
    loss = run_fwd(model, b)[0]
    opt.zero_grad()
    loss.backward()
    opt.step()
    first = site_seeds(eng, ocfg)
    assert first == outs[0][2]
    run_fwd(model, b)[0].backward()
    second = site_seeds(eng, ocfg)
    assert all(a[0] == THR16 and c[0] == THR16 and a[1] != c[1] for a, c in zip(first, second)), (first, second)
    # an eval forward draws nothing and leaves the record of the last TRAINING forward alone
    with torch.no_grad():
        run_fwd(model.eval(), b)
    assert site_seeds(eng, ocfg) == second
    # a training forward with the setting at 0 records zeros
    eng.set_activation_dropout(0.0)
    run_fwd(model.train(), b)[0].backward()
    assert site_seeds(eng, ocfg) == [(0, 0)] * len(second)

    # ---- eval, generate and score: bit-identical to a model built with activation_dropout = 0 on the same weights
    plain = build(G.tiny_config(), sd).eval()
    drop = build(ocfg, sd).eval()
    assert drop._engine.activation_dropout == P_ACT and plain._engine.activation_dropout == 0.0
    feats = [f.to(DEV) for f in b["image_features"]]
    res = []
    for m in (plain, drop):
        with torch.no_grad():
            loss, logits = run_fwd(m, b, return_logits=True)[:2]
            ids = m.generate(input_ids=b["input_ids"].to(DEV), image_features=feats, attention_mask=b["attention_mask"].to(DEV),
                             num_beams=3, max_length=10, early_stopping=True)
            sc = m.score(input_ids=b["input_ids"].to(DEV), image_features=feats, attention_mask=b["attention_mask"].to(DEV),
                         decoder_input_ids=b["decoder_input_ids"].to(DEV), decoder_attention_mask=b["decoder_attention_mask"].to(DEV),
                         labels=b["labels"].to(DEV))
        torch.cuda.synchronize()
        res.append((loss.clone(), logits.clone(), ids.clone(), sc.token_logprobs.clone(), sc.nll.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert torch.equal(res[0][2], res[1][2])
    assert torch.equal(res[0][3], res[1][3]) and torch.equal(res[0][4], res[1][4])


def test_existing_dropout_sites_keep_their_masks():
    """dropout = attention_dropout = 0.1 with activation dropout on and off: the attention sites report the same seeds, and the
    embedding sites (numbers 1 and 2, seed splitmix(seed ^ splitmix(step * 0x10001 + site)) as ever) drop exactly the elements
    they drop without it."""
    sd = G.golden_state_dict(G.tiny_config(), seed=21)
    b = tiny_batch(seed=31, **RAGGED4)
    seed, step = 4242, 1
    states, losses, attn = [], [], []
    for p_act in (P_ACT, 0.0, P_ACT):
        ocfg = G.tiny_config(dropout=0.1, attention_dropout=0.1, activation_dropout=p_act)
        model = build(ocfg, sd).train()
        model._engine.set_seed(seed)
        loss = run_fwd(model, b)[0]
        enc0, dec0 = model._engine.hidden_states(0)[0].clone(), model._engine.hidden_states(1)[0].clone()
        loss.backward()
        g = grads_of(model)
        assert math.isfinite(float(loss)) and all(bool(torch.isfinite(x).all()) for x in g.values())
        states.append((enc0, dec0, g))
        losses.append(float(loss))
        attn.append(attn_site_seeds(model._engine, ocfg))
        assert all(thr == (THR16 if p_act else 0) for thr, _ in site_seeds(model._engine, ocfg))
    assert losses[0] == losses[2]                                                                                # deterministic
    assert not same_gradients(states[0][2], states[2][2], b["input_ids"].numel() + b["decoder_input_ids"].numel())
    assert losses[0] != losses[1]                                                                                # and really dropped
    assert attn[0] == attn[1] == attn[2] and all(thr == THR16 for thr, _ in attn[0])
    # the embedding outputs precede every FFN: the same bits with and without activation dropout
    assert torch.equal(states[0][0], states[1][0]) and torch.equal(states[0][1], states[1][1])
    d = 128
    for site, x in ((1, states[0][0]), (2, states[0][1])):
        site_seed = _splitmix(seed ^ _splitmix(step * 0x10001 + site)) & 0xffffffff
        rows = x.numel() // d
        keep = dropout_mask(site_seed, 0.1, rows, d)
        x2 = x.reshape(rows, d)
        assert bool((x2[~keep] == 0).all()), site
        assert float((x2[keep] == 0).float().mean()) < 1e-3, site   # (a kept LayerNorm output is zero only by accident)
    # the activation sites' seeds are the documented ones
    model = build(G.tiny_config(dropout=0.1, attention_dropout=0.1, activation_dropout=P_ACT), sd).train()
    model._engine.set_seed(seed)
    run_fwd(model, b)[0].backward()
    for (kind, l), (thr, s) in zip(site_list(G.tiny_config()), site_seeds(model._engine, G.tiny_config())):
        assert s == _splitmix(seed ^ _splitmix(step * 0x10001 + 0x60000000 + 2 * l + kind)) & 0xffffffff, (kind, l)


BART_BASE = dict(dropout=0.1, attention_dropout=0.1, activation_dropout=P_ACT)


def _two_steps(model, fwd):
    """two optimizer steps; ([loss per step], gradients of the second step)"""
    opt = AdamW(model.parameters(), lr=1e-4)
    model._engine.set_seed(5)
    losses = []
    for _ in range(2):
        loss = fwd(model)
        opt.zero_grad()
        loss.backward()
        g = grads_of(model)
        opt.step()
        losses.append(float(loss))
    return losses, g


def test_all_three_probabilities_train_every_model_class():
    # ---- the conditional-generation model
    sd = G.golden_state_dict(G.tiny_config(), seed=21)
    b = tiny_batch(seed=31, **RAGGED4)
    runs = {}
    for name, over in (("all", BART_BASE), ("no_act", dict(BART_BASE, activation_dropout=0.0))):
        model = build(G.tiny_config(**over), sd).train()
        runs[name] = _two_steps(model, lambda m: run_fwd(m, b)[0])
        assert all(math.isfinite(x) for x in runs[name][0])
        assert all(g is not None and bool(torch.isfinite(g).all()) for g in runs[name][1].values())
    assert all(a != c for a, c in zip(runs["all"][0], runs["no_act"][0])), runs

    # ---- the pre-training model, all heads
    from src.data.synthetic import make_pretrain_batch
    kw = dict(num_labels=37, num_attributes=11, num_relations=9, lm_loss_factor=5.0, mrm_loss_factor=1.0, attribute_loss_factor=2.0,
              relation_loss_factor=0.5)
    ocfg = G.tiny_config(**BART_BASE, **kw)
    psd = G.golden_state_dict(ocfg, seed=33)
    pb = make_pretrain_batch(3, enc_len=24, dec_len=16, num_regions=6, seed=77, num_labels=37, num_attributes=11, num_relations=9,
                             vocab_hi=G.TINY_SPECIAL_BASE, img_feat_id=ocfg.img_feat_id, special_base=G.TINY_SPECIAL_BASE,
                             cls_id=ocfg.cls_token_id, mrm_probability=0.3)
    pb["image_features"] = G.golden_features([6, 6, 6])
    terms = ("loss", "lm_loss", "mrm_loss", "attribute_loss", "relation_loss")
    seen = {}

    def pre_fwd(m):
        out = m(input_ids=pb["input_ids"].to(DEV), image_features=[f.to(DEV) for f in pb["image_features"]],
                attention_mask=pb["attention_mask"].to(DEV), decoder_input_ids=pb["decoder_input_ids"].to(DEV),
                decoder_attention_mask=pb["decoder_attention_mask"].to(DEV), labels=pb["labels"].to(DEV), mrm_labels=pb["mrm_labels"],
                mrm_mask=pb["mrm_mask"], attribute_labels=pb["attribute_labels"], attribute_mask=pb["attribute_mask"],
                relation_labels=pb["relation_labels"])[0]
        assert all(math.isfinite(float(out[k])) for k in terms)
        return out["loss"]

    for name, over in (("all", BART_BASE), ("no_act", dict(BART_BASE, activation_dropout=0.0))):
        model = build(G.tiny_config(**over, **kw), psd, cls=MultiModalBartForPreTraining, **kw).train()
        seen[name] = _two_steps(model, pre_fwd)
        assert all(math.isfinite(x) for x in seen[name][0])
        assert all(g is not None and bool(torch.isfinite(g).all()) for g in seen[name][1].values())
        if name == "all":
            assert all(thr == THR16 for thr, _ in site_seeds(model._engine, ocfg))
    assert all(a != c for a, c in zip(seen["all"][0], seen["no_act"][0])), seen

    # ---- the bare model (no head, no loss, hence no backward): two training forwards, finite and unlike the run without
    vb = tiny_batch(seed=41, **RAGGED4)
    args = dict(input_ids=vb["input_ids"].to(DEV), image_features=[f.to(DEV) for f in vb["image_features"]],
                attention_mask=vb["attention_mask"].to(DEV), decoder_input_ids=vb["decoder_input_ids"].to(DEV),
                decoder_attention_mask=vb["decoder_attention_mask"].to(DEV))
    bare = {}
    for name, over in (("all", BART_BASE), ("no_act", dict(BART_BASE, activation_dropout=0.0))):
        torch.manual_seed(0)
        m = MultiModalBartModel(cfg_from_oracle(G.tiny_config(**over)))
        m.to(DEV).train()
        m._engine.set_seed(5)
        vals = []
        for _ in range(2):
            with torch.no_grad():
                dec = m(**args)[0]
            vals.append(dec.float().clone())
            assert bool(torch.isfinite(vals[-1]).all())
        bare[name] = vals
        assert all(thr == (THR16 if name == "all" else 0) for thr, _ in site_seeds(m._engine, G.tiny_config()))
    assert all(not torch.equal(a, c) for a, c in zip(bare["all"], bare["no_act"]))


def test_fine_tuning_driver_runs_with_activation_dropout(tmp_path):
    """vcg_train.py --synthetic ... --activation_dropout 0.1 on a two-layer d = 128 configuration (the synthetic batches carry the full
    vocabulary's ids): the flag reaches the engine and every logged loss is finite."""
    cfg = dict(vocab_size=50320, d_model=128, encoder_layers=2, decoder_layers=2, encoder_attention_heads=2, decoder_attention_heads=2,
               encoder_ffn_dim=256, decoder_ffn_dim=256, max_position_embeddings=128, dropout=0.1, attention_dropout=0.0,
               activation_dropout=0.0, init_std=0.02)
    (tmp_path / "tiny.json").write_text(json.dumps(cfg))
    cmd = [sys.executable, os.path.join(ROOT, "km-bart_amd", "vcg_train.py"), "--model_config", str(tmp_path / "tiny.json"),
           "--checkpoint_dir", str(tmp_path / "ckpt"), "--synthetic", "3", "--epochs", "1", "--batch_size", "4", "--activation_dropout", "0.1"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    losses = [float(x) for x in re.findall(r"Loss: ([-+.\w]+)", r.stdout)]
    assert len(losses) == 3 and all(math.isfinite(x) and 0.0 < x < 20.0 for x in losses), r.stdout[-1500:]
    saved = json.load(open(tmp_path / "ckpt" / "epoch1" / "config.json"))
    assert saved["activation_dropout"] == 0.1
