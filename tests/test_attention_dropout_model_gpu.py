"""GPU: attention dropout through the engine and the model classes (config.attention_dropout; a run-time setting of the handle).

1. Oracle parity of a training step: the masks the engine drew are read back per site (kmb_attention_dropout_site -> kmb_op_dropout_mask)
   and the oracle's F.dropout is replaced, inside the test, by one that applies them in call order.
2. Determinism per (seed, step); eval forwards, generate() and score() do not depend on the value.
3. The existing dropout sites draw the masks they drew before: the encoder embedding's mask, exported through the seed the engine has
   always derived for site 1, is the zero pattern of the embedding output whether attention dropout is on or not.
4. The pre-training model, the bare model and the fine-tuning driver run with it.
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
from src.model import (MultiModalBartConfig, MultiModalBartForConditionalGeneration, MultiModalBartForPreTraining,  # noqa: E402
                       MultiModalBartModel)
from kmbart.optim import AdamW  # noqa: E402
from gpu_util import dropout_mask  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
LOSS_TOL = 1e-3   # relative: the project's loss bound (tests/test_model_gpu.py)
GRAD_TOL = 3e-2   # norm-wise, per parameter: the tiny-config bound (tests/test_model_gpu.py)
P_ATTN = 0.1
THR16 = int(round(P_ATTN * 65536))
SCALE = 1.0 / (1.0 - THR16 / 65536.0)
RAGGED4 = dict(regions=(6, 3, 0, 5), event_lens=(8, 4, 9, 6), label_lens=(12, 7, 9, 5))


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def cfg_from_oracle(ocfg, **over):
    keys = ("vocab_size", "d_model", "encoder_layers", "decoder_layers", "encoder_attention_heads",
            "decoder_attention_heads", "encoder_ffn_dim", "decoder_ffn_dim", "max_position_embeddings",
            "image_feature_size", "img_feat_id", "cls_token_id", "dropout", "attention_dropout",
            "activation_dropout", "init_std")
    d = {k: getattr(ocfg, k) for k in keys}
    d.update(over)
    return MultiModalBartConfig.from_dict(d)


def build(ocfg, sd, cls=MultiModalBartForConditionalGeneration, **over):
    model = cls(cfg_from_oracle(ocfg, **over))
    model.load_state_dict(sd, strict=False)
    model.to(DEV)
    return model


def run_fwd(model, b, **kw):
    return model(input_ids=b["input_ids"].to(DEV), image_features=[f.to(DEV) for f in b["image_features"]],
                 attention_mask=b["attention_mask"].to(DEV), decoder_input_ids=b["decoder_input_ids"].to(DEV),
                 decoder_attention_mask=b["decoder_attention_mask"].to(DEV), labels=b["labels"].to(DEV), **kw)


def grads_of(model):
    torch.cuda.synchronize()
    return {n: p.grad.detach().clone() for n, p in model.named_parameters()}


TIED = "model.shared.weight"


def same_gradients(g0, g1, n_rows):
    """Two backward passes of the same forward.  Every gradient is written once, in a fixed order, and must have the same bits -- except the
    tied matrix's: the head's weight gradient first, then the two embedding scatter-adds as fp32 atomics, whose order the hardware
    picks ("the only run-to-run non-determinism of a step (last bit of model.shared.weight.grad)", with or
    without any dropout).  An element there is a sum of at most 1 + n_rows fp32 terms (n_rows = B * (S + T) embedded tokens); another
    order moves each of its partial sums by at most one fp32 rounding, 2^-24 relative: the tensor must agree within
    (1 + n_rows) * 2^-23 norm-wise.  Returns the list of what does not hold."""
    bad = [n for n in g0 if n != TIED and not torch.equal(g0[n], g1[n])]
    if TIED in g0:
        e = float((g0[TIED].double() - g1[TIED].double()).norm() / g0[TIED].double().norm())
        print(f"{TIED}: run-to-run difference {e:.3e} (< {(1 + n_rows) * 2.0 ** -23:.3e})")
        if not e < (1 + n_rows) * 2.0 ** -23:
            bad.append(f"{TIED} ({e:.3e})")
    return bad


def site_list(ocfg):
    """(kind, layer) in the order the oracle calls its attention dropout: encoder layers, then per decoder layer self then cross"""
    return [(0, l) for l in range(ocfg.encoder_layers)] + [s for l in range(ocfg.decoder_layers) for s in ((1, l), (2, l))]


def site_seeds(eng, ocfg):
    return [eng.attention_dropout_site(kind, l) for kind, l in site_list(ocfg)]


def test_training_step_matches_the_oracle_under_the_exported_masks(monkeypatch):
    ocfg = G.tiny_config(attention_dropout=P_ATTN)   # dropout = 0: the attention masks are the only ones
    sd = G.golden_state_dict(ocfg, seed=21)
    b = tiny_batch(seed=31, **RAGGED4)
    model = build(ocfg, sd).train()
    eng = model._engine
    eng.set_seed(777)
    loss = run_fwd(model, b)[0]
    loss.backward()
    got = grads_of(model)
    B, S = b["input_ids"].shape
    T = b["decoder_input_ids"].shape[1]
    H = ocfg.encoder_attention_heads
    masks = []
    for (kind, l), (thr, seed) in zip(site_list(ocfg), site_seeds(eng, ocfg)):
        assert thr == THR16, (kind, l, thr)
        Tq, Tk = ((S, S), (T, T), (T, S))[kind]
        masks.append(dropout_mask(seed, thr / 65536.0, B * H * Tq, Tk).view(B, H, Tq, Tk).cpu())
    assert len({seed for _, seed in site_seeds(eng, ocfg)}) == len(masks), "every site draws its own seed"
    pending = iter(masks)
    used = []

    def masked_dropout(x, p=0.5, training=True, inplace=False):
        if not training or p == 0.0:   # the hidden / activation dropout calls of this configuration
            return x
        m = next(pending)
        assert tuple(x.shape) == tuple(m.shape), (tuple(x.shape), tuple(m.shape))
        assert p == P_ATTN
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
    print(f"attention dropout {P_ATTN}: loss {float(loss):.6f} vs oracle {float(ref_loss):.6f} (rel {d_loss:.2e})")
    assert d_loss < LOSS_TOL
    worst = ("", 0.0)
    for n, g in got.items():
        r = osd[n].grad
        if float(r.norm()) < 1e-6:   # k_proj.bias: softmax is shift-invariant, the true gradient is zero (the dropped dS rows still sum to zero)
            assert float(g.norm()) < 1e-2, n
            continue
        e = rel(g, r)
        if e > worst[1]:
            worst = (n, e)
    print(f"attention dropout {P_ATTN}: worst gradient error {worst[1]:.3e} ({worst[0]})")
    assert worst[1] < GRAD_TOL, worst
    # the loss really is a dropped one: the eval loss of the same weights differs
    assert float(run_fwd(model.eval(), b)[0]) != float(loss)


def test_determinism_per_seed_and_step_and_eval_independence():
    ocfg = G.tiny_config(attention_dropout=P_ATTN)
    sd = G.trained_state_dict()
    b = tiny_batch(seed=41, **RAGGED4)
    model = build(ocfg, sd).train()
    eng = model._engine
    outs = []
    for _ in range(2):
        eng.set_seed(123)
        loss = run_fwd(model, b)[0]
        loss.backward()
        outs.append((float(loss), grads_of(model), site_seeds(eng, ocfg)))
    assert outs[0][0] == outs[1][0] and outs[0][2] == outs[1][2]
    n_rows = b["input_ids"].numel() + b["decoder_input_ids"].numel()
    assert not same_gradients(outs[0][1], outs[1][1], n_rows)
    assert math.isfinite(outs[0][0]) and all(bool(torch.isfinite(g).all()) for g in outs[0][1].values())
    eng.set_seed(124)
    other = float(run_fwd(model, b)[0])
    assert other != outs[0][0] and site_seeds(eng, ocfg) != outs[0][2]
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
    eng.set_attention_dropout(0.0)
    run_fwd(model.train(), b)[0].backward()
    assert site_seeds(eng, ocfg) == [(0, 0)] * len(second)

    # ---- eval, generate and score: bit-identical to a model built with attention_dropout = 0 on the same weights
    plain = build(G.tiny_config(), sd).eval()
    drop = build(ocfg, sd).eval()
    assert drop._engine.attention_dropout == P_ATTN and plain._engine.attention_dropout == 0.0
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
            att = run_fwd(m.train() if m is drop else m, b, output_attentions=True)   # the weights BEFORE dropout (HF 3.0.2)
            m.eval()
        torch.cuda.synchronize()
        res.append((loss.clone(), logits.clone(), ids.clone(), sc.token_logprobs.clone(), sc.nll.clone(), [a.clone() for a in att[2]]))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert torch.equal(res[0][2], res[1][2])
    assert torch.equal(res[0][3], res[1][3]) and torch.equal(res[0][4], res[1][4])
    # output_attentions of a TRAINING forward with dropout: layer 0's self-attention weights (their input precedes every attention
    # dropout) are the undropped softmax, i.e. the eval model's bits
    assert torch.equal(res[0][5][0], res[1][5][0])


def _splitmix(x):
    M = (1 << 64) - 1
    x = (x + 0x9E3779B97F4A7C15) & M
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M
    return x ^ (x >> 31)


def test_existing_dropout_sites_keep_their_masks():
    """dropout = 0.1 AND attention_dropout = 0.1: finite, deterministic, and the embedding site (number 1, seed
    splitmix(seed ^ splitmix(step * 0x10001 + 1)) as ever) drops exactly the elements it drops without attention dropout."""
    sd = G.golden_state_dict(G.tiny_config(), seed=21)
    b = tiny_batch(seed=31, **RAGGED4)
    seed, step = 4242, 1
    states, losses = [], []
    for p_attn in (P_ATTN, 0.0, P_ATTN):
        model = build(G.tiny_config(dropout=0.1, attention_dropout=p_attn), sd).train()
        model._engine.set_seed(seed)
        loss = run_fwd(model, b)[0]
        enc0, dec0 = model._engine.hidden_states(0)[0].clone(), model._engine.hidden_states(1)[0].clone()
        loss.backward()
        g = grads_of(model)
        assert math.isfinite(float(loss)) and all(bool(torch.isfinite(x).all()) for x in g.values())
        states.append((enc0, dec0, g))
        losses.append(float(loss))
    assert losses[0] == losses[2]                                                                                # deterministic
    assert not same_gradients(states[0][2], states[2][2], b["input_ids"].numel() + b["decoder_input_ids"].numel())
    assert losses[0] != losses[1]                                                                                # and really dropped
    # the embedding outputs precede every attention: the same bits with and without attention dropout
    assert torch.equal(states[0][0], states[1][0]) and torch.equal(states[0][1], states[1][1])
    B, S = b["input_ids"].shape
    d = 128
    for site, x in ((1, states[0][0]), (2, states[0][1])):
        site_seed = _splitmix(seed ^ _splitmix(step * 0x10001 + site)) & 0xffffffff
        rows = x.numel() // d
        keep = dropout_mask(site_seed, 0.1, rows, d)
        x2 = x.reshape(rows, d)
        assert bool((x2[~keep] == 0).all()), site
        assert float((x2[keep] == 0).float().mean()) < 1e-3, site   # (a kept LayerNorm output is zero only by accident)


def test_pretraining_and_bare_models_train_with_attention_dropout():
    from src.data.synthetic import make_pretrain_batch
    kw = dict(num_labels=37, num_attributes=11, num_relations=9, lm_loss_factor=5.0, mrm_loss_factor=1.0, attribute_loss_factor=2.0,
              relation_loss_factor=0.5)
    ocfg = G.tiny_config(attention_dropout=P_ATTN, **kw)
    sd = G.golden_state_dict(ocfg, seed=33)
    b = make_pretrain_batch(3, enc_len=24, dec_len=16, num_regions=6, seed=77, num_labels=37, num_attributes=11, num_relations=9,
                            vocab_hi=G.TINY_SPECIAL_BASE, img_feat_id=ocfg.img_feat_id, special_base=G.TINY_SPECIAL_BASE,
                            cls_id=ocfg.cls_token_id, mrm_probability=0.3)
    b["image_features"] = G.golden_features([6, 6, 6])
    model = build(ocfg, sd, cls=MultiModalBartForPreTraining, **kw).train()
    outs = []
    for seed in (5, 5, 6):
        model._engine.set_seed(seed)
        losses = model(input_ids=b["input_ids"].to(DEV), image_features=[f.to(DEV) for f in b["image_features"]],
                       attention_mask=b["attention_mask"].to(DEV), decoder_input_ids=b["decoder_input_ids"].to(DEV),
                       decoder_attention_mask=b["decoder_attention_mask"].to(DEV), labels=b["labels"].to(DEV), mrm_labels=b["mrm_labels"],
                       mrm_mask=b["mrm_mask"], attribute_labels=b["attribute_labels"], attribute_mask=b["attribute_mask"],
                       relation_labels=b["relation_labels"])[0]
        losses["loss"].backward()
        g = grads_of(model)
        assert all(math.isfinite(float(losses[k])) for k in ("loss", "lm_loss", "mrm_loss", "attribute_loss", "relation_loss"))
        assert all(bool(torch.isfinite(x).all()) for x in g.values())
        assert all(thr == THR16 for thr, _ in site_seeds(model._engine, ocfg))
        outs.append(([float(losses[k]) for k in ("loss", "lm_loss", "mrm_loss", "attribute_loss", "relation_loss")], g,
                     site_seeds(model._engine, ocfg)))
    # the forward has no atomics: every loss term and every site's seed per seed, bit for bit
    assert outs[0][0] == outs[1][0] and outs[0][2] == outs[1][2]
    assert outs[0][0][0] != outs[2][0][0] and outs[0][2] != outs[2][2]
    # backward: the three heads hand their input gradients to the decoder states by fp32 atomic scatter-adds (csrc/heads.hip; rows repeat:
    # relations share objects) before the sum is rounded to bf16, so -- with or without dropout -- an element of that bf16 tensor may land
    # one ulp (2^-8 relative) apart between two runs, and every gradient behind it with it: far inside 2^-8 norm-wise, which a mask
    # that moved would not be (the other seed's gradients are compared for contrast)
    for n in outs[0][1]:
        if float(outs[0][1][n].norm()) == 0.0:
            assert float(outs[1][1][n].norm()) == 0.0, n
            continue
        assert rel(outs[1][1][n], outs[0][1][n]) < 2.0 ** -8, n
    moved = [n for n in outs[0][1] if float(outs[0][1][n].norm()) > 0 and rel(outs[2][1][n], outs[0][1][n]) >= 2.0 ** -8]
    assert len(moved) > len(outs[0][1]) // 2, "another seed must move the gradients"

    bare = MultiModalBartModel(cfg_from_oracle(G.tiny_config(attention_dropout=P_ATTN)))
    bare.to(DEV)
    vb = tiny_batch(seed=41, **RAGGED4)
    args = dict(input_ids=vb["input_ids"].to(DEV), image_features=[f.to(DEV) for f in vb["image_features"]],
                attention_mask=vb["attention_mask"].to(DEV), decoder_input_ids=vb["decoder_input_ids"].to(DEV),
                decoder_attention_mask=vb["decoder_attention_mask"].to(DEV))
    with torch.no_grad():
        dec_train = bare.train()(**args)[0].clone()
        assert all(thr == THR16 for thr, _ in site_seeds(bare._engine, G.tiny_config()))
        dec_eval = bare.eval()(**args)[0].clone()
    assert bool(torch.isfinite(dec_train.float()).all()) and not torch.equal(dec_train, dec_eval)


def test_fine_tuning_driver_runs_with_attention_dropout(tmp_path):
    """vcg_train.py --synthetic ... --attention_dropout 0.1 on a two-layer d = 128 configuration (the synthetic batches carry the full
    vocabulary's ids): the flag reaches the engine and every logged loss is finite."""
    cfg = dict(vocab_size=50320, d_model=128, encoder_layers=2, decoder_layers=2, encoder_attention_heads=2, decoder_attention_heads=2,
               encoder_ffn_dim=256, decoder_ffn_dim=256, max_position_embeddings=128, dropout=0.1, attention_dropout=0.0,
               activation_dropout=0.0, init_std=0.02)
    (tmp_path / "tiny.json").write_text(json.dumps(cfg))
    cmd = [sys.executable, os.path.join(ROOT, "km-bart_amd", "vcg_train.py"), "--model_config", str(tmp_path / "tiny.json"),
           "--checkpoint_dir", str(tmp_path / "ckpt"), "--synthetic", "3", "--epochs", "1", "--batch_size", "4", "--attention_dropout", "0.1"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    losses = [float(x) for x in re.findall(r"Loss: ([-+.\w]+)", r.stdout)]
    assert len(losses) == 3 and all(math.isfinite(x) and 0.0 < x < 20.0 for x in losses), r.stdout[-1500:]
    saved = json.load(open(tmp_path / "ckpt" / "epoch1" / "config.json"))
    assert saved["attention_dropout"] == 0.1
