"""GPU: classification-head dropout through the engine and the model classes (config.classif_dropout; a run-time setting of the handle).

1. Oracle parity of a pre-training step: the six masks the engine drew (three heads x input, hidden) are read back per site
   (kmb_classif_dropout_site -> kmb_op_dropout_mask) and the oracle's classification head is replaced, inside the test, by one that applies
   them in call order (masked-region, attribute, relation head; HF 3.0.2 BartClassificationHead: dropout, dense, tanh, dropout, out_proj).
2. Determinism per (seed, step); eval forwards, score() and generate() do not depend on the value; a head without rows reports zeros; the
   setting back at 0 gives the bits of a handle that never had it.
3. The other three dropout families keep their seeds whether classif_dropout is on or not.
4. pretrain.py --classif_dropout 0.1 trains.
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
from src.data.synthetic import make_pretrain_batch  # noqa: E402
from src.model import MultiModalBartForPreTraining  # noqa: E402
from gpu_util import dropout_mask  # noqa: E402
from test_attention_dropout_model_gpu import DEV, GRAD_TOL, ROOT, _splitmix, build, grads_of, rel, same_gradients  # noqa: E402
from test_attention_dropout_model_gpu import site_seeds as attn_site_seeds  # noqa: E402
from test_activation_dropout_model_gpu import site_seeds as act_site_seeds  # noqa: E402

P_CLS = 0.1
THR16 = 6554
SCALE = float(torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(float(THR16)) / 65536.0))   # fp32, as the engine computes it
HEADS = ("mrm_head", "attribute_head", "relation_head")
SITES = [(head, which) for head in range(3) for which in range(2)]
TERMS = ("loss", "lm_loss", "mrm_loss", "attribute_loss", "relation_loss")
# the tiny pre-training configuration and batch of tests/test_model_gpu.py::test_pretraining_heads_against_oracle
KW = dict(num_labels=37, num_attributes=11, num_relations=9, lm_loss_factor=5.0, mrm_loss_factor=1.0, attribute_loss_factor=2.0,
          relation_loss_factor=0.5)


def tiny_pretrain_batch():
    ocfg = G.tiny_config(**KW)
    b = make_pretrain_batch(3, enc_len=24, dec_len=16, num_regions=6, seed=77, num_labels=37, num_attributes=11, num_relations=9,
                            vocab_hi=G.TINY_SPECIAL_BASE, img_feat_id=ocfg.img_feat_id, special_base=G.TINY_SPECIAL_BASE,
                            cls_id=ocfg.cls_token_id, mrm_probability=0.3)
    b["image_features"] = G.golden_features([6, 6, 6])
    return b


def pre_model(sd, classif_dropout=P_CLS, **drops):
    """the pre-training model on the golden weights; classif_dropout reaches the engine through the config, as pretrain.py passes it"""
    return build(G.tiny_config(**drops, **KW), sd, cls=MultiModalBartForPreTraining, classif_dropout=classif_dropout, **KW)


def pre_fwd(model, b, **over):
    args = dict(input_ids=b["input_ids"].to(DEV), image_features=[f.to(DEV) for f in b["image_features"]],
                attention_mask=b["attention_mask"].to(DEV), decoder_input_ids=b["decoder_input_ids"].to(DEV),
                decoder_attention_mask=b["decoder_attention_mask"].to(DEV), labels=b["labels"].to(DEV), mrm_labels=b["mrm_labels"],
                mrm_mask=b["mrm_mask"], attribute_labels=b["attribute_labels"], attribute_mask=b["attribute_mask"],
                relation_labels=b["relation_labels"])
    args.update(over)
    return model(**args)[0]


def cls_sites(eng):
    return [eng.classif_dropout_site(head, which) for head, which in SITES]


def head_rows(b):
    return [int(b["mrm_mask"].sum()), int(b["attribute_mask"].sum()), sum(len(r) for r in b["relation_labels"])]


def values(losses):
    return {k: float(losses[k].detach()) for k in TERMS if k in losses}


def test_pretraining_step_matches_the_oracle_under_the_exported_masks(monkeypatch):
    ocfg = G.tiny_config(**KW)               # dropout = attention_dropout = activation_dropout = 0: the head masks are the only ones
    sd = G.golden_state_dict(ocfg, seed=33)
    b = tiny_pretrain_batch()
    model = pre_model(sd).train()
    eng = model._engine
    assert eng.classif_dropout == P_CLS
    eng.set_seed(777)
    losses = pre_fwd(model, b)
    losses["loss"].backward()
    got = grads_of(model)
    d = ocfg.d_model
    n = head_rows(b)
    assert all(x > 0 for x in n), n
    sites = cls_sites(eng)
    assert all(thr == THR16 for thr, _ in sites), sites
    assert len({seed for _, seed in sites}) == 6, "every site draws its own seed"
    masks = []
    for (head, which), (thr, seed) in zip(SITES, sites):
        cols = d if which == 1 else (2 * d if head == 2 else d)
        m = dropout_mask(seed, thr / 65536.0, n[head], cols).cpu()
        keep_p, count = 1.0 - thr / 65536.0, n[head] * cols
        sigma = math.sqrt(keep_p * (1.0 - keep_p) / count)
        rate = float(m.float().mean())
        print(f"classif site {head}/{which}: {n[head]} x {cols}, keep rate {rate:.4f} ({(rate - keep_p) / sigma:+.2f} sigma)")
        assert abs(rate - keep_p) <= 5.0 * sigma, (head, which, rate)
        masks.append(m)
    pending = iter(masks)
    called = []

    def masked_head(sd_, name, x):
        """dropout -> dense -> tanh -> dropout -> out_proj with the engine's masks (reference src/model/model.py:133-158)"""
        m_in, m_h = next(pending), next(pending)
        assert tuple(x.shape) == tuple(m_in.shape), (name, tuple(x.shape), tuple(m_in.shape))
        called.append(name)
        x = x * (m_in.to(x.dtype) * SCALE)
        y = torch.tanh(O._lin(x, sd_, name + ".dense"))
        assert tuple(y.shape) == tuple(m_h.shape)
        return O._lin(y * (m_h.to(y.dtype) * SCALE), sd_, name + ".out_proj")

    monkeypatch.setattr(O, "classification_head", masked_head)
    osd = {k: v.clone().requires_grad_(k != "final_logits_bias") for k, v in sd.items()}
    ref, _ = O.pretrain_forward(osd, ocfg, b["input_ids"], b["image_features"], b["attention_mask"], b["decoder_input_ids"],
                                b["decoder_attention_mask"], b["labels"], b["mrm_labels"], b["mrm_mask"], b["attribute_labels"],
                                b["attribute_mask"], b["relation_labels"], training=True)
    ref["loss"].backward()
    monkeypatch.undo()
    assert called == list(HEADS) and next(pending, None) is None
    got_losses = values(losses)
    assert set(got_losses) == set(TERMS)
    for k in TERMS:
        print(f"classif dropout {P_CLS}: {k} {got_losses[k]:.6f} vs oracle {float(ref[k]):.6f}")
        assert abs(got_losses[k] - float(ref[k])) <= 2e-3 * abs(float(ref[k])) + 1e-4, (k, got_losses[k], float(ref[k]))
    worst = ("", 0.0)
    for name, g in got.items():
        r = osd[name].grad
        if r is None:
            continue
        if float(r.norm()) < 1e-6:   # k_proj.bias: softmax is shift-invariant, the true gradient is zero
            assert float(g.norm()) < 1e-2, name
            continue
        e = rel(g, r)
        if e > worst[1]:
            worst = (name, e)
    print(f"classif dropout {P_CLS}: worst gradient error {worst[1]:.3e} ({worst[0]})")
    assert worst[1] < GRAD_TOL, worst
    assert all(osd[h + ".dense.weight"].grad is not None for h in HEADS)
    # the losses really are dropped ones: the eval losses of the same weights differ, and an eval forward leaves the record alone
    with torch.no_grad():
        ev = values(pre_fwd(model.eval(), b))
    assert all(ev[k] != got_losses[k] for k in ("loss", "mrm_loss", "attribute_loss", "relation_loss")), ev
    assert abs(ev["lm_loss"] - got_losses["lm_loss"]) <= 1e-3 * ev["lm_loss"]   # nothing in front of the LM head drops in this configuration
    assert cls_sites(eng) == sites


def test_determinism_and_isolation():
    sd = G.golden_state_dict(G.tiny_config(**KW), seed=33)
    b = tiny_pretrain_batch()
    n_rows = b["input_ids"].numel() + b["decoder_input_ids"].numel()
    model = pre_model(sd).train()
    eng = model._engine
    runs = []
    for _ in range(2):
        eng.set_seed(123)
        losses = pre_fwd(model, b)
        losses["loss"].backward()
        runs.append((values(losses), grads_of(model), cls_sites(eng)))
    assert runs[0][0] == runs[1][0] and runs[0][2] == runs[1][2]
    assert not same_gradients(runs[0][1], runs[1][1], n_rows)
    assert all(math.isfinite(v) for v in runs[0][0].values()) and all(bool(torch.isfinite(g).all()) for g in runs[0][1].values())
    # the documented seeds: splitmix(seed ^ splitmix(step * 0x10001 + 0x50000000 + 2 * head + which)), step 1
    for (head, which), (thr, s) in zip(SITES, runs[0][2]):
        assert thr == THR16 and s == _splitmix(123 ^ _splitmix(0x10001 + 0x50000000 + 2 * head + which)) & 0xffffffff, (head, which)
    # the next step of the same seed, and another seed, draw other masks
    pre_fwd(model, b)["loss"].backward()
    second = cls_sites(eng)
    assert all(a[1] != c[1] and c[0] == THR16 for a, c in zip(runs[0][2], second))
    eng.set_seed(124)
    other = pre_fwd(model, b)
    other["loss"].backward()
    assert values(other) != runs[0][0] and all(a[1] != c[1] for a, c in zip(runs[0][2], cls_sites(eng)))
    # a head whose row list is empty reports zeros (the reference skips the term), the others draw as before
    eng.set_seed(123)
    no_rel = pre_fwd(model, b, relation_labels=[[] for _ in b["relation_labels"]])
    no_rel["loss"].backward()
    assert "relation_loss" not in no_rel
    sites = cls_sites(eng)
    assert sites[:4] == runs[0][2][:4] and sites[4:] == [(0, 0), (0, 0)]
    assert values(no_rel)["mrm_loss"] == runs[0][0]["mrm_loss"] and values(no_rel)["attribute_loss"] == runs[0][0]["attribute_loss"]

    # ---- the setting back at 0: the bits of a handle that never had it (train mode, same seed)
    plain = pre_model(sd, classif_dropout=0.0).train()
    assert plain._engine.classif_dropout == 0.0
    res = []
    eng.set_classif_dropout(0.0)
    for m in (plain, model):
        m._engine.set_seed(123)
        losses = pre_fwd(m, b)
        losses["loss"].backward()
        res.append((values(losses), grads_of(m)))
        assert cls_sites(m._engine) == [(0, 0)] * 6
    assert res[0][0] == res[1][0] and not same_gradients(res[0][1], res[1][1], n_rows)
    assert res[0][0] != runs[0][0]
    eng.set_classif_dropout(P_CLS)

    # ---- eval forwards, score() and generate(): bit-identical to the model built with classif_dropout = 0
    feats = [f.to(DEV) for f in b["image_features"]]
    out = []
    for m in (plain, model):
        m.eval()
        with torch.no_grad():
            ev = values(pre_fwd(m, b))
            ids = m.generate(input_ids=b["input_ids"].to(DEV), image_features=feats, attention_mask=b["attention_mask"].to(DEV),
                             num_beams=3, max_length=10, early_stopping=True)
            sc = m.score(input_ids=b["input_ids"].to(DEV), image_features=feats, attention_mask=b["attention_mask"].to(DEV),
                         decoder_input_ids=b["decoder_input_ids"].to(DEV), decoder_attention_mask=b["decoder_attention_mask"].to(DEV),
                         labels=b["labels"].to(DEV))
        torch.cuda.synchronize()
        out.append((ev, ids.clone(), sc.token_logprobs.clone(), sc.nll.clone()))
    assert model._engine.classif_dropout == P_CLS
    assert out[0][0] == out[1][0] and torch.equal(out[0][1], out[1][1])
    assert torch.equal(out[0][2], out[1][2]) and torch.equal(out[0][3], out[1][3])


def test_the_other_dropout_families_keep_their_seeds():
    """dropout = attention_dropout = activation_dropout = 0.1 with classif_dropout 0.1 and 0: the attention and the activation sites report the
    same seeds, the model trains, and the head sites draw only when the setting is on"""
    base = dict(dropout=0.1, attention_dropout=0.1, activation_dropout=0.1)
    ocfg = G.tiny_config(**base, **KW)
    sd = G.golden_state_dict(G.tiny_config(**KW), seed=33)
    b = tiny_pretrain_batch()
    seen = []
    for p_cls in (P_CLS, 0.0):
        model = pre_model(sd, classif_dropout=p_cls, **base).train()
        model._engine.set_seed(4242)
        losses = pre_fwd(model, b)
        losses["loss"].backward()
        g = grads_of(model)
        assert all(math.isfinite(v) for v in values(losses).values()) and all(bool(torch.isfinite(x).all()) for x in g.values())
        seen.append((attn_site_seeds(model._engine, ocfg), act_site_seeds(model._engine, ocfg), cls_sites(model._engine), values(losses)))
    assert seen[0][0] == seen[1][0] and all(thr == THR16 for thr, _ in seen[0][0])
    assert seen[0][1] == seen[1][1] and all(thr == THR16 for thr, _ in seen[0][1])
    assert all(thr == THR16 for thr, _ in seen[0][2]) and seen[1][2] == [(0, 0)] * 6
    assert seen[0][3]["lm_loss"] == seen[1][3]["lm_loss"]          # everything in front of the heads drew the same masks
    assert seen[0][3]["mrm_loss"] != seen[1][3]["mrm_loss"]
    every = [s for _, s in seen[0][0] + seen[0][1] + seen[0][2]]
    assert len(set(every)) == len(every)


def test_pretraining_driver_runs_with_classif_dropout(tmp_path):
    """pretrain.py --synthetic 2 --classif_dropout 0.1 on a two-layer d = 128 configuration (the synthetic batches carry the full vocabulary's
    ids and the full class counts): the flag reaches the engine and every logged loss is finite"""
    cfg = dict(vocab_size=50320, d_model=128, encoder_layers=2, decoder_layers=2, encoder_attention_heads=2, decoder_attention_heads=2,
               encoder_ffn_dim=256, decoder_ffn_dim=256, max_position_embeddings=128, dropout=0.1, attention_dropout=0.0,
               activation_dropout=0.0, classif_dropout=0.0, init_std=0.02, num_labels=1601, num_attributes=129, num_relations=129)
    (tmp_path / "tiny.json").write_text(json.dumps(cfg))
    cmd = [sys.executable, os.path.join(ROOT, "km-bart_amd", "pretrain.py"), "--model_config", str(tmp_path / "tiny.json"),
           "--checkpoint_dir", str(tmp_path / "ckpt"), "--synthetic", "2", "--epochs", "1", "--batch_size", "4", "--max_img_num", "6",
           "--classif_dropout", "0.1"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    losses = [float(x) for x in re.findall(r"Loss: ([-+.\w]+)", r.stdout)]
    assert len(losses) == 2 and all(math.isfinite(x) and 0.0 < x < 100.0 for x in losses), r.stdout[-1500:]
    saved = json.load(open(tmp_path / "ckpt" / "model0" / "config.json"))
    assert saved["classif_dropout"] == 0.1
