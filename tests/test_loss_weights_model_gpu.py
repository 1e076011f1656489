"""GPU: per-row loss weights through the model classes, against the CPU oracle's logits fed to F.cross_entropy(reduction="none"), weighted and
reduced in torch with autograd (the oracle itself is unchanged), on the tiny configuration (bf16 head, fp32 head, fp32 validation mode), on
the smallest configuration that takes the fused head, on the pre-training model and through src.training.self_critical_step.

The weights are per sequence, w_b = (1.75, -0.5, 0.75, 1.25)[b % 4].  Each test first asserts, of the reference alone, that the weights move
the loss by >= 20 x LOSS_TOL and every compared gradient by >= 3 x GRAD_TOL against the unweighted reference (on the CPU oracle: tiny
6.195 -> 5.657 and the smallest gradient move 0.71; fused 9.029 -> 7.783 and 0.28).

Tolerances are the project's own: LOSS_TOL = 1e-3 relative and GRAD_TOL = 3e-2 norm-wise (tests/test_model_gpu.py); fused against two-kernel
head 2e-4 on the loss and 1.5e-2 norm-wise per gradient (tests/test_label_smoothing_model_gpu.py); 1e-4 on the fp32 validation mode's loss
(tests/test_fp32_mode_gpu.py); the tied matrix's bits under the spread rule of tests/test_grad_accum_model_gpu.py (its embedding
scatter-adds are fp32 atomics)."""
import json
import os
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "km-bart_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import goldenlib as G  # noqa: E402
from oracle import kmbart_oracle as O  # noqa: E402
from oracle.make_golden import tiny_batch  # noqa: E402
from src.data.synthetic import make_pretrain_batch  # noqa: E402
from src.model import MultiModalBartForPreTraining  # noqa: E402
from src.model.utils import labels_from_generated  # noqa: E402
from src.training import self_critical_step  # noqa: E402
import loss_weights_ref as W  # noqa: E402
from test_model_gpu import GRAD_TOL, LOSS_TOL, build, cfg_from_oracle, rel, run_fwd  # noqa: E402
from test_grad_accum_model_gpu import PRE_KW, bits, tied_range, ulp_of  # noqa: E402
from test_label_smoothing_model_gpu import (FORM_BF16, FORM_FP32, FORM_FUSED, _grads, _per_param_err, assert_reference_moves,  # noqa: E402
                                            check_against, fused_batch, oracle_logits)

DEV = "cuda:0"


# ------------------------------------------------------------------------------------------------ the reference
def weighted_loss(logits, labels, w_bt, reduction, eps=0.0):
    """sum_r w_r F.cross_entropy(reduction='none')_r / D; the weights of -100 rows are not read (they may be NaN)"""
    rows = F.cross_entropy(logits.reshape(-1, logits.shape[-1]), labels.reshape(-1), ignore_index=-100, label_smoothing=eps, reduction="none")
    ok = labels.reshape(-1) != -100
    w = torch.where(ok, w_bt.reshape(-1).to(rows.dtype), torch.zeros_like(rows))
    return (w * rows).sum() / (int(ok.sum()) if reduction == "mean" else 1)


def reference(ocfg, sd, b, w, reduction, eps=0.0):
    """(loss, {name: gradient}); w: [B] or [B, T] or None (unweighted)"""
    osd, logits = oracle_logits(ocfg, sd, b, grad=True)
    B, T = b["labels"].shape
    w_bt = torch.ones(B, T) if w is None else (w[:, None].expand(B, T) if w.dim() == 1 else w)
    loss = weighted_loss(logits, b["labels"], w_bt, reduction, eps)
    loss.backward()
    return float(loss.detach()), {k: v.grad for k, v in osd.items() if v.grad is not None}


class Case:
    """a configuration, its weights, a batch and the references: computed once, never changed"""

    def __init__(self, ocfg, sd, b):
        self.ocfg, self.sd, self.b = ocfg, sd, b
        self.w = W.seq_weights(b["labels"].shape[0])
        self.refs = {}

    def ref(self, weighted, reduction, eps=0.0):
        key = (weighted, reduction, eps)
        if key not in self.refs:
            self.refs[key] = reference(self.ocfg, self.sd, self.b, self.w if weighted else None, reduction, eps)
        return self.refs[key]

    def model(self):
        return build(self.ocfg, self.sd).eval()


@pytest.fixture(scope="module")
def tiny():
    ocfg = G.tiny_config()
    return Case(ocfg, G.golden_state_dict(ocfg, seed=21), tiny_batch(seed=31, regions=(6, 3), event_lens=(8, 4), label_lens=(12, 7)))


@pytest.fixture(scope="module")
def fusedcase():
    ocfg = G.tiny_config(vocab_size=8150)
    return Case(ocfg, G.golden_state_dict(ocfg, seed=23), fused_batch(41))


def _fwd_bwd(model, b, **kw):
    loss = run_fwd(model, b, **kw)[0]
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), _grads(model)


# ------------------------------------------------------------------------------------------------ (a) the tiny configuration, bf16 head
@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_a_tiny_against_the_oracle(tiny, reduction):
    ref = tiny.ref(True, reduction)
    assert_reference_moves(tiny.ref(False, reduction), ref)
    print("tiny %s: unweighted %.4f weighted %.4f, valid labels %d" % (reduction, tiny.ref(False, reduction)[0], ref[0],
                                                                        int((tiny.b["labels"] != -100).sum())))
    model = tiny.model()
    loss = run_fwd(model, tiny.b, loss_weights=tiny.w.to(DEV), loss_reduction=reduction)[0]
    model._engine.check_inputs()
    assert model._engine.last_head_form() == FORM_BF16
    loss.backward()
    torch.cuda.synchronize()
    check_against(model, ref, "tiny weighted %s" % reduction, loss)
    with torch.no_grad():   # an eval no_grad forward returns the same weighted loss
        loss_ng = run_fwd(model, tiny.b, loss_weights=tiny.w.to(DEV), loss_reduction=reduction)[0]
    assert abs(float(loss_ng) - ref[0]) / abs(ref[0]) < LOSS_TOL


# ------------------------------------------------------------------------------------------------ (b) the fused head
@pytest.mark.parametrize("eps", [0.0, 0.2])
def test_b_fused_head_against_the_oracle_and_the_two_kernel_head(fusedcase, monkeypatch, eps):
    c = fusedcase
    ref = c.ref(True, "mean", eps)
    assert_reference_moves(c.ref(False, "mean", eps), ref)
    print("fused eps %.1f: unweighted %.4f weighted %.4f, valid labels %d" % (eps, c.ref(False, "mean", eps)[0], ref[0],
                                                                              int((c.b["labels"] != -100).sum())))
    model = c.model()
    model.label_smoothing = eps
    eng = model._engine
    w = c.w.to(DEV)
    loss, g_fused = _fwd_bwd(model, c.b, loss_weights=w)
    eng.check_inputs()
    assert eng.last_head_form() == FORM_FUSED
    check_against(model, ref, "fused head weighted eps=%.1f" % eps, loss)
    # [B, T] weights equal to the broadcast [B] ones: identical bits (the tied matrix under its spread rule)
    B, T = c.b["labels"].shape
    loss_bt, g_bt = _fwd_bwd(model, c.b, loss_weights=w[:, None].expand(B, T).contiguous())
    _, g_again = _fwd_bwd(model, c.b, loss_weights=w)
    assert torch.equal(bits(loss_bt), bits(loss))
    _same_bits_outside_tied(eng, g_bt, g_fused, g_again)
    monkeypatch.setenv("KMB_FUSED_CE", "0")
    loss2, g_two = _fwd_bwd(model, c.b, loss_weights=w)
    assert eng.last_head_form() == FORM_BF16
    monkeypatch.delenv("KMB_FUSED_CE")
    check_against(model, ref, "two-kernel head weighted eps=%.1f" % eps, loss2)
    print("loss fused %.6f vs two-kernel %.6f vs oracle %.6f" % (float(loss), float(loss2), ref[0]))
    assert abs(float(loss) - float(loss2)) <= 2e-4 * abs(float(loss2))
    errs = _per_param_err(eng, g_fused, g_two)
    print("worst gradient differences fused vs two-kernel:", errs[:4])
    assert max(e for e, name in errs if "k_proj.bias" not in name) < 1.5e-2, errs[:6]


def _same_bits_outside_tied(eng, got, want, want_again):
    """gradient bits equal outside the tied matrix; inside it within the spread of two runs of the same thing (fp32 atomics)"""
    lo, hi = tied_range(eng)
    same = bits(got) == bits(want)
    same[lo:hi] = True
    assert bool(same.all()), int((~same).sum())
    spread = float((want[lo:hi] - want_again[lo:hi]).abs().max())
    bound = max(4.0 * spread, ulp_of(float(want[lo:hi].abs().max())))
    assert float((got[lo:hi] - want[lo:hi]).abs().max()) <= bound


# ------------------------------------------------------------------------------------------------ (c) the fp32 head
def test_c_fp32_head_and_fp32_validation_mode(tiny):
    ref = tiny.ref(True, "mean")
    assert_reference_moves(tiny.ref(False, "mean"), ref)
    model = tiny.model()
    w = tiny.w.to(DEV)
    loss = run_fwd(model, tiny.b, return_logits=True, loss_weights=w)[0]
    assert model._engine.last_head_form() == FORM_FP32
    assert abs(float(loss) - ref[0]) / abs(ref[0]) < LOSS_TOL
    loss.backward()
    torch.cuda.synchronize()
    check_against(model, ref, "fp32 head weighted")
    model._engine.set_precision(True)
    try:
        with torch.no_grad():
            loss32 = run_fwd(model, tiny.b, loss_weights=w)[0]
            sum32 = run_fwd(model, tiny.b, loss_weights=w, loss_reduction="sum")[0]
    finally:
        model._engine.set_precision(False)
    print("fp32 validation mode: weighted loss %.6f against %.6f" % (float(loss32), ref[0]))
    assert abs(float(loss32) - ref[0]) / abs(ref[0]) < 1e-4
    assert abs(float(sum32) - tiny.ref(True, "sum")[0]) / abs(tiny.ref(True, "sum")[0]) < 1e-4


# ------------------------------------------------------------------------------------------------ (d) identity
@pytest.mark.parametrize("which", ["tiny", "fused"])
def test_d_none_and_unit_weights_are_identical(tiny, fusedcase, which):
    c = tiny if which == "tiny" else fusedcase
    model = c.model()
    B, T = c.b["labels"].shape
    l_none, g_none = _fwd_bwd(model, c.b)
    _, g_none2 = _fwd_bwd(model, c.b)
    assert model._engine.last_head_form() == (FORM_BF16 if which == "tiny" else FORM_FUSED)
    for ones in (torch.ones(B, device=DEV), torch.ones(B, T, device=DEV)):
        l_one, g_one = _fwd_bwd(model, c.b, loss_weights=ones)
        assert torch.equal(bits(l_one), bits(l_none)), (float(l_one), float(l_none))
        _same_bits_outside_tied(model._engine, g_one, g_none, g_none2)


# ------------------------------------------------------------------------------------------------ (e) ignored rows
def test_e_nan_weights_on_ignored_rows(tiny):
    model = tiny.model()
    B, T = tiny.b["labels"].shape
    w_bt = tiny.w[:, None].expand(B, T).clone()
    l_a, g_a = _fwd_bwd(model, tiny.b, loss_weights=w_bt.to(DEV))
    _, g_a2 = _fwd_bwd(model, tiny.b, loss_weights=w_bt.to(DEV))
    ignored = tiny.b["labels"] == -100
    assert int(ignored.sum()) > 0
    w_bt[ignored] = float("nan")
    l_n, g_n = _fwd_bwd(model, tiny.b, loss_weights=w_bt.to(DEV))
    assert bool(torch.isfinite(l_n)) and bool(torch.isfinite(g_n).all())
    assert torch.equal(bits(l_n), bits(l_a))
    _same_bits_outside_tied(model._engine, g_n, g_a, g_a2)
    assert abs(float(l_n) - tiny.ref(True, "mean")[0]) / abs(tiny.ref(True, "mean")[0]) < LOSS_TOL


# ------------------------------------------------------------------------------------------------ (f) accumulation
def _half(b, lo, hi):
    out = {k: (v[lo:hi] if torch.is_tensor(v) else v) for k, v in b.items()}
    out["image_features"] = b["image_features"][lo:hi]
    return out


def test_f_sum_is_additive_over_micro_batches(fusedcase):
    c = fusedcase
    ref = c.ref(True, "sum")
    assert_reference_moves(c.ref(False, "sum"), ref)
    B = c.b["labels"].shape[0]
    model = c.model()
    model.accumulate_gradients(True)
    model.zero_grad()
    total = 0.0
    for lo, hi in ((0, B // 2), (B // 2, B)):
        loss = run_fwd(model, _half(c.b, lo, hi), loss_weights=c.w[lo:hi].to(DEV), loss_reduction="sum")[0]
        loss.backward()
        total += float(loss)
    torch.cuda.synchronize()
    model.accumulate_gradients(False)
    assert abs(total - ref[0]) / abs(ref[0]) < LOSS_TOL, (total, ref[0])
    check_against(model, ref, "two weighted micro-batches, sum")


# ------------------------------------------------------------------------------------------------ (g) pre-training
def test_g_pretraining_weights_touch_the_lm_term_only():
    ocfg = G.tiny_config(**PRE_KW)
    sd = G.golden_state_dict(ocfg, seed=33)
    b = make_pretrain_batch(2, enc_len=24, dec_len=16, num_regions=6, seed=77, num_labels=37, num_attributes=11, num_relations=9,
                            vocab_hi=G.TINY_SPECIAL_BASE, img_feat_id=ocfg.img_feat_id, special_base=G.TINY_SPECIAL_BASE,
                            cls_id=ocfg.cls_token_id, mrm_probability=0.3, n_rel=2)
    b["image_features"] = G.golden_features([6, 6])
    w = W.seq_weights(2)
    B, T = b["labels"].shape
    lm_labels = b["labels"].clone()
    lm_labels[lm_labels == ocfg.cls_token_id] = -100          # reference src/model/model.py:297-298
    osd = {k: v.clone().requires_grad_(k != "final_logits_bias") for k, v in sd.items()}
    ref, logits = O.pretrain_forward(osd, ocfg, b["input_ids"], b["image_features"], b["attention_mask"], b["decoder_input_ids"],
                                     b["decoder_attention_mask"], b["labels"], b["mrm_labels"], b["mrm_mask"], b["attribute_labels"],
                                     b["attribute_mask"], b["relation_labels"])
    lm_w = PRE_KW["lm_loss_factor"] * weighted_loss(logits, lm_labels, w[:, None].expand(B, T), "mean")
    total = ref["loss"] - ref["lm_loss"] + lm_w
    total.backward()
    assert abs(float(lm_w) - float(ref["lm_loss"])) / abs(float(ref["lm_loss"])) >= 20 * LOSS_TOL

    m = MultiModalBartForPreTraining(cfg_from_oracle(ocfg, **PRE_KW))
    m.load_state_dict(sd, strict=False)
    m.to(DEV).eval()

    def fwd(**kw):
        return m(input_ids=b["input_ids"].to(DEV), image_features=[f.to(DEV) for f in b["image_features"]],
                 attention_mask=b["attention_mask"].to(DEV), decoder_input_ids=b["decoder_input_ids"].to(DEV),
                 decoder_attention_mask=b["decoder_attention_mask"].to(DEV), labels=b["labels"].to(DEV),
                 mrm_labels=b["mrm_labels"], mrm_mask=b["mrm_mask"], attribute_labels=b["attribute_labels"],
                 attribute_mask=b["attribute_mask"], relation_labels=b["relation_labels"], **kw)[0]

    with torch.no_grad():
        plain = {k: v.clone() for k, v in fwd().items()}
    losses = fwd(loss_weights=w.to(DEV))
    assert abs(float(losses["lm_loss"]) - float(lm_w)) / abs(float(lm_w)) < LOSS_TOL, (float(losses["lm_loss"]), float(lm_w))
    for k in ("mrm_loss", "attribute_loss", "relation_loss"):
        assert torch.equal(bits(losses[k].detach().reshape(1)), bits(plain[k].reshape(1))), k
    parts = sum(float(losses[k]) for k in ("lm_loss", "mrm_loss", "attribute_loss", "relation_loss"))
    assert abs(float(losses["loss"]) - parts) <= 4 * 2.0 ** -23 * abs(parts)       # three fp32 additions
    assert abs(float(losses["loss"]) - float(total)) <= 2e-3 * abs(float(total)) + 1e-4      # tests/test_model_gpu.py's bound on these terms
    losses["loss"].backward()
    torch.cuda.synchronize()
    check_against(m, (float(total), {k: v.grad for k, v in osd.items() if v.grad is not None}), "pre-training, weighted LM term")


# ------------------------------------------------------------------------------------------------ (h) the self-critical step
def _reward(ids):
    pad = G.tiny_config().pad_token_id
    return 0.5 + (torch.arange(ids.shape[0], device=ids.device) % 3).float() + 0.01 * (ids != pad).sum(1).float()


def _oracle_seq(ocfg, sd, batch, ids, grad):
    """the oracle's teacher-forced log p(y_b) [B] for generated ids, with the parameters it was computed from"""
    dec_in, mask, labels = labels_from_generated(ids.cpu(), ocfg.pad_token_id, ocfg.eos_token_id)
    b = dict(batch, decoder_input_ids=dec_in, decoder_attention_mask=mask, labels=labels)
    osd, logits = oracle_logits(ocfg, sd, b, grad=grad)
    rows = F.cross_entropy(logits.reshape(-1, logits.shape[-1]), labels.reshape(-1), ignore_index=-100, reduction="none")
    return osd, -rows.reshape(labels.shape).sum(1)


def test_h_self_critical_step(gold_dir):
    """Measured on the MI355X (seed 11, max_length 12, the trained tiny fixture, top_k=0, top_p=1.0, 43 tokens): -sum_logprobs.sum() of the
    sampler 0.398999, the unit-weight "sum" forward 0.401008, the oracle's teacher-forced value 0.399823: gaps 8.2e-4 (sampler) and 1.19e-3
    (training forward), 2.0e-3 between the two (loss_weights_ref.py).  The step itself at temperature 3: loss 134.084 against
    the oracle's 134.180 (7.2e-4 relative), worst gradient 2.3e-2; with the greedy baseline 0.589518 against 0.590108.
    The unit-weight "sum" forward and -sum_logprobs.sum() of the sampler are each taken against the oracle's teacher-forced value for the
    same ids; the allowed gap between the two is twice the larger oracle gap (the decode and the training kernels round independently),
    and each oracle gap is itself inside LOSS_TOL."""
    gen = json.load(open(os.path.join(gold_dir, "tiny_generate.json")))
    ocfg, sd = G.tiny_config(), G.trained_state_dict()
    model = build(ocfg, sd).eval()
    batch = dict(input_ids=torch.tensor(gen["input_ids"]), attention_mask=torch.tensor(gen["attention_mask"]),
                 image_features=G.golden_features(gen["regions"], seed=gen["seed"]))
    B = batch["input_ids"].shape[0]
    kw = dict(max_length=12, min_length=0)
    # The fixture is trained and peaked: at temperature 1 its samples are the likely sequences, log p(y_b) ~ -0.05 and the loss 0.12, where
    # a bound RELATIVE to the loss says nothing (measured there: 0.118938 against the oracle's 0.120188, 1.25e-3 absolute over 60 tokens).
    # The step's samples are drawn at temperature 3 instead, so that the loss is of the size LOSS_TOL is meant for; the loss and its gradient
    # are those of the temperature-1 log-softmax whatever drew the ids.
    step_kw = dict(kw, temperature=3.0)
    for baseline, seed in ((None, 11), ("greedy", 12)):
        torch.manual_seed(seed)
        loss, info = self_critical_step(model, batch, _reward, DEV, baseline=baseline, sample_kwargs=step_kw)
        assert model._engine.last_head_form() == FORM_BF16
        A = info["advantages"].cpu()
        assert bool((A.abs() > 1e-3).all()) or baseline == "greedy", A
        assert torch.equal(info["rewards"].cpu(), _reward(info["sample_ids"].cpu()))
        osd, logp = _oracle_seq(ocfg, sd, batch, info["sample_ids"], grad=True)
        want = -(A * logp).sum() / B
        print("self-critical step, baseline %r: loss %.6f oracle %.6f, advantages %s" % (baseline, float(loss), float(want), A.tolist()))
        # LOSS_TOL relative to sum_b |A_b| |log p(y_b)| / B: the loss itself while the advantages share a sign (baseline None), and the larger
        # operand of the cancellation when they do not (the greedy baseline leaves advantages of +-0.01 here: a sum near zero)
        scale = float((A.abs() * logp.detach().abs()).sum() / B)
        assert scale > 0.5, "the relative bound needs a scale far from zero"
        if baseline is None:
            assert abs(scale - abs(float(want))) <= 1e-6 * scale
        assert abs(float(loss) - float(want)) <= LOSS_TOL * scale, (float(loss), float(want), scale)
        if baseline is None:
            loss.backward()
            torch.cuda.synchronize()
            want.backward()
            check_against(model, (float(want), {k: v.grad for k, v in osd.items() if v.grad is not None}), "self-critical step")
        else:
            assert "greedy_ids" in info and torch.equal(info["baseline"].cpu(), _reward(info["greedy_ids"].cpu()))
    # unfiltered sampling: the training forward's log-probabilities are the sampler's
    torch.manual_seed(11)
    with torch.no_grad():
        ids, lp = model.generate(input_ids=batch["input_ids"].to(DEV), image_features=[f.to(DEV) for f in batch["image_features"]],
                                 attention_mask=batch["attention_mask"].to(DEV), do_sample=True, num_beams=1, top_k=0, top_p=1.0,
                                 return_logprobs=True, **kw)
        dec_in, mask, labels = labels_from_generated(ids, ocfg.pad_token_id, ocfg.eos_token_id)
        b = dict(batch, decoder_input_ids=dec_in, decoder_attention_mask=mask, labels=labels)
        train = float(run_fwd(model, b, loss_weights=torch.ones(B, device=DEV), loss_reduction="sum")[0])
        decode = -float(lp.sum_logprobs.sum())
        oracle = -float(_oracle_seq(ocfg, sd, batch, ids, grad=False)[1].sum())
    gap_train, gap_decode = abs(train - oracle), abs(decode - oracle)
    n_tokens = int((labels != -100).sum())
    print("sum of log-probabilities over %d tokens: training forward %.6f, sampler %.6f, oracle %.6f: gaps %.3e (training) %.3e (sampler)"
          % (n_tokens, train, decode, oracle, gap_train, gap_decode))
    # each side against the oracle: LOSS_TOL of one nat per token (the sums here are near zero -- a peaked model's likely sequences -- so the
    # bound is absolute: what LOSS_TOL allows a token whose loss is one nat)
    assert gap_train <= LOSS_TOL * n_tokens and gap_decode <= LOSS_TOL * n_tokens
    assert abs(train - decode) <= 2 * max(gap_train, gap_decode)
