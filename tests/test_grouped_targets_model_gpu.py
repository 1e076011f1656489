"""GPU: forward(..., targets_per_input=G) -- G target sequences per input, the encoder side run once -- against the CPU oracle on the inputs
replicated G-fold with repeat_interleave.

The reference is the oracle's autograd on the REPLICATED batch with the B * G targets (helpers of tests/test_loss_weights_model_gpu.py and
tests/test_label_smoothing_model_gpu.py); tolerances are the project's LOSS_TOL / GRAD_TOL (tests/test_model_gpu.py) and check_against's
per-class rules -- no new numbers.  (e) compares the grouped step with the product's own replicated step: both pass check_against, and their
direct difference is bounded by the triangle inequality over the two oracle bounds (2 LOSS_TOL, 2 GRAD_TOL).
"""
import ctypes as C
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from kmbart import _lib  # noqa: E402
from kmbart._lib import KmbAttn, KmbForwardOpts, KmbPretrain  # noqa: E402
from oracle import goldenlib as G  # noqa: E402
from src.data.synthetic import make_batch  # noqa: E402
from src.model.utils import labels_from_generated  # noqa: E402
from src.training import self_critical_step  # noqa: E402
import loss_weights_ref as W  # noqa: E402
from test_model_gpu import GRAD_TOL, LOSS_TOL, build, rel, run_fwd  # noqa: E402
from test_grad_accum_model_gpu import bits  # noqa: E402
from test_label_smoothing_model_gpu import FORM_BF16, FORM_FUSED, _grads, check_against, oracle_logits  # noqa: E402
from test_loss_weights_model_gpu import _oracle_seq, _reward, _same_bits_outside_tied, reference  # noqa: E402
from test_fp32_mode_gpu import FP32_TOL  # noqa: E402

DEV = "cuda:0"
HD = 64


def grouped_batch(B, G_, T, S=24, seed=1, full_rows=False):
    """B inputs (ragged regions / events, S tokens) and B * G_ targets of T tokens whose lengths differ inside a group; target row 1 is
    entirely -100 (an ignored sequence).  Returns the grouped batch and the batch replicated G_-fold for the oracle."""
    g = torch.Generator().manual_seed(seed)
    regions = torch.randint(0, 7, (B,), generator=g).tolist()
    ev = [int(torch.randint(1, S - 5 - r + 1, (1,), generator=g)) for r in regions]
    kw = dict(vocab_hi=G.TINY_SPECIAL_BASE, img_feat_id=G.TINY["img_feat_id"], special_base=G.TINY_SPECIAL_BASE)
    src = make_batch(B, enc_len=S, dec_len=T, regions=regions, event_lens=ev, label_lens=[T] * B, seed=seed, **kw)
    lens = [T] * (B * G_) if full_rows else torch.randint(3, T + 1, (B * G_,), generator=g).tolist()
    tgt = make_batch(B * G_, enc_len=8, dec_len=T, regions=[0] * (B * G_), event_lens=[1] * (B * G_), label_lens=lens, seed=seed + 1000, **kw)
    feats = G.golden_features(regions)
    b = dict(input_ids=src["input_ids"], attention_mask=src["attention_mask"], image_features=feats,
             decoder_input_ids=tgt["decoder_input_ids"], decoder_attention_mask=tgt["decoder_attention_mask"], labels=tgt["labels"].clone())
    if not full_rows:
        b["labels"][1] = -100
    rep = dict(b, input_ids=b["input_ids"].repeat_interleave(G_, 0), attention_mask=b["attention_mask"].repeat_interleave(G_, 0),
               image_features=[feats[i // G_] for i in range(B * G_)])
    return b, rep


def cross_route(B, H, Tq, Tk):
    """kmb_debug_attn_route of the step's cross-attention problem, forward and backward"""
    a = KmbAttn()
    d = H * HD
    for f in ("Q", "K", "V", "O", "lse", "dO", "dQ", "dK", "dV"):
        setattr(a, f, C.c_void_p(0x10000))
    a.ldq = a.ldo = a.lddo = a.lddq = d
    a.ldk = a.ldv = a.lddk = a.lddv = 2 * 2 * d   # Ld = 2 layers of k | v
    a.B, a.H, a.Tq, a.Tk, a.causal, a.dq_scale = B, H, Tq, Tk, 0, 0.125
    lib = _lib.load()
    return lib.kmb_debug_attn_route(C.byref(a), 0), lib.kmb_debug_attn_route(C.byref(a), 1)


def fwd_bwd(model, b, **kw):
    loss = run_fwd(model, b, **kw)[0]
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), _grads(model)


class Case:
    def __init__(self, ocfg, sd, B, G_, T, S=24, seed=1, full_rows=False):
        self.ocfg, self.sd, self.B, self.G, self.T, self.S = ocfg, sd, B, G_, T, S
        self.b, self.rep = grouped_batch(B, G_, T, S, seed, full_rows)
        self.w = W.seq_weights(B * G_)
        self.refs = {}

    def ref(self, weighted, reduction, eps=0.0):
        key = (weighted, reduction, eps)
        if key not in self.refs:
            self.refs[key] = reference(self.ocfg, self.sd, self.rep, self.w if weighted else None, reduction, eps)
        return self.refs[key]

    def model(self):
        return build(self.ocfg, self.sd).eval()


@pytest.fixture(scope="module")
def tiny():
    ocfg = G.tiny_config()
    return Case(ocfg, G.golden_state_dict(ocfg, seed=21), B=2, G_=5, T=16, seed=51)


@pytest.fixture(scope="module")
def fusedcase():
    ocfg = G.tiny_config(vocab_size=8150)
    return Case(ocfg, G.golden_state_dict(ocfg, seed=23), B=8, G_=4, T=32, seed=52)


# ------------------------------------------------------------------------------------------------ (a) tiny configuration, bf16 head
def test_a_tiny_against_the_oracle(tiny):
    c = tiny
    assert cross_route(c.B, 2, c.G * c.T, c.S) == (3, 3)   # Tq = 80: the query-streaming kernels
    model = c.model()
    loss = run_fwd(model, c.b, targets_per_input=c.G)[0]
    model._engine.check_inputs()
    assert model._engine.last_head_form() == FORM_BF16
    loss.backward()
    torch.cuda.synchronize()
    check_against(model, c.ref(False, "mean"), "tiny grouped mean", loss)
    w = c.w.to(DEV)
    assert bool((c.w > 0).any()) and bool((c.w < 0).any())
    loss = run_fwd(model, c.b, targets_per_input=c.G, loss_weights=w, loss_reduction="sum")[0]
    loss.backward()
    torch.cuda.synchronize()
    check_against(model, c.ref(True, "sum"), "tiny grouped weighted sum", loss)
    with torch.no_grad():
        loss_ng = run_fwd(model, c.b, targets_per_input=c.G, loss_weights=w, loss_reduction="sum")[0]
    assert abs(float(loss_ng) - c.ref(True, "sum")[0]) / abs(c.ref(True, "sum")[0]) < LOSS_TOL


# ------------------------------------------------------------------------------------------------ (b) the fused head
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_b_fused_head(fusedcase, eps):
    c = fusedcase
    assert c.B * c.G * c.T == 1024 and cross_route(c.B, 2, c.G * c.T, c.S) == (3, 3)
    model = c.model()
    model.label_smoothing = eps
    loss, _ = fwd_bwd(model, c.b, targets_per_input=c.G, loss_weights=c.w.to(DEV))
    model._engine.check_inputs()
    assert model._engine.last_head_form() == FORM_FUSED
    check_against(model, c.ref(True, "mean", eps), "fused grouped eps=%.1f" % eps, loss)


# ------------------------------------------------------------------------------------------------ (c) the other two attention routes
@pytest.mark.parametrize("which", ["single_tile", "general"])
def test_c_other_attention_routes(which):
    if which == "single_tile":   # Tq = G T = 64: the existing single-tile kernel
        ocfg = G.tiny_config()
        c = Case(ocfg, G.golden_state_dict(ocfg, seed=21), B=3, G_=2, T=32, S=24, seed=53)
        assert cross_route(c.B, 2, 64, c.S)[1] == 1
    else:                        # S = 70 keys: the general kernel
        ocfg = G.tiny_config(max_position_embeddings=128)
        c = Case(ocfg, G.golden_state_dict(ocfg, seed=21), B=2, G_=3, T=32, S=70, seed=54)
        assert cross_route(c.B, 2, 96, 70) == (0, 0)
    model = c.model()
    loss, _ = fwd_bwd(model, c.b, targets_per_input=c.G)
    check_against(model, c.ref(False, "mean"), "grouped, %s cross-attention" % which, loss)
    loss, _ = fwd_bwd(model, c.b, targets_per_input=c.G, loss_weights=c.w.to(DEV), loss_reduction="sum")
    check_against(model, c.ref(True, "sum"), "grouped weighted, %s cross-attention" % which, loss)


# ------------------------------------------------------------------------------------------------ (d) identity
@pytest.mark.parametrize("which", ["tiny", "fused"])
def test_d_none_and_one_are_identical(which):
    if which == "tiny":
        ocfg = G.tiny_config()
        c = Case(ocfg, G.golden_state_dict(ocfg, seed=21), B=2, G_=1, T=12, seed=55)
    else:
        ocfg = G.tiny_config(vocab_size=8150)
        c = Case(ocfg, G.golden_state_dict(ocfg, seed=23), B=32, G_=1, T=32, seed=56)
    model = c.model()
    l_none, g_none = fwd_bwd(model, c.b)
    _, g_none2 = fwd_bwd(model, c.b)
    assert model._engine.last_head_form() == (FORM_BF16 if which == "tiny" else FORM_FUSED)
    for tpi in (None, 1):
        l_one, g_one = fwd_bwd(model, c.b, targets_per_input=tpi)
        assert torch.equal(bits(l_one), bits(l_none)), (float(l_one), float(l_none))
        _same_bits_outside_tied(model._engine, g_one, g_none, g_none2)


# ------------------------------------------------------------------------------------------------ (e) against the replicated forward
def test_e_grouped_against_the_replicated_step(fusedcase):
    c = fusedcase
    model = c.model()
    ref = c.ref(True, "mean")
    w = c.w.to(DEV)
    l_g, g_g = fwd_bwd(model, c.b, targets_per_input=c.G, loss_weights=w)
    check_against(model, ref, "grouped", l_g)
    grads_g = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    l_r, g_r = fwd_bwd(model, c.rep, loss_weights=w)
    check_against(model, ref, "replicated", l_r)
    dl = abs(float(l_g) - float(l_r)) / abs(float(l_r))
    worst = ("", 0.0)
    for n, p in model.named_parameters():
        if float(ref[1][n].norm()) < 1e-6:
            continue
        e = rel(grads_g[n], p.grad)
        if e > worst[1]:
            worst = (n, e)
    print("grouped vs replicated: loss %.6f / %.6f (rel %.3e), worst gradient difference %.3e (%s)" % (float(l_g), float(l_r), dl, worst[1], worst[0]))
    assert dl < 2 * LOSS_TOL and worst[1] < 2 * GRAD_TOL


# ------------------------------------------------------------------------------------------------ (f) training mode with dropout
def test_f_training_mode_with_dropout(fusedcase):
    c = fusedcase
    out = []
    for _ in range(2):
        model = build(c.ocfg, c.sd, dropout=0.1, attention_dropout=0.1, activation_dropout=0.1).train()
        model._engine.set_seed(1234)
        loss, g = fwd_bwd(model, c.b, targets_per_input=c.G, loss_weights=c.w.to(DEV))
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(g).all())
        thr, _seed = model._engine.attention_dropout_site(2, 0)
        assert thr != 0
        out.append((loss, g, model._engine))
    (l1, g1, eng), (l2, g2, _) = out
    assert torch.equal(bits(l1), bits(l2))
    from test_grad_accum_model_gpu import tied_range
    lo, hi = tied_range(eng)
    same = bits(g1) == bits(g2)
    same[lo:hi] = True
    assert bool(same.all()), int((~same).sum())


# ------------------------------------------------------------------------------------------------ (g) refusals, before any launch
def test_g_refusals(tiny):
    model = tiny.model()
    eng = model._engine
    lib = eng.lib
    run_fwd(model, tiny.b, targets_per_input=tiny.G)   # binds a workspace
    torch.cuda.synchronize()
    ws = eng.workspace
    ws.fill_(0xA5)
    check_pattern = lambda: bool((ws == 0xA5).all())  # noqa: E731
    b, keep, _ = eng._batch(tiny.b["input_ids"], tiny.b["image_features"], tiny.b["attention_mask"], tiny.b["decoder_input_ids"],
                            tiny.b["decoder_attention_mask"], tiny.b["labels"])
    opts = KmbForwardOpts()
    opts.targets_per_input = 25            # G T = 400
    assert lib.kmb_forward_ex(eng.h, C.byref(b), C.byref(opts), 0, 0, None, None, None, None) != 0
    assert b"384" in lib.kmb_last_error()
    opts.targets_per_input = -1
    assert lib.kmb_forward_ex(eng.h, C.byref(b), C.byref(opts), 0, 0, None, None, None, None) != 0
    assert b"negative" in lib.kmb_last_error()
    opts.targets_per_input = 2
    ex = KmbPretrain(lm_factor=1.0, mrm_factor=1.0, attr_factor=1.0, rel_factor=1.0)
    assert lib.kmb_forward_pretrain_ex(eng.h, C.byref(b), C.byref(ex), C.byref(opts), 0, 0, None, None, None) != 0
    assert b"pre-training" in lib.kmb_last_error()
    torch.cuda.synchronize()
    assert check_pattern(), "a refused call wrote to the workspace"
    with pytest.raises(Exception, match="384"):
        run_fwd(model, dict(tiny.b, decoder_input_ids=tiny.b["decoder_input_ids"].repeat(5, 1), decoder_attention_mask=tiny.b["decoder_attention_mask"].repeat(5, 1),
                            labels=tiny.b["labels"].repeat(5, 1)), targets_per_input=25)


# ------------------------------------------------------------------------------------------------ (h) the fp32 validation mode
def test_h_fp32_validation_mode(tiny):
    c = tiny
    with torch.no_grad():
        _, ref_logits = oracle_logits(c.ocfg, c.sd, c.rep, grad=False)
    model = c.model()
    model._engine.set_precision(True)
    try:
        with torch.no_grad():
            logits = run_fwd(model, c.b, targets_per_input=c.G, return_logits=True)[1]
    finally:
        model._engine.set_precision(False)
    dm = c.b["decoder_attention_mask"].bool()
    assert tuple(logits.shape[:2]) == (c.B * c.G, c.T)
    e = rel(logits.cpu()[dm], ref_logits[dm])
    print("fp32 validation mode, grouped logits against the oracle on the replicated batch: %.3e" % e)
    assert e < FP32_TOL


# ------------------------------------------------------------------------------------------------ (i) self_critical_step
def test_i_self_critical_step_with_samples_per_input(gold_dir):
    gen = json.load(open(os.path.join(gold_dir, "tiny_generate.json")))
    ocfg, sd = G.tiny_config(), G.trained_state_dict()
    model = build(ocfg, sd).eval()
    batch = dict(input_ids=torch.tensor(gen["input_ids"]), attention_mask=torch.tensor(gen["attention_mask"]),
                 image_features=G.golden_features(gen["regions"], seed=gen["seed"]))
    B, Gs = batch["input_ids"].shape[0], 4
    rep = dict(input_ids=batch["input_ids"].repeat_interleave(Gs, 0), attention_mask=batch["attention_mask"].repeat_interleave(Gs, 0),
               image_features=[batch["image_features"][i // Gs] for i in range(B * Gs)])
    kw = dict(max_length=12, min_length=0, temperature=3.0)   # (temperature: test_h_self_critical_step's reasoning)
    torch.manual_seed(21)
    loss, info = self_critical_step(model, batch, _reward, DEV, baseline="mean", sample_kwargs=kw, samples_per_input=Gs)
    loss.backward()   # (before model.score below: a score is a forward of its own and ends this one's pending backward)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    loss = loss.detach()
    r, A = info["rewards"].cpu(), info["advantages"].cpu()
    assert r.shape == (B * Gs,) and info["sample_ids"].shape[0] == B * Gs
    assert torch.equal(r, _reward(info["sample_ids"].cpu()))
    want_A = torch.empty(B * Gs, dtype=torch.float64)
    for i in range(B):
        for j in range(Gs):
            want_A[i * Gs + j] = float(r[i * Gs + j]) - sum(float(r[i * Gs + k]) for k in range(Gs) if k != j) / (Gs - 1)
    assert float((A.double() - want_A).abs().max()) <= 16 * 2.0 ** -24 * float(r.abs().max()) * Gs
    # the loss: - sum_i A_i log p_i / (B G), log p_i from model.score on the replicated batch
    dec_in, mask, labels = labels_from_generated(info["sample_ids"], ocfg.pad_token_id, ocfg.eos_token_id)
    with torch.no_grad():
        sc = model.score(input_ids=rep["input_ids"].to(DEV), image_features=[f.to(DEV) for f in rep["image_features"]],
                         attention_mask=rep["attention_mask"].to(DEV), decoder_input_ids=dec_in, decoder_attention_mask=mask, labels=labels)
    logp = -sc.nll.cpu().double()
    want = -(A.double() * logp).sum() / (B * Gs)
    scale = float((A.double().abs() * logp.abs()).sum() / (B * Gs))
    print("grouped self-critical step: loss %.6f, from model.score %.6f, scale %.4f" % (float(loss), float(want), scale))
    assert scale > 0.5, "the relative bound needs a scale far from zero"
    assert abs(float(loss) - float(want)) <= LOSS_TOL * scale, (float(loss), float(want), scale)
    # ... and against the oracle's teacher-forced log-probabilities on the replicated batch (test_h_self_critical_step's rule)
    with torch.no_grad():
        _, ologp = _oracle_seq(ocfg, sd, rep, info["sample_ids"], grad=False)
    owant = -(A * ologp).sum() / (B * Gs)
    assert abs(float(loss) - float(owant)) <= LOSS_TOL * scale, (float(loss), float(owant), scale)
    # the greedy baseline: one greedy reward per input, broadcast over its samples
    torch.manual_seed(22)
    loss, info = self_critical_step(model, batch, _reward, DEV, baseline="greedy", sample_kwargs=kw, samples_per_input=Gs)
    assert info["greedy_ids"].shape[0] == B and info["baseline"].shape == (B * Gs,)
    assert torch.equal(info["baseline"].cpu(), _reward(info["greedy_ids"].cpu().repeat_interleave(Gs, 0)))
    assert bool(torch.isfinite(loss))


def test_i_self_critical_step_with_the_device_reward_repeated(gold_dir):
    """... with CiderReward.for_batch(batch, repeats=G) as the reward: what _self_critical_fine_tune and vcg_train.py --sc_samples run.  The
    fixtures are tests/test_cider_reward_model_gpu.py's (the trained tiny model, references made from its greedy decode).  Row i of the B * G
    samples is scored against item i // G: checked against the table-side restatement (tests/cider_ref.py) within the kernel's bound."""
    import math
    import random
    import cider_ref as R
    from src.rewards import CiderReward, reward_tokens
    gen = json.load(open(os.path.join(gold_dir, "tiny_generate.json")))
    ocfg, sd = G.tiny_config(), G.trained_state_dict()
    pad, bos, eos = ocfg.pad_token_id, ocfg.bos_token_id, ocfg.eos_token_id
    model = build(ocfg, sd).eval()
    B, Gs = len(gen["input_ids"]), 4
    rng = random.Random(2)
    words = list(range(10, 80))
    groups = []
    for row in gen["cases"][0]["ids"]:
        t = reward_tokens(row, pad, bos, eos)
        groups.append([t, R.edit(t, rng, words), R.edit(R.edit(t, rng, words), rng, words)])
    keys = [(50 + b, "intent") for b in range(B)]
    rew = CiderReward(groups, ocfg.vocab_size, pad, bos, eos, device=DEV, group_keys=keys)
    tab = R.TableReference(rew.tables)
    batch = dict(input_ids=torch.tensor(gen["input_ids"]), attention_mask=torch.tensor(gen["attention_mask"]),
                 image_features=G.golden_features(gen["regions"], seed=gen["seed"]), index=[k[0] for k in keys], task_type=[k[1] for k in keys])
    torch.manual_seed(23)
    loss, info = self_critical_step(model, batch, rew.for_batch(batch, repeats=Gs), DEV, baseline="mean",
                                    sample_kwargs=dict(max_length=12, min_length=0, temperature=1.5), samples_per_input=Gs)
    got = info["rewards"]
    assert got.dtype == torch.float32 and got.device.type == "cuda" and got.shape == (B * Gs,)
    assert info["sample_ids"].shape[0] == B * Gs and "greedy_ids" not in info
    rows, r = info["sample_ids"].cpu().tolist(), got.double().cpu()
    for i in range(B * Gs):
        t = reward_tokens(rows[i], pad, bos, eos)
        want = tab.score(t, i // Gs, "D")     # row i against item i // G
        assert abs(float(r[i]) - want) <= R.bound(want, len(t), 3), (i, float(r[i]), want)
    print("grouped CIDEr-D rewards: %s" % ["%.4f" % float(x) for x in r])
    assert float(r.max()) > 0.0, "no sample resembles its references: the check says nothing"
    A = info["advantages"].double().cpu()
    want_A = torch.empty(B * Gs, dtype=torch.float64)
    for i in range(B):
        for j in range(Gs):
            want_A[i * Gs + j] = float(r[i * Gs + j]) - sum(float(r[i * Gs + k]) for k in range(Gs) if k != j) / (Gs - 1)
    assert float((A - want_A).abs().max()) <= 16 * 2.0 ** -24 * max(float(r.abs().max()), 1.0) * Gs   # fp32: a sum of G rewards and a division
    assert float(A.view(B, Gs).sum(dim=1).abs().max()) <= 32 * 2.0 ** -24 * max(float(r.abs().max()), 1.0) * Gs
    assert math.isfinite(float(loss.detach()))
    loss.backward()
    torch.cuda.synchronize()
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert grads and all(bool(torch.isfinite(g).all()) for g in grads)


# ------------------------------------------------------------------------------------------------ (j) accumulation
def _inputs_slice(b, lo, hi, G_):
    out = dict(b)
    for k in ("input_ids", "attention_mask"):
        out[k] = b[k][lo:hi]
    out["image_features"] = b["image_features"][lo:hi]
    for k in ("decoder_input_ids", "decoder_attention_mask", "labels"):
        out[k] = b[k][lo * G_:hi * G_]
    return out


def test_j_two_grouped_micro_batches_accumulate(fusedcase):
    c = fusedcase
    ref = c.ref(True, "sum")
    model = c.model()
    model.accumulate_gradients(True)
    model.zero_grad()
    total = 0.0
    for lo, hi in ((0, c.B // 2), (c.B // 2, c.B)):
        loss = run_fwd(model, _inputs_slice(c.b, lo, hi, c.G), targets_per_input=c.G, loss_weights=c.w[lo * c.G:hi * c.G].to(DEV), loss_reduction="sum")[0]
        loss.backward()
        total += float(loss)
    torch.cuda.synchronize()
    model.accumulate_gradients(False)
    assert abs(total - ref[0]) / abs(ref[0]) < LOSS_TOL, (total, ref[0])
    check_against(model, ref, "two grouped micro-batches, sum")
