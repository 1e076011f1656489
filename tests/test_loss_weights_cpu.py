"""CPU: per-row loss weights -- the references of tests/loss_weights_ref.py against torch autograd, the emulation's figures at the GPU
tests' shape with mixed-sign weights, the kmb_forward_opts layout, labels_from_generated against the reference's sent_lengths loop,
self_critical_step on a stub model, and the forward's two refusals.

Measured here (float64, CPU) at loss_ref.FUSED (M = 1024, V = 8150, Vpad = 8192, d = 128, every seventh label -100) with
row_weights() = (1.75, -0.5, 0.75, 1.25)[r % 4] * (1 + 0.5 * (r // 4 % 2)), "mean", emulation against float64 reference: the figures
recorded in loss_weights_ref.EMU_W.  A recorded figure below its measurement, or more than 10 % above it, fails."""
import ctypes as C
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import label_smoothing_ref as L  # noqa: E402
import loss_ref as R  # noqa: E402
import loss_weights_ref as W  # noqa: E402


def _holds(measured, recorded, what):
    print("%-40s measured %.4e  recorded %.4e" % (what, measured, recorded))
    assert measured <= recorded, (what, measured, recorded)
    assert recorded <= 1.1 * measured, (what, "recorded figure is more than 10 % above the measurement", measured, recorded)


# ------------------------------------------------------------------------------------------------ references
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_references_agree_with_torch_autograd(eps, reduction):
    """w_rows / w_grad are sum_r w_r F.cross_entropy(reduction='none')_r / D and its gradient; a NaN weight on an ignored row is not read"""
    g = torch.Generator().manual_seed(1)
    x = torch.randn(11, 40, generator=g, dtype=torch.float64).requires_grad_(True)   # 37 real columns, 3 pad
    labels = torch.randint(0, 37, (11,), generator=g)
    labels[3] = R.IGNORE
    w = W.row_weights(11)
    per_row = F.cross_entropy(x[:, :37], labels, ignore_index=R.IGNORE, label_smoothing=eps, reduction="none")
    n = int((labels != R.IGNORE).sum())
    loss = 2.5 * (R.f64(w) * per_row).sum() / (n if reduction == "mean" else 1)
    loss.backward()
    w_nan = w.clone()
    w_nan[3] = float("nan")
    rows, ok = W.w_rows(x.detach(), labels, 37, eps, w_nan)
    assert torch.allclose(W.w_loss(rows, ok, reduction) * 2.5, loss.detach(), rtol=1e-12)
    grad, big = W.w_grad(x.detach(), labels, 37, 2.5, eps, w_nan, reduction)
    assert torch.allclose(grad, x.grad[:, :37], rtol=1e-10, atol=1e-15)
    assert bool((big >= grad.abs() - 1e-18).all())
    assert float(grad[3].abs().max()) == 0.0 and float(rows[3]) == 0.0
    assert bool((w < 0).any()) and float(W.w_loss(*W.w_rows(x.detach(), labels.fill_(R.IGNORE), 37, eps, w), "sum")) == 0.0


@pytest.fixture(scope="module")
def case():
    return R.fused_case()


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_dense_reference_against_autograd_and_its_own_factors(case, eps):
    H, E, bias, labels = case
    c = R.FUSED
    w = W.row_weights(c["M"])
    ref = W.fused_w_ref(H, E, bias, labels, c["V"], c["lm_factor"], eps, w)
    Hd, Ed, bd = R.f64(H).requires_grad_(True), R.f64(E[: c["V"]]).requires_grad_(True), R.f64(bias)
    per_row = F.cross_entropy(Hd @ Ed.t() + bd, labels, ignore_index=R.IGNORE, label_smoothing=eps, reduction="none")
    loss = c["lm_factor"] * (R.f64(w) * per_row).sum() / int(ref["ok"].sum())
    loss.backward()
    assert R.rel_norm(ref["dH"], Hd.grad) < 1e-12 and R.rel_norm(ref["dE"], Ed.grad) < 1e-12
    assert abs(float(c["lm_factor"] * W.w_loss(ref["loss_rows"], ref["ok"], "mean") - loss.detach())) < 1e-12 * abs(float(loss.detach()))
    # "sum" is "mean" times the valid count
    ref_s = W.fused_w_ref(H, E, bias, labels, c["V"], c["lm_factor"], eps, w, "sum")
    n = int(ref["ok"].sum())
    assert R.rel_norm(ref_s["dH"], ref["dH"] * n) < 1e-14 and R.rel_norm(ref_s["alpha"], ref["alpha"] * n) < 1e-14


# ------------------------------------------------------------------------------------------------ the emulation's figures
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_unit_weights_reproduce_the_unweighted_emulation(case, eps):
    H, E, bias, labels = case
    c = R.FUSED
    e0 = L.emu_fused_ls(H, E, bias, labels, c["V"], c["lm_factor"], eps)
    e = W.emu_fused_w(H, E, bias, labels, c["V"], c["lm_factor"], eps, torch.ones(c["M"]))
    for k in ("dH", "dE", "loss_rows", "Pl", "aH", "alpha", "beta", "u"):
        assert torch.equal(e0[k], e[k]), k


@pytest.mark.parametrize("eps", sorted(W.EMU_W))
def test_emulation_figures(case, eps):
    H, E, bias, labels = case
    c = R.FUSED
    w = W.row_weights(c["M"])
    ref = W.fused_w_ref(H, E, bias, labels, c["V"], c["lm_factor"], eps, w)
    emu = W.emu_fused_w(H, E, bias, labels, c["V"], c["lm_factor"], eps, w)
    ok = ref["ok"]
    assert bool((w[ok] < 0).any()) and bool((w[ok] > 0).any()) and len(set(w.tolist())) == 8
    # gradient elements: the float64 row rounded once (the two-kernel path), and the fused a . P' (nothing but P's and the label entry's
    # rounding), within 2^-8 of |w_r| times the larger operand
    assert bool(((R.rb(ref["G"]) - ref["G"]).abs() <= R.EMU_ONE_ROUNDING * ref["big"]).all())
    aP = emu["aP"][:, : c["V"]]
    if eps == 0.0:
        assert bool(((aP - ref["G"]).abs() <= R.EMU_ONE_ROUNDING * ref["big"]).all())
    # dH: a row scale cancels in a row's relative norm.  That holds exactly for everything in front of the row's one bf16 rounding -- the
    # rows' relative errors of alpha P' E - beta wsum are the unweighted ones -- and the rounding itself lands elsewhere on w x than on x
    # (the weights are no powers of two), so the figure behind it is measured like the others.
    un_ref = L.fused_ls_ref(H, E, bias, labels, c["V"], c["lm_factor"], eps)
    un_emu = W.emu_fused_w(H, E, bias, labels, c["V"], c["lm_factor"], eps, torch.ones(c["M"]))
    pre_w = (emu["dH_pre"] - ref["dH"]).norm(dim=1)[ok] / ref["dH"].norm(dim=1)[ok]
    pre_1 = (un_emu["dH_pre"] - un_ref["dH"]).norm(dim=1)[ok] / un_ref["dH"].norm(dim=1)[ok]
    # (1e-6: beta is held in fp32 with and without the weight, one rounding of a term far below the row's norm)
    assert torch.allclose(pre_w, pre_1, rtol=1e-6, atol=0.0), float((pre_w - pre_1).abs().max())
    worst, whole = R.row_rel_norms(emu["dH"], ref["dH"])
    print("eps %.1f dH worst row: weighted %.4e, unweighted %.4e" % (eps, worst, R.row_rel_norms(un_emu["dH"], un_ref["dH"])[0]))
    fig = W.EMU_W[eps]
    _holds(worst, fig["dH_worst"], "eps %.1f weighted dH worst row" % eps)
    _holds(whole, fig["dH_matrix"], "eps %.1f weighted dH matrix" % eps)
    worst, whole = R.row_rel_norms(emu["dE"], ref["dE"])
    _holds(worst, fig["dE_worst"], "eps %.1f weighted dE worst row" % eps)
    _holds(whole, fig["dE_matrix"], "eps %.1f weighted dE matrix" % eps)
    row_err = float((emu["loss_rows"] - ref["loss_rows"]).abs().max())
    if eps == 0.0:
        _holds(row_err, W.EMU_W_ROW_LOSS_ABS, "eps 0.0 weighted row loss, absolute")
    assert row_err <= W.EMU_W_ROW_LOSS_ABS, row_err
    # weight-free by construction: the stored matrix, its row sums and the label's entry
    for k in ("P", "Pl", "S"):
        assert torch.equal(emu[k], un_emu[k]), k
    assert float(emu["dH"][~ok].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ the library, without a GPU
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from kmbart import _lib
    return _lib.load()


def test_forward_opts_layout(lib):
    from kmbart._lib import KmbForwardOpts
    assert C.sizeof(KmbForwardOpts) == lib.kmb_abi_sizeof_forward_opts()
    names = [f[0] for f in KmbForwardOpts._fields_]
    assert names[:3] == ["encoder_states", "decoder_states_out", "skip_head"], "the existing fields keep their places"
    assert names[-2:] == ["row_weights", "loss_reduction"], "the appended fields come last"
    assert KmbForwardOpts.row_weights.offset > KmbForwardOpts.skip_head.offset
    assert KmbForwardOpts.loss_reduction.offset == KmbForwardOpts.row_weights.offset + C.sizeof(C.c_void_p)
    z = KmbForwardOpts()
    assert not z.row_weights and z.loss_reduction == 0


def test_op_entry_points_refuse_bad_arguments(lib):
    """before any launch: no device pointer is touched (these run without a GPU)"""
    p = C.c_void_p(16)
    assert lib.kmb_op_ce_weighted(p, 8, 8, p, 1, 1.0, 0.0, None, 2, p, None, p, p, None) != 0
    assert b"reduction" in lib.kmb_last_error()
    assert lib.kmb_op_ce_bf16_weighted(p, 8, 8, p, 1, 1.0, 1.0, None, 0, p, None, p, p, None, None) != 0
    assert b"eps" in lib.kmb_last_error()
    assert lib.kmb_op_ce_rows_finish_weighted(p, 4, 4, None, None, p, p, 1.0, 0.0, None, 3, 1, 8, 8, None, 8, None, p, p, p, None, None, None,
                                              8, None, None, None) != 0
    assert b"reduction" in lib.kmb_last_error()


# ------------------------------------------------------------------------------------------------ labels_from_generated
PAD, BOS, EOS = 1, 0, 2


def _reference_sent_lengths(ids):
    """the reference's loop, restated (reference src/model/utils.py:11-54): sent_lengths starts at max_length; the step that adds a row's
    first EOS stores the length including it; logprobs[i, sent_lengths[i] - 1:] = 0"""
    B, max_length = ids.shape
    unfinished = [1] * B
    sent_lengths = [max_length] * B
    cur_len = 1
    while cur_len < max_length:
        tokens = [int(ids[i, cur_len]) for i in range(B)]
        cur_len += 1
        for i in range(B):
            if unfinished[i] and tokens[i] == EOS:
                sent_lengths[i] = cur_len
            if tokens[i] == EOS:
                unfinished[i] = 0
    keep = torch.ones(B, max_length - 1, dtype=torch.bool)
    for i in range(B):
        keep[i, sent_lengths[i] - 1:] = False
    return keep


def test_labels_from_generated():
    from src.model.utils import labels_from_generated
    ids = torch.tensor([
        [BOS, EOS, PAD, PAD, PAD, PAD],     # EOS first
        [BOS, 7, 8, 9, 10, EOS],            # EOS last
        [BOS, 7, 8, 9, 10, 11],             # no EOS
        [BOS, 7, EOS, 9, EOS, PAD],         # a second EOS behind the first
        [BOS, 7, 8, EOS, PAD, PAD],         # pad behind the EOS
        [BOS, PAD, PAD, PAD, PAD, PAD],     # a pad row without any EOS: the reference's rule keeps all of it
    ])
    dec_in, mask, labels = labels_from_generated(ids, PAD, EOS)
    keep = _reference_sent_lengths(ids)
    assert torch.equal(dec_in, ids[:, :-1]) and dec_in.is_contiguous()
    assert torch.equal(labels, torch.where(keep, ids[:, 1:], torch.full_like(ids[:, 1:], -100)))
    assert torch.equal(mask, keep.long())
    assert labels[0].tolist() == [EOS, -100, -100, -100, -100]
    assert labels[1].tolist() == [7, 8, 9, 10, EOS]
    assert labels[3].tolist() == [7, EOS, -100, -100, -100]
    assert int(mask.sum(1).min()) >= 1, "no row is masked out entirely"
    # pad_to_multiple_of: T = 5 -> 8, pad ids, mask 0, labels -100; a multiple that already divides T changes nothing
    d8, m8, l8 = labels_from_generated(ids, PAD, EOS, pad_to_multiple_of=8)
    assert d8.shape == (6, 8) and torch.equal(d8[:, :5], dec_in) and bool((d8[:, 5:] == PAD).all())
    assert torch.equal(l8[:, :5], labels) and bool((l8[:, 5:] == -100).all())
    assert torch.equal(m8[:, :5], mask) and bool((m8[:, 5:] == 0).all())
    d5, m5, l5 = labels_from_generated(ids, PAD, EOS, pad_to_multiple_of=5)
    assert torch.equal(d5, dec_in) and torch.equal(l5, labels) and torch.equal(m5, mask)


# ------------------------------------------------------------------------------------------------ self_critical_step on a stub
class _StubModel:
    class config:
        pad_token_id, eos_token_id = PAD, EOS

    def __init__(self):
        self.generate_calls, self.forward_calls = [], []
        self.sample = torch.tensor([[BOS, 7, 8, EOS, PAD], [BOS, 9, EOS, PAD, PAD], [BOS, 5, 6, 7, 8]])
        self.greedy = torch.tensor([[BOS, 7, EOS], [BOS, 9, 9], [BOS, EOS, PAD]])

    def generate(self, **kw):
        assert not torch.is_grad_enabled(), "generate runs under no_grad"
        self.generate_calls.append(kw)
        return self.sample if kw.get("do_sample") else self.greedy

    def forward(self, **kw):
        assert torch.is_grad_enabled(), "the training forward runs with grad enabled"
        self.forward_calls.append(kw)
        return (torch.tensor(3.5), None, None)


def _reward(ids):
    return 0.5 + torch.arange(ids.shape[0], dtype=torch.float32) + 0.25 * (ids != PAD).sum(1).float()


@pytest.mark.parametrize("baseline", ["greedy", None, "tensor"])
def test_self_critical_step_on_a_stub(baseline):
    from src.training import self_critical_step
    m = _StubModel()
    batch = dict(input_ids=torch.zeros(3, 4, dtype=torch.long), image_features=[torch.zeros(2, 8)] * 3,
                 attention_mask=torch.ones(3, 4, dtype=torch.long))
    given = torch.tensor([0.25, -1.0, 2.0])
    loss, info = self_critical_step(m, batch, _reward, torch.device("cpu"), baseline=given if baseline == "tensor" else baseline,
                                    sample_kwargs=dict(max_length=5, pad_to_multiple_of=8))
    assert float(loss) == 3.5
    # the sampling call: unfiltered one-beam sampling; the greedy call only for the greedy baseline
    s = m.generate_calls[0]
    assert s["do_sample"] is True and s["num_beams"] == 1 and s["top_k"] == 0 and s["top_p"] == 1.0 and s["max_length"] == 5
    assert "pad_to_multiple_of" not in s and torch.equal(s["input_ids"], batch["input_ids"])
    if baseline == "greedy":
        assert len(m.generate_calls) == 2
        gk = m.generate_calls[1]
        assert gk["do_sample"] is False and gk["num_beams"] == 1 and gk["max_length"] == 5 and "top_k" not in gk and "top_p" not in gk
        base = _reward(m.greedy)
        assert torch.equal(info["greedy_ids"], m.greedy)
    else:
        assert len(m.generate_calls) == 1
        base = torch.zeros(3) if baseline is None else given
    rewards = _reward(m.sample)
    assert torch.equal(info["rewards"], rewards) and torch.equal(info["advantages"], rewards - base) and torch.equal(info["baseline"], base)
    assert torch.equal(info["sample_ids"], m.sample)
    (f,) = m.forward_calls
    assert f["loss_reduction"] == "sum" and torch.equal(f["loss_weights"], (rewards - base) / 3)
    assert f["labels"].shape == (3, 8) and f["labels"][0].tolist() == [7, 8, EOS, -100, -100, -100, -100, -100]
    assert f["labels"][2].tolist()[:4] == [5, 6, 7, 8] and f["decoder_input_ids"][0].tolist() == [BOS, 7, 8, EOS, PAD, PAD, PAD, PAD]
    assert torch.equal(f["decoder_attention_mask"], (f["labels"] != -100).long())
    with pytest.raises(ValueError):
        self_critical_step(m, batch, _reward, torch.device("cpu"), sample_kwargs=dict(top_k=50))
    with pytest.raises(ValueError):
        self_critical_step(m, batch, _reward, torch.device("cpu"), baseline="beam")


# ------------------------------------------------------------------------------------------------ the forward's refusals
def test_forward_refuses_weights_without_labels_and_an_unknown_reduction():
    """both are raised before the engine is touched -- but behind the check that there is an engine, so the model gets a stand-in"""
    from src.model.config import MultiModalBartConfig
    from src.model.model import MultiModalBartForConditionalGeneration, MultiModalBartForPreTraining
    from oracle import goldenlib as G
    ids = torch.zeros(2, 4, dtype=torch.long)
    for cls in (MultiModalBartForConditionalGeneration, MultiModalBartForPreTraining):
        m = cls(MultiModalBartConfig.from_dict(dict(G.TINY)))
        m._engine = object()
        with pytest.raises(ValueError, match="labels"):
            m.forward(ids, [], decoder_input_ids=ids, loss_weights=torch.ones(2))
        with pytest.raises(ValueError, match="loss_reduction"):
            m.forward(ids, [], decoder_input_ids=ids, labels=ids, loss_reduction="batchmean")
