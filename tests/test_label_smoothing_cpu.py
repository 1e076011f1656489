"""CPU: label smoothing -- the references of tests/label_smoothing_ref.py against torch autograd, the rank-one form the kernels use against
the dense form, the emulation's figures at the GPU tests' shape, the setter's refusals through the library, and the two command-line flags.

Measured here (float64, CPU) at loss_ref.FUSED (M = 1024, V = 8150, Vpad = 8192, d = 128, every seventh label -100), emulation against
float64 reference: eps = 0.1 row loss 1.34e-7 absolute, dH worst row 4.22e-3 / matrix 2.33e-3, dE worst row 4.29e-3 / matrix 2.34e-3;
eps = 0.3 dH 4.26e-3 / 2.31e-3, dE 4.41e-3 / 2.34e-3; eps = 0 reproduces loss_ref.emu_fused bit for bit (4.12e-3 / 2.34e-3 / 4.38e-3 /
2.37e-3).  A figure that no longer holds, or that has grown slack (more than 1.5 x the measurement), fails."""
import ctypes as C
import math
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
from test_attention_dropout_cpu import VCG_BASE  # noqa: E402


def _holds(measured, recorded, what):
    print("%-40s measured %.4e  recorded %.4e" % (what, measured, recorded))
    assert measured <= recorded, (what, measured, recorded)
    assert recorded <= 1.5 * measured, (what, "recorded figure is slack", measured, recorded)


# ------------------------------------------------------------------------------------------------ references
@pytest.mark.parametrize("eps", [0.0, 0.1, 0.3])
def test_references_agree_with_torch_autograd(eps):
    """ls_rows / ls_grad are F.cross_entropy(ignore_index=-100, label_smoothing=eps) and its gradient; out-of-range labels count as ignored"""
    g = torch.Generator().manual_seed(1)
    x = torch.randn(11, 40, generator=g, dtype=torch.float64).requires_grad_(True)   # 37 real columns, 3 pad
    labels = torch.randint(0, 37, (11,), generator=g)
    labels[3] = R.IGNORE
    loss = F.cross_entropy(x[:, :37], labels, ignore_index=R.IGNORE, label_smoothing=eps) * 2.5
    loss.backward()
    rows, ok = L.ls_rows(x.detach(), labels, 37, eps)
    assert torch.allclose(R.ce_mean(rows, ok) * 2.5, loss.detach(), rtol=1e-12)
    grad, big = L.ls_grad(x.detach(), labels, 37, 2.5, eps)
    assert torch.allclose(grad, x.grad[:, :37], rtol=1e-10, atol=1e-15)
    assert bool((big >= grad.abs() - 1e-18).all())
    assert float(grad[3].abs().max()) == 0.0 and float(rows[3]) == 0.0
    labels2 = labels.clone()
    labels2[5] = 37                       # out of range: treated as ignored, not counted
    rows2, ok2 = L.ls_rows(x.detach(), labels2, 37, eps)
    assert not bool(ok2[5]) and float(rows2[5]) == 0.0 and int(ok2.sum()) == int(ok.sum()) - 1
    if eps == 0.0:
        assert torch.equal(rows, R.ce_rows(x.detach(), labels, 37)[0])


@pytest.fixture(scope="module")
def case():
    return R.fused_case()


@pytest.mark.parametrize("eps", [0.1, 0.3])
def test_rank_one_form_equals_dense_form(case, eps):
    """zbar = (h . wsum + bsum) / V, the onehot part inside the matrix, beta wsum and u outside: float64, nothing rounded"""
    H, E, bias, labels = case
    c = R.FUSED
    ref = L.fused_ls_ref(H, E, bias, labels, c["V"], c["lm_factor"], eps)
    r1 = L.fused_ls_rank_one(H, E, bias, labels, c["V"], c["lm_factor"], eps)
    assert float((r1["loss_rows"] - ref["loss_rows"]).abs().max()) < 1e-13
    assert R.rel_norm(r1["dH"], ref["dH"]) < 1e-13 and R.rel_norm(r1["dE"], ref["dE"]) < 1e-13
    # and against autograd of the criterion itself on the dense logits
    Hd, Ed, bd = R.f64(H).requires_grad_(True), R.f64(E[: c["V"]]).requires_grad_(True), R.f64(bias)
    loss = c["lm_factor"] * F.cross_entropy(Hd @ Ed.t() + bd, labels, ignore_index=R.IGNORE, label_smoothing=eps)
    loss.backward()
    assert R.rel_norm(ref["dH"], Hd.grad) < 1e-12 and R.rel_norm(ref["dE"], Ed.grad) < 1e-12
    assert abs(float(c["lm_factor"] * R.ce_mean(ref["loss_rows"], ref["ok"]) - loss.detach())) < 1e-12 * abs(float(loss.detach()))


# ------------------------------------------------------------------------------------------------ the emulation's figures
def test_emulation_at_eps_zero_is_loss_ref(case):
    H, E, bias, labels = case
    c = R.FUSED
    e0 = R.emu_fused(H, E, bias, labels, c["V"], c["lm_factor"])
    e = L.emu_fused_ls(H, E, bias, labels, c["V"], c["lm_factor"], 0.0)
    for k in ("dH", "dE", "loss_rows", "Pl", "aH"):
        assert torch.equal(e0[k], e[k]), k
    ref = R.fused_ref(H, E, bias, labels, c["V"], c["lm_factor"])
    worst, whole = R.row_rel_norms(e["dH"], ref["dH"])
    _holds(worst, R.EMU_DH_WORST_ROW, "eps 0 dH worst row")
    _holds(whole, R.EMU_DH_MATRIX, "eps 0 dH matrix")
    worst, whole = R.row_rel_norms(e["dE"], ref["dE"])
    _holds(worst, R.EMU_DE_WORST_ROW, "eps 0 dE worst row")
    _holds(whole, R.EMU_DE_MATRIX, "eps 0 dE matrix")


@pytest.mark.parametrize("eps", sorted(L.EMU_LS))
def test_emulation_figures(case, eps):
    H, E, bias, labels = case
    c = R.FUSED
    ref = L.fused_ls_ref(H, E, bias, labels, c["V"], c["lm_factor"], eps)
    emu = L.emu_fused_ls(H, E, bias, labels, c["V"], c["lm_factor"], eps)
    fig = L.EMU_LS[eps]
    worst, whole = R.row_rel_norms(emu["dH"], ref["dH"])
    _holds(worst, fig["dH_worst"], "eps %.1f dH worst row" % eps)
    _holds(whole, fig["dH_matrix"], "eps %.1f dH matrix" % eps)
    worst, whole = R.row_rel_norms(emu["dE"], ref["dE"])
    _holds(worst, fig["dE_worst"], "eps %.1f dE worst row" % eps)
    _holds(whole, fig["dE_matrix"], "eps %.1f dE matrix" % eps)
    if eps == 0.1:
        _holds(float((emu["loss_rows"] - ref["loss_rows"]).abs().max()), L.EMU_LS_ROW_LOSS_ABS, "eps 0.1 row loss, absolute")
    # the smoothing term is visible in the rows: the GPU test's 3e-4 on a row loss would not pass a kernel that forgot it
    rows0 = L.ls_rows(ref["v"], labels, c["V"], 0.0)[0]
    assert float((ref["loss_rows"] - rows0).abs().max()) > 0.05
    assert float(emu["dH"][~ref["ok"]].abs().max()) == 0.0
    # the label's entry: one bf16 rounding of 1 - (1 - eps) S
    rix = torch.arange(c["M"])[ref["ok"]]
    lab = labels[ref["ok"]]
    assert torch.equal(emu["Pl"][rix, lab], R.rb(1.0 - (1.0 - eps) * emu["S"][ref["ok"]]))


def test_one_rounding_of_the_smoothed_gradient_row():
    """the two-kernel path with eps: the float64 row rounded once is within 2^-8 of the LARGER operand of the subtraction everywhere, and
    no bound relative to the difference itself can hold (softmax meets eps / V within a factor of a few somewhere in every row)"""
    V, ld, eps = 8150, 8192, 0.1
    x, labels = R.ce_case(V, ld, 9, seed=V, bf16=True, pad_value=0.0)
    ref, big = L.ls_grad(x, labels, V, 3.0, eps)
    emu = L.emu_ls_grad(x, labels, V, 3.0, eps)
    assert bool(((emu - ref).abs() <= R.BF16_ROUND * big).all())
    nz = ref != 0
    assert float((big[nz] / ref.abs()[nz]).max()) > 100.0      # cancellation: |p - eps / V| far below max(p, eps / V) somewhere


# ------------------------------------------------------------------------------------------------ the library, without a GPU
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from kmbart import _lib
    return _lib.load()


def test_setter_takes_eps_in_the_half_open_unit_interval(lib):
    from kmbart._lib import KmbConfig, check
    h = C.c_void_p()
    check(lib.kmb_create(C.byref(KmbConfig(**VCG_BASE)), C.byref(h)))
    try:
        assert lib.kmb_last_head_form(h) == -1
        for ok in (0.0, 0.1, 0.999):
            assert lib.kmb_set_label_smoothing(h, ok) == 0, ok
        for bad in (-0.1, 1.0, 1.5, math.nan, math.inf):
            assert lib.kmb_set_label_smoothing(h, bad) != 0, bad
            assert b"kmb_set_label_smoothing" in lib.kmb_last_error(), bad
        assert lib.kmb_set_label_smoothing(None, 0.1) != 0
        assert b"kmb_set_label_smoothing" in lib.kmb_last_error()
        assert lib.kmb_last_head_form(None) == -1
    finally:
        lib.kmb_destroy(h)


def test_structs_keep_their_layout(lib):
    from kmbart._lib import KmbBatch, KmbConfig, KmbGemm, KmbPretrain
    assert C.sizeof(KmbConfig) == 24 * 4
    for S in (KmbConfig, KmbBatch, KmbPretrain, KmbGemm):
        assert not [f for f in S._fields_ if "smooth" in f[0]]


def test_op_entry_points_refuse_a_bad_eps(lib):
    """before any launch: no device pointer is touched (these run without a GPU)"""
    for bad in (-0.1, 1.0, math.nan):
        assert lib.kmb_op_ce_smooth(C.c_void_p(16), 8, 8, C.c_void_p(16), 1, 1.0, bad, C.c_void_p(16), None, C.c_void_p(16), C.c_void_p(16), None) != 0
        assert b"eps" in lib.kmb_last_error()
        assert lib.kmb_op_ce_bf16_smooth(C.c_void_p(16), 8, 8, C.c_void_p(16), 1, 1.0, bad, C.c_void_p(16), None, C.c_void_p(16), C.c_void_p(16),
                                         None, None) != 0
        assert b"eps" in lib.kmb_last_error()
    assert lib.kmb_op_ce_vocab_sum_scratch(50320, 768) == 512 * (768 + 8)
    assert lib.kmb_op_ce_rows_finish_smooth_scratch(32768, 768) == 1024 * 768


def test_model_property_and_config_round_trip():
    """config.label_smoothing (an extra key: config.py's defaults do not list it) seeds the model's property; writes are validated"""
    from src.model.config import MultiModalBartConfig
    from src.model.model import MultiModalBartForConditionalGeneration, MultiModalBartForPreTraining, MultiModalBartModel
    from oracle import goldenlib as G
    tiny = dict(G.TINY)
    cfg = MultiModalBartConfig.from_dict(dict(tiny, label_smoothing=0.1))
    assert cfg.to_dict()["label_smoothing"] == 0.1
    for cls in (MultiModalBartForConditionalGeneration, MultiModalBartForPreTraining, MultiModalBartModel):
        m = cls(cfg)
        assert m.label_smoothing == 0.1
        m.label_smoothing = 0.25
        assert m.label_smoothing == 0.25
        for bad in (-0.1, 1.0, float("nan")):
            with pytest.raises(ValueError):
                m.label_smoothing = bad
        assert m.label_smoothing == 0.25
    assert MultiModalBartForConditionalGeneration(MultiModalBartConfig.from_dict(tiny)).label_smoothing == 0.0
    with pytest.raises(ValueError):
        MultiModalBartForConditionalGeneration(MultiModalBartConfig.from_dict(dict(tiny, label_smoothing=1.0)))


# ------------------------------------------------------------------------------------------------ the command lines
@pytest.mark.parametrize("script", ["vcg_train", "pretrain"])
def test_cli_flag(script):
    import importlib
    mod = importlib.import_module(script)
    base = ["--checkpoint_dir", "x", "--model_config", "y", "--synthetic", "2"]
    assert mod.parse_args(base).label_smoothing == 0.0
    assert mod.parse_args(base + ["--label_smoothing", "0.1"]).label_smoothing == pytest.approx(0.1)
    for bad in ("-0.1", "1.0", "nan"):
        with pytest.raises(ValueError, match="label_smoothing"):
            mod.parse_args(base + ["--label_smoothing", bad])
