"""CPU: the emulations of tests/loss_ref.py against its float64 references, at the shapes and seeds the GPU tests use.

Every composite bound of test_loss_ops_gpu.py / test_heads_ops_gpu.py is 2 x a figure of loss_ref.EMU_*; this module re-measures each
figure (printing it: run with -s) and fails when the measurement exceeds the recorded figure, or when the recorded figure has grown
slack (more than 1.5 x the measurement), so a bound can neither be missed by the emulation itself nor be widened quietly.
Measured here (float64, CPU): one bf16 rounding of a gradient element 0.9962 * 2^-8 worst (fp32 logits, bf16 logits and the fused
a . P' alike); fused dH worst row 4.12e-3 / matrix 2.34e-3; dE worst row 4.38e-3 / matrix 2.37e-3; fused row loss 1.5e-7 absolute; MRM head (n = 203, d = 768, C = 1601) 1.6e-3 .. 3.0e-3 per gradient tensor."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import loss_ref as R  # noqa: E402


def _holds(measured, recorded, what):
    print("%-40s measured %.4e  recorded %.4e" % (what, measured, recorded))
    assert measured <= recorded, (what, measured, recorded)
    assert recorded <= 1.5 * measured, (what, "recorded figure is slack", measured, recorded)


def test_references_agree_with_torch_autograd():
    """the closed forms of loss_ref are torch's own losses: F.cross_entropy (mean over labels != -100) and F.kl_div batchmean"""
    g = torch.Generator().manual_seed(1)
    x = torch.randn(11, 37, generator=g, dtype=torch.float64).requires_grad_(True)
    labels = torch.randint(0, 37, (11,), generator=g)
    labels[3] = R.IGNORE
    loss = F.cross_entropy(x, labels) * 2.5
    loss.backward()
    rows, ok = R.ce_rows(x.detach(), labels, 37)
    assert torch.allclose(R.ce_mean(rows, ok) * 2.5, loss.detach(), rtol=1e-12)
    assert torch.allclose(R.ce_grad(x.detach(), labels, 37, 2.5), x.grad, rtol=1e-10, atol=1e-15)
    y = torch.randn(5, 19, generator=g, dtype=torch.float64).requires_grad_(True)
    t = torch.softmax(torch.randn(5, 19, generator=g, dtype=torch.float64), 1)
    t[1] = 0.0
    t[1, 4] = 1.0
    t[2] *= 0.6
    kl = 3.0 * F.kl_div(torch.log_softmax(y, 1), t, reduction="batchmean")
    kl.backward()
    rows, grad, big = R.kl_ref(y.detach(), t, 19, 3.0)
    assert torch.allclose(3.0 * rows.sum() / 5, kl.detach(), rtol=1e-12)
    assert torch.allclose(grad, y.grad, rtol=1e-9, atol=1e-15)
    assert bool((big >= grad.abs() - 1e-18).all())


@pytest.mark.parametrize("V,ld,bf16", [(1601, 1608, False), (129, 136, True), (8150, 8192, True)])
def test_one_rounding_of_the_gradient_row(V, ld, bf16):
    """the two-kernel path writes the float64 gradient rounded once: every element within 2^-8 relative, so the GPU tests' rule
    2^-8 + 2^-15 leaves the kernel's fp32 exp / log-sum-exp the 2^-15"""
    x, labels = R.ce_case(V, ld, 9, seed=V, bf16=bf16, pad_value=0.0)
    ref = R.ce_grad(x, labels, V, 3.0)
    emu = R.emu_ce_grad(x, labels, V, 3.0)
    nz = ref != 0
    worst = float(((emu - ref).abs()[nz] / ref.abs()[nz]).max())
    print("one rounding, V = %d: worst element %.5f * 2^-8" % (V, worst / 2.0 ** -8))
    assert worst <= R.EMU_ONE_ROUNDING
    assert float(torch.softmax(R.f64(x[:, :V]), 1).max()) < 0.9   # the label's p - 1 does not cancel


@pytest.fixture(scope="module")
def fused():
    H, E, bias, labels = R.fused_case()
    c = R.FUSED
    return R.fused_ref(H, E, bias, labels, c["V"], c["lm_factor"]), R.emu_fused(H, E, bias, labels, c["V"], c["lm_factor"])


def test_fused_chain_emulation_elementwise(fused):
    ref, emu = fused
    G = ref["G"]
    nz = G != 0
    worst = float(((emu["aP"] - G).abs()[nz] / G.abs()[nz]).max())
    print("fused a . P', label entry included: worst element %.5f * 2^-8" % (worst / 2.0 ** -8))
    assert worst <= R.EMU_ONE_ROUNDING * (1 + 1e-6)
    assert float(emu["aP"][~ref["ok"]].abs().max()) == 0.0
    _holds(float((emu["loss_rows"] - ref["loss_rows"]).abs().max()), R.EMU_ROW_LOSS_ABS, "fused row loss, absolute")
    assert float(torch.softmax(ref["v"], 1).max()) < 0.9
    sig = float(ref["v"].std())
    assert 1.5 < sig < 1.9, sig


def test_fused_chain_emulation_gradients(fused):
    ref, emu = fused
    worst, whole = R.row_rel_norms(emu["dH"], ref["dH"])
    _holds(worst, R.EMU_DH_WORST_ROW, "dH worst row, relative norm")
    _holds(whole, R.EMU_DH_MATRIX, "dH whole matrix")
    worst, whole = R.row_rel_norms(emu["dE"], ref["dE"])
    _holds(worst, R.EMU_DE_WORST_ROW, "dE worst row, relative norm")
    _holds(whole, R.EMU_DE_MATRIX, "dE whole matrix")


def test_head_emulation():
    k = R.head_case()
    ref, emu = R.head_ref(k), R.emu_head(k)
    for name, recorded in R.EMU_HEAD.items():
        _holds(R.rel_norm(emu[name], ref[name]), recorded, "MRM head " + name)
    _holds(R.row_rel_norms(emu["d_states"], ref["d_states"])[0], R.EMU_HEAD_STATES_WORST_ROW, "MRM head d_states worst row")
    loss_err = abs(float(emu["loss"] - ref["loss"])) / abs(float(ref["loss"]))
    print("MRM head loss, relative: %.3e" % loss_err)
    assert loss_err < 0.1 * R.F32_TOL     # the GPU test holds the loss to F32_TOL: the emulation's share of it is small
    # the head's own gradient, not the upstream one, dominates the rows it touches
    t = k["rows"].long().unique()
    assert float((ref["d_states"][t] - R.f64(k["dhdec"])[t]).norm()) > float(R.f64(k["dhdec"])[t].norm())
