"""Plain-torch references and emulations of the per-row weighted cross-entropy (kmb_forward_opts.row_weights / loss_reduction; DESIGN.md
section 6q); a helper module of test_loss_weights_cpu.py, test_loss_weights_ops_gpu.py and test_loss_weights_model_gpu.py, built on
tests/loss_ref.py and tests/label_smoothing_ref.py (same conventions: float64 REFERENCES from the values the kernel receives, EMULATIONS
with the kernels' documented roundings, figures measured between the two).

The criterion:  L = sum_r w_r nll_r / D  over the rows whose label is in [0, V), nll_r the (label-smoothed) cross-entropy row, D the number
of those rows ("mean") or 1 ("sum").  The weight of an ignored row is never read: it may be NaN.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import label_smoothing_ref as L  # noqa: E402
import loss_ref as R  # noqa: E402

SEQ_WEIGHTS = (1.75, -0.5, 0.75, 1.25)   # the per-sequence pattern of the model tests: w_b = SEQ_WEIGHTS[b % 4]

# ---- figures of emu_fused_w against fused_w_ref at loss_ref.FUSED (M = 1024, V = 8150, Vpad = 8192, d = 128, lm_factor = 5, every seventh
# ---- label -100) with the mixed-sign row weights of row_weights(), "mean", measured by test_loss_weights_cpu.py (which fails when a
# ---- recorded figure is below its measurement or more than 10 % above it); the GPU tests allow 2 x these.
# dH: a row scale cancels in a row's relative norm -- exactly so in front of the row's one bf16 rounding (the CPU test asserts that the rows'
# relative errors of alpha P' E - beta wsum are the unweighted ones); the rounding itself lands elsewhere on w x than on x (the weights are no
# powers of two), so the figures behind it are measured like the others: worst row 4.37e-3 against the unweighted 4.12e-3 at eps = 0.
# dE: rows of opposite sign cancel in the sum over rows, so the figures may exceed the unweighted ones (they do not, at these weights).
# eps -> relative norms
EMU_W = {
    0.0: dict(dH_worst=4.5e-3, dH_matrix=2.45e-3, dE_worst=4.45e-3, dE_matrix=2.45e-3),   # measured 4.373e-3, 2.366e-3, 4.301e-3, 2.385e-3
    0.1: dict(dH_worst=4.45e-3, dH_matrix=2.42e-3, dE_worst=4.55e-3, dE_matrix=2.44e-3),  # measured 4.335e-3, 2.343e-3, 4.403e-3, 2.363e-3
}
EMU_W_ROW_LOSS_ABS = 4.2e-7       # weighted row loss, absolute (measured 3.91e-7 at eps = 0, 3.52e-7 at 0.1): |w| <= 2.625 times the shift's fp32 rounding

# ---- recorded results of tests/test_loss_weights_model_gpu.py on the MI355X
# (d) identity, on the bf16 head (tiny) and on the fused head: loss_weights=None, all-ones [B] and all-ones [B, T] give the same loss bits and
#     the same gradient bits outside the tied matrix; the tied matrix (fp32 atomics) stays inside the spread of two unweighted runs.
# (h) trained tiny fixture, unfiltered sampling, 43 tokens: sampler -sum_logprobs.sum() 0.398999, "sum" forward with unit weights 0.401008,
#     oracle teacher-forced 0.399823 -> oracle gaps 8.2e-4 (sampler) and 1.19e-3 (training forward); the two differ by 2.0e-3 <= 2 x 1.19e-3.
H_GAP_SAMPLER, H_GAP_TRAINING = 8.2e-4, 1.19e-3


def seq_weights(B):
    """float32 [B]: SEQ_WEIGHTS[b % 4]"""
    return torch.tensor([SEQ_WEIGHTS[b % 4] for b in range(B)], dtype=torch.float32)


def row_weights(M):
    """float32 [M]: SEQ_WEIGHTS[r % 4] * (1 + 0.5 * (r // 4 % 2)) -- both signs, six magnitudes, every value exact in bf16"""
    r = torch.arange(M)
    base = torch.tensor(SEQ_WEIGHTS, dtype=torch.float64)[r % 4]
    return (base * (1.0 + 0.5 * ((r // 4) % 2).to(torch.float64))).to(torch.float32)


def masked(w, ok):
    """float64 weights with the entries of ignored rows replaced by 0 (they are never read: NaN there must not leak)"""
    return torch.where(ok, R.f64(w), torch.zeros_like(R.f64(w)))


def denominator(ok, reduction):
    """D as a float: the number of valid rows ("mean") or 1 ("sum"); 0 without a valid row (nothing is divided then)"""
    n = int(ok.sum())
    return float(n) if reduction == "mean" else (1.0 if n > 0 else 0.0)


# ------------------------------------------------------------------------------------------------ the criterion, dense
def w_rows(logits, labels, V, eps, w):
    """float64 w_r * (lse - (1 - eps) v[label] - eps mean v) (exactly 0 in ignored rows) and the valid mask"""
    rows, ok = L.ls_rows(logits, labels, V, eps)
    return masked(w, ok) * rows, ok


def w_loss(rows, ok, reduction):
    """the reduced loss of weighted rows: NaN for "mean" without a valid label (as torch's mean), exactly 0 for "sum\""""
    if reduction == "sum":
        return rows.sum()
    return R.ce_mean(rows, ok)


def w_grad(logits, labels, V, scale, eps, w, reduction="mean"):
    """float64 w_r (softmax - target) * scale / D over [rows, V] and |w_r| times the larger operand of the subtraction"""
    G, big = L.ls_grad(logits, labels, V, scale, eps)      # divided by the count
    ok = R.valid_labels(labels, V)
    k = float(int(ok.sum())) if reduction == "sum" else 1.0
    wm = masked(w, ok)[:, None]
    return G * wm * k, big * wm.abs() * k


# ------------------------------------------------------------------------------------------------ the fused chain
def fused_w_ref(H, E, bias, labels, V, lm_factor, eps, w, reduction="mean"):
    """float64, dense: v = H E[:V]^T + b, weighted loss rows, G = w (softmax - target) lm_factor / D, dH = G E[:V], dE = G^T H, and the
    per-row factors of the rank-one form: alpha = w g / S, beta = w eps g / V, u = sum_r beta_r h_r (g = lm_factor / D)"""
    v = R.f64(H) @ R.f64(E[:V]).t() + R.f64(bias)
    rows, ok = w_rows(v, labels, V, eps, w)
    G, big = w_grad(v, labels, V, lm_factor, eps, w, reduction)
    D = denominator(ok, reduction)
    g = lm_factor / D if D > 0 else 0.0
    lab = labels.clamp(0, V - 1)
    c = v[torch.arange(v.shape[0]), lab]
    S = torch.exp(v - c[:, None]).sum(1)
    wm = masked(w, ok)
    alpha = wm * g / S
    beta = wm * (eps * g / V)
    u = (beta[:, None] * R.f64(H)).sum(0)
    return dict(v=v, loss_rows=rows, ok=ok, G=G, big=big, dH=G @ R.f64(E[:V]), dE=G.t() @ R.f64(H), alpha=alpha, beta=beta, u=u, S=S)


def emu_fused_w(H, E, bias, labels, V, lm_factor, eps, w, reduction="mean"):
    """label_smoothing_ref.emu_fused_ls with the weight where the kernels put it (csrc/loss.hip ce_rows_finish*_kernel<true>): alpha and
    beta are multiplied by w_r, so aH = bf16(w alpha H), dH = bf16(w alpha P' E - w beta wsum) and u carry it; P, S and the label's entry
    bf16(1 - (1 - eps) S) are weight-free.  Unit weights reproduce emu_fused_ls bit for bit."""
    v = R.f64(H) @ R.f64(E[:V]).t() + R.f64(bias)
    ok = R.valid_labels(labels, V)
    D = denominator(ok, reduction)
    lab = labels.clamp(0, V - 1)
    rix = torch.arange(v.shape[0], device=v.device)
    f32 = lambda t: t.to(torch.float32).to(torch.float64)  # noqa: E731
    wsum, bsum = L.vocab_sums(E, bias, V)
    wsum, bsum = f32(wsum), f32(bsum)
    c = f32(v[rix, lab])
    ex = torch.exp(v - c[:, None])
    ex[~ok] = 0.0
    S = ex.sum(1)
    P = R.rb(ex)
    Pl = P.clone()
    Pl[rix[ok], lab[ok]] = R.rb(1.0 - (1.0 - eps) * S[ok])
    g = lm_factor / D if D > 0 else 0.0
    wm = masked(w, ok)
    alpha = torch.where(ok, g / S.clamp(min=1e-300), torch.zeros_like(S)) * wm
    beta = f32(f32(torch.where(ok, torch.full_like(S, eps * g / V), torch.zeros_like(S))) * wm)
    aH = R.rb(alpha[:, None] * R.f64(H))
    zbar = (R.f64(H) @ wsum + bsum) / V
    rows = wm * torch.where(ok, torch.log(S.clamp(min=1e-300)) + eps * (c - zbar), torch.zeros_like(S))
    u = f32((beta[:, None] * R.f64(H)).sum(0))
    dH_pre = alpha[:, None] * (Pl @ R.f64(E[:V])) - beta[:, None] * wsum[None, :]   # what the data-gradient finish rounds, once
    return dict(shift=c, P=P, Pl=Pl, S=S, alpha=alpha, beta=beta, aH=aH, loss_rows=rows, wsum=wsum, bsum=bsum, u=u,
                aP=alpha[:, None] * Pl, dH_pre=dH_pre, dH=R.rb(dH_pre), dE=Pl.t() @ aH - u[None, :])
