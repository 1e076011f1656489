"""Plain-torch references and emulations of the label-smoothed cross-entropy (csrc/loss.hip "Label smoothing as rank-one terms"); a helper
module of test_label_smoothing_cpu.py and test_label_smoothing_ops_gpu.py, built on tests/loss_ref.py (same conventions: float64 REFERENCES
of the operation from the values the kernel receives, EMULATIONS with the kernels' documented roundings, figures measured between the two).

The criterion is torch's F.cross_entropy(logits[:, :V], labels, ignore_index=-100, label_smoothing=eps): the target row is
(1 - eps) onehot + eps / V, the mean runs over the rows whose label is in [0, V).
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import loss_ref as R  # noqa: E402

# ---- figures of emu_fused_ls against fused_ls_ref at loss_ref.FUSED (M = 1024, V = 8150, Vpad = 8192, d = 128, lm_factor = 5, every seventh
# ---- label -100), measured by test_label_smoothing_cpu.py (which fails when one no longer holds); the GPU tests allow 2 x these.
# eps -> (dH worst row, dH whole matrix, dE worst row, dE whole matrix), relative norms
EMU_LS = {
    0.1: dict(dH_worst=4.3e-3, dH_matrix=2.4e-3, dE_worst=4.3e-3, dE_matrix=2.4e-3),   # measured 4.22e-3, 2.33e-3, 4.29e-3, 2.34e-3
    0.3: dict(dH_worst=4.3e-3, dH_matrix=2.4e-3, dE_worst=4.5e-3, dE_matrix=2.4e-3),   # measured 4.26e-3, 2.31e-3, 4.41e-3, 2.34e-3
}
EMU_LS_ROW_LOSS_ABS = 1.4e-7      # row loss at eps = 0.1, absolute (measured 1.34e-7): the shift held in fp32; far inside the GPU test's 3e-4


# ------------------------------------------------------------------------------------------------ the criterion, dense
def ls_rows(logits, labels, V, eps):
    """float64 loss rows lse - (1 - eps) v[label] - eps mean_{j < V} v_j (0 where the label is -100 or out of range) and the valid mask"""
    x = R.f64(logits[:, :V])
    ok = R.valid_labels(labels, V)
    lse = torch.logsumexp(x, dim=1)
    pick = x.gather(1, labels.clamp(0, V - 1)[:, None])[:, 0]
    rows = lse - (1.0 - eps) * pick - eps * x.mean(dim=1)
    return torch.where(ok, rows, torch.zeros_like(rows)), ok


def ls_grad(logits, labels, V, scale, eps):
    """float64 (softmax - (1 - eps) onehot - eps / V) * scale / count over [rows, V], zero in ignored / out-of-range rows, and the larger of
    the two operands of that subtraction (softmax and the target, both times scale / count) for the cancellation-aware bound, as
    loss_ref.kl_ref returns it: p_j meets eps / V within a factor of a few all over the row, so no bound relative to the difference holds"""
    x = R.f64(logits[:, :V])
    ok = R.valid_labels(labels, V)
    n = int(ok.sum())
    k = scale / n if n > 0 else 0.0
    a = torch.softmax(x, dim=1) * k
    t = torch.full_like(x, eps / V)
    t[torch.arange(x.shape[0], device=x.device), labels.clamp(0, V - 1)] += 1.0 - eps
    b = t * k
    a[~ok] = 0.0
    b[~ok] = 0.0
    return a - b, torch.maximum(a.abs(), b.abs())


def emu_ls_grad(logits, labels, V, scale, eps):
    """the two-kernel path: the float64 gradient row rounded once to bf16"""
    return R.rb(ls_grad(logits, labels, V, scale, eps)[0])


# ------------------------------------------------------------------------------------------------ the fused chain
def vocab_sums(E, bias, V):
    """float64 wsum = sum_{j < V} E_j and bsum = sum_{j < V} b_j"""
    return R.f64(E[:V]).sum(0), R.f64(bias[:V]).sum()


def fused_ls_ref(H, E, bias, labels, V, lm_factor, eps):
    """float64, dense: logits v = H E[:V]^T + b, loss rows, G = (softmax - target) lm_factor / count, dH = G E[:V], dE = G^T H"""
    v = R.f64(H) @ R.f64(E[:V]).t() + R.f64(bias)
    rows, ok = ls_rows(v, labels, V, eps)
    G, big = ls_grad(v, labels, V, lm_factor, eps)
    return dict(v=v, loss_rows=rows, ok=ok, G=G, big=big, dH=G @ R.f64(E[:V]), dE=G.t() @ R.f64(H))


def fused_ls_rank_one(H, E, bias, labels, V, lm_factor, eps):
    """float64, the rank-one form the kernels use and nothing rounded: zbar = (h . wsum + bsum) / V; loss = log S + eps (c - zbar) with c
    the label's logit and S = sum_j exp(v_j - c); the onehot part inside the matrix (P'[label] = 1 - (1 - eps) S), the uniform part outside:
    dH = a (P' E) - beta wsum, dE = P'^T (a H) - u, beta = eps g / V on valid rows, u = sum_r beta_r h_r"""
    v = R.f64(H) @ R.f64(E[:V]).t() + R.f64(bias)
    ok = R.valid_labels(labels, V)
    n = int(ok.sum())
    lab = labels.clamp(0, V - 1)
    rix = torch.arange(v.shape[0], device=v.device)
    wsum, bsum = vocab_sums(E, bias, V)
    c = v[rix, lab]
    ex = torch.exp(v - c[:, None])
    ex[~ok] = 0.0
    S = ex.sum(1)
    Pl = ex.clone()
    Pl[rix[ok], lab[ok]] = 1.0 - (1.0 - eps) * S[ok]
    g = lm_factor / n if n > 0 else 0.0
    alpha = torch.where(ok, g / S.clamp(min=1e-300), torch.zeros_like(S))
    beta = torch.where(ok, torch.full_like(S, eps * g / V), torch.zeros_like(S))
    zbar = (R.f64(H) @ wsum + bsum) / V
    rows = torch.where(ok, torch.log(S.clamp(min=1e-300)) + eps * (c - zbar), torch.zeros_like(S))
    u = (beta[:, None] * R.f64(H)).sum(0)
    return dict(loss_rows=rows, dH=alpha[:, None] * (Pl @ R.f64(E[:V])) - beta[:, None] * wsum[None, :],
                dE=Pl.t() @ (alpha[:, None] * R.f64(H)) - u[None, :], u=u, beta=beta, wsum=wsum, bsum=bsum)


def emu_fused_ls(H, E, bias, labels, V, lm_factor, eps):
    """loss_ref.emu_fused with the smoothing terms and their roundings (csrc/loss.hip): c = fp32(label's logit); P = bf16(exp(v - c)); S the
    unrounded sum; wsum, bsum held in fp32; loss = log S + eps (c - zbar); P'[label] = bf16(1 - (1 - eps) S); aH = bf16(alpha H);
    dH = bf16(alpha P' E - beta wsum), ONE rounding; u in fp32; dE = P'^T aH - u.  eps = 0 reproduces loss_ref.emu_fused."""
    v = R.f64(H) @ R.f64(E[:V]).t() + R.f64(bias)
    ok = R.valid_labels(labels, V)
    n = int(ok.sum())
    lab = labels.clamp(0, V - 1)
    rix = torch.arange(v.shape[0], device=v.device)
    f32 = lambda t: t.to(torch.float32).to(torch.float64)  # noqa: E731
    wsum, bsum = vocab_sums(E, bias, V)
    wsum, bsum = f32(wsum), f32(bsum)
    c = f32(v[rix, lab])
    ex = torch.exp(v - c[:, None])
    ex[~ok] = 0.0
    S = ex.sum(1)
    P = R.rb(ex)
    Pl = P.clone()
    Pl[rix[ok], lab[ok]] = R.rb(1.0 - (1.0 - eps) * S[ok])
    g = lm_factor / n if n > 0 else 0.0
    alpha = torch.where(ok, g / S.clamp(min=1e-300), torch.zeros_like(S))
    beta = f32(torch.where(ok, torch.full_like(S, eps * g / V), torch.zeros_like(S)))
    aH = R.rb(alpha[:, None] * R.f64(H))
    zbar = (R.f64(H) @ wsum + bsum) / V
    rows = torch.where(ok, torch.log(S.clamp(min=1e-300)) + eps * (c - zbar), torch.zeros_like(S))
    u = f32((beta[:, None] * R.f64(H)).sum(0))
    return dict(shift=c, P=P, Pl=Pl, S=S, alpha=alpha, beta=beta, aH=aH, loss_rows=rows, wsum=wsum, bsum=bsum, u=u,
                dH=R.rb(alpha[:, None] * (Pl @ R.f64(E[:V])) - beta[:, None] * wsum[None, :]), dE=Pl.t() @ aH - u[None, :])
