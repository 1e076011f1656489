"""Plain-torch references and emulations of the training-loss and pre-training-head kernels (a helper module of
test_loss_emulation_cpu.py, test_loss_ops_gpu.py and test_heads_ops_gpu.py; runs on whatever device its inputs live on).

Two kinds of code:

* float64 REFERENCES of the operation itself, computed from the bf16 / fp32 values the kernel receives: cross-entropy rows
  (reference src/model/model.py:397-403, CrossEntropyLoss(): mean over labels != -100), (softmax - onehot) * scale / count,
  F.kl_div(log_softmax, t, 'batchmean') and its gradient (:248-258), dense -> tanh -> out_proj (:133-158).
* EMULATIONS: the same float64 arithmetic with the roundings the kernels document (csrc/loss.hip, csrc/heads.hip) applied at the
  documented points -- the gradient row rounded once to bf16; P = bf16(exp(v - c)); the label's entry bf16(1 - S); a . H and dH
  rounded to bf16.  They exist so that every composite bound of the GPU tests is a figure measured between emulation and
  reference, never between kernel and reference: test_loss_emulation_cpu.py re-measures the EMU_* figures below at the GPU
  tests' own shapes and seeds, the GPU tests allow twice the figure (fp32 accumulation order is all the margin has to cover).
"""
import torch

IGNORE = -100
BF16_ROUND = 2.0 ** -8            # worst relative error of one round-to-nearest bf16 rounding (half an ulp at a power of two)
F32_EXP_NOISE = 2.0 ** -15        # fp32 exp / log-sum-exp at arguments below 32 in magnitude: 32 * 2^-24 = 2^-19 absolute on the
#                                   exponent, a few of them (max, log of the sum, the subtraction) -- 2^-15 covers sixteen
ELEM_RULE = BF16_ROUND + F32_EXP_NOISE
BF16_MAX = 3.3895313892515355e38  # largest finite bf16

# ---- figures of the emulation against the float64 reference, measured by test_loss_emulation_cpu.py (which fails when a
# ---- figure no longer holds); the GPU tests bound kernel-against-reference by 2 x these
# fused tied-head chain at fused_case(): M = 1024, V = 8150, Vpad = 8192, d = 128, lm_factor = 5
EMU_ONE_ROUNDING = 2.0 ** -8      # gradient element, relative: fp32 logits, bf16 logits, fused a . P' with the label's entry (measured 0.9961 * 2^-8)
EMU_DH_WORST_ROW = 4.2e-3         # dH row, relative norm   (measured 4.12e-3)
EMU_DH_MATRIX = 2.4e-3            #                         (measured 2.34e-3)
EMU_DE_WORST_ROW = 4.4e-3         #                         (measured 4.38e-3)
EMU_DE_MATRIX = 2.4e-3            #                         (measured 2.37e-3)
EMU_ROW_LOSS_ABS = 2e-7           # fused row loss, absolute: the shift held in fp32 (measured 1.5e-7); far inside the GPU test's 3e-4
# MRM head at head_case(): n = 203, d = 768, C = 1601: relative norm of the whole tensor (measured 2.17e-3, 1.57e-3, 2.83e-3, 2.81e-3,
# 2.98e-3), and the worst row of the decoder-state gradient (measured 4.30e-3).  The head's loss carries no bf16 rounding of its own beyond
# tanh's (measured 3.4e-6 relative): it is held to the project's fp32 tolerance instead.
EMU_HEAD = {"d_out_w": 2.3e-3, "d_out_b": 1.7e-3, "d_dense_w": 3.0e-3, "d_dense_b": 3.0e-3, "d_states": 3.1e-3}
EMU_HEAD_STATES_WORST_ROW = 4.4e-3
F32_TOL = 1e-4                    # tests/test_ops_gpu.py F32_TOL


def f64(x):
    return x.to(torch.float64)


def rb(x):
    """float64 -> the float64 value of its bf16 rounding (through fp32, as the kernels round)"""
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def valid_labels(labels, V):
    return (labels >= 0) & (labels < V)


# ------------------------------------------------------------------------------------------------ cross-entropy
def ce_rows(logits, labels, V):
    """float64 loss rows (0 where the label is -100 or out of range) and the valid mask; logits [rows, >= V] of any float type"""
    x = f64(logits[:, :V])
    ok = valid_labels(labels, V)
    lse = torch.logsumexp(x, dim=1)
    pick = x.gather(1, labels.clamp(0, V - 1)[:, None])[:, 0]
    return torch.where(ok, lse - pick, torch.zeros_like(lse)), ok


def ce_mean(rows, ok):
    n = int(ok.sum())
    return rows.sum() / n if n > 0 else torch.tensor(float("nan"), dtype=torch.float64, device=rows.device)


def ce_grad(logits, labels, V, scale):
    """float64 (softmax - onehot) * scale / count over [rows, V]; zero rows where the label is ignored / out of range"""
    x = f64(logits[:, :V])
    ok = valid_labels(labels, V)
    n = int(ok.sum())
    g = torch.softmax(x, dim=1)
    g[torch.arange(x.shape[0], device=x.device), labels.clamp(0, V - 1)] -= 1.0
    g = g * (scale / n if n > 0 else 0.0)
    g[~ok] = 0.0
    return g


def emu_ce_grad(logits, labels, V, scale):
    """the two-kernel path: the float64 gradient row rounded once to bf16"""
    return rb(ce_grad(logits, labels, V, scale))


def elementwise_excess(got, ref, bound):
    """worst |got - ref| - bound over all elements (<= 0 passes), with its (row, column), got, ref for the failure message"""
    ex = (f64(got) - ref).abs() - bound
    i = int(torch.argmax(ex))
    r, c = divmod(i, ex.shape[1])
    return float(ex.reshape(-1)[i]), (r, c, float(f64(got)[r, c]), float(ref[r, c]))


def assert_elementwise(got, ref, rel=ELEM_RULE, extra_abs=None, what=""):
    """|got - ref| <= rel * |ref| (+ extra_abs, a tensor broadcastable to ref) for EVERY element"""
    bound = rel * ref.abs()
    if extra_abs is not None:
        bound = bound + extra_abs
    ex, (r, c, g, w) = elementwise_excess(got, ref, bound)
    assert ex <= 0.0, "%s: element (%d, %d) got %.9g want %.9g: |diff| = %.3g exceeds its bound by %.3g" % (what, r, c, g, w, abs(g - w), ex)


def row_rel_norms(got, ref):
    """(worst row's relative norm over rows whose reference is not zero, whole-matrix relative norm)"""
    d = (f64(got) - ref).norm(dim=1)
    n = ref.norm(dim=1)
    nz = n > 0
    worst = float((d[nz] / n[nz]).max()) if bool(nz.any()) else 0.0
    return worst, float((f64(got) - ref).norm() / ref.norm())


# ------------------------------------------------------------------------------------------------ case generators (CPU)
def ce_case(V, ld, rows, seed, bf16, pad_value):
    """logits [rows, ld] (sigma 3: the label's probability stays far below 0.9, so p - 1 does not cancel), pad columns = pad_value;
    labels: 0, V - 1, a column of a thread's last chunk, -100, V (out of range), a pad-range value, a column of the row's last 8, then random"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(rows, ld, generator=g) * 3.0
    x[:, V:] = pad_value
    labels = torch.randint(0, V, (rows,), generator=g)
    last_chunk = min(((V - 1) // 8192) * 8192 + 43, V - 1)     # inside the last register chunk of some thread (loss.hip ce_kernel_reg*)
    special = [0, V - 1, last_chunk, IGNORE, V, (V + ld) // 2, max(V - 5, 0)]
    for i, s in enumerate(special[:rows]):
        labels[i] = s
    return (x.to(torch.bfloat16) if bf16 else x), labels


FUSED = dict(M=1024, V=8150, Vpad=8192, d=128, lm_factor=5.0, seed=2024)


def fused_case(all_ignored=False):
    """the smallest shape KmbGemm act 5 accepts (4 x 32 = 128 tiles); logits sigma ~ 1.7; every seventh label -100; rows V..Vpad-1 of E
    hold non-zero garbage that the -1e30 pad bias must silence"""
    c = FUSED
    g = torch.Generator(device="cpu").manual_seed(c["seed"])
    H = torch.randn(c["M"], c["d"], generator=g).to(torch.bfloat16)
    E = (torch.randn(c["Vpad"], c["d"], generator=g) * 0.15).to(torch.bfloat16)
    E[c["V"]:] = (torch.randn(c["Vpad"] - c["V"], c["d"], generator=g) * 2.0 + 1.0).to(torch.bfloat16)
    bias = torch.randn(c["V"], generator=g) * 0.3
    labels = torch.randint(0, c["V"], (c["M"],), generator=g)
    labels[::7] = IGNORE
    labels[1], labels[2] = 0, c["V"] - 1
    if all_ignored:
        labels[:] = IGNORE
    return H, E, bias, labels


# ------------------------------------------------------------------------------------------------ the fused chain
def fused_ref(H, E, bias, labels, V, lm_factor):
    """float64: logits v = H E[:V]^T + b, loss rows, G = (softmax - onehot) lm_factor / count, dH = G E[:V], dE = G^T H"""
    v = f64(H) @ f64(E[:V]).t() + f64(bias)
    rows, ok = ce_rows(v, labels, V)
    G = ce_grad(v, labels, V, lm_factor)
    return dict(v=v, loss_rows=rows, ok=ok, G=G, dH=G @ f64(E[:V]), dE=G.t() @ f64(H))


def emu_fused(H, E, bias, labels, V, lm_factor):
    """the fused chain's documented roundings on float64 arithmetic (csrc/loss.hip "Tied-head cross-entropy WITHOUT a pass over
    the logits"): c = fp32(h . E[label] + b[label]); P = bf16(exp(v - c)); S = sum_j exp(v - c) (unrounded, as the GEMM epilogue sums);
    loss = log S (the engine passes no pick); P'[label] = bf16(1 - S); alpha = lm_factor / (count S); aH = bf16(alpha H); dH = bf16(alpha P' E); dE = P'^T aH"""
    v = f64(H) @ f64(E[:V]).t() + f64(bias)
    ok = valid_labels(labels, V)
    n = int(ok.sum())
    lab = labels.clamp(0, V - 1)
    rix = torch.arange(v.shape[0], device=v.device)
    c = v[rix, lab].to(torch.float32).to(torch.float64)
    ex = torch.exp(v - c[:, None])
    ex[~ok] = 0.0
    S = ex.sum(1)
    P = rb(ex)
    Pl = P.clone()
    Pl[rix[ok], lab[ok]] = rb(1.0 - S[ok])
    alpha = torch.where(ok, lm_factor / (n * S.clamp(min=1e-300)), torch.zeros_like(S)) if n > 0 else torch.zeros_like(S)
    aH = rb(alpha[:, None] * f64(H))
    loss_rows = torch.where(ok, torch.log(S.clamp(min=1e-300)), torch.zeros_like(S))   # pick = null, as the engine runs it: the shift's fp32 rounding stays in
    return dict(shift=c, P=P, Pl=Pl, S=S, alpha=alpha, aH=aH, loss_rows=loss_rows, aP=alpha[:, None] * Pl,
                dH=rb(alpha[:, None] * (Pl @ f64(E[:V]))), dE=Pl.t() @ aH)


# ------------------------------------------------------------------------------------------------ KL divergence (MRM head)
def kl_ref(logits, target, C, scale):
    """float64 F.kl_div(log_softmax(logits[:, :C]), target, 'batchmean'): (loss rows, gradient of scale * batchmean wrt the logits,
    the two operands of the gradient's subtraction -- sum(t) softmax and t, both times scale / rows -- for the cancellation-aware bound)"""
    x, t = f64(logits[:, :C]), f64(target[:, :C])
    logp = torch.log_softmax(x, dim=1)
    rows = torch.where(t > 0, t * (torch.log(t.clamp(min=1e-300)) - logp), torch.zeros_like(t)).sum(1)
    k = scale / x.shape[0]
    a, b = t.sum(1, keepdim=True) * torch.exp(logp) * k, t * k
    return rows, a - b, torch.maximum(a.abs(), b.abs())


# ------------------------------------------------------------------------------------------------ one classification head
HEAD = dict(n=203, d=768, C=1601, Cpad=1608, rows_total=640, factor=1.0, seed=77)


def head_case():
    """MRM head at the real class count: decoder states [rows_total, d] bf16 with an upstream gradient already in place, n gathered
    rows (with repeats), soft targets, bf16 weights and fp32 biases of dense [d, d] and out_proj [C, d]"""
    c = HEAD
    g = torch.Generator(device="cpu").manual_seed(c["seed"])
    hdec = torch.randn(c["rows_total"], c["d"], generator=g).to(torch.bfloat16)
    dhdec = (torch.randn(c["rows_total"], c["d"], generator=g) * 1e-5).to(torch.bfloat16)
    rows = torch.randint(0, c["rows_total"], (c["n"],), generator=g).to(torch.int32)
    rows[:6] = rows[6]                       # one state gathered seven times
    Wd = (torch.randn(c["d"], c["d"], generator=g) * 0.03).to(torch.bfloat16)
    bd = torch.randn(c["d"], generator=g) * 0.02
    Wo = (torch.randn(c["C"], c["d"], generator=g) * 0.05).to(torch.bfloat16)
    bo = torch.randn(c["C"], generator=g) * 0.02
    tgt = torch.softmax(torch.randn(c["n"], c["C"], generator=g) * 2.0, dim=1)
    return dict(hdec=hdec, dhdec=dhdec, rows=rows, Wd=Wd, bd=bd, Wo=Wo, bo=bo, tgt=tgt)


def head_forward(x, Wd, bd, Wo, bo):
    """float64 dense -> tanh -> out_proj (BartClassificationHead, classif_dropout = 0)"""
    y = torch.tanh(f64(x) @ f64(Wd).t() + f64(bd))
    return y, y @ f64(Wo).t() + f64(bo)


def head_ref(k):
    """float64 autograd of factor * kl_div(log_softmax(head(hdec[rows])), tgt, 'batchmean') on the same weights; the decoder-state
    gradient is the upstream one plus the head's"""
    import torch.nn.functional as F
    hdec = f64(k["hdec"]).requires_grad_(True)
    p = [f64(k[n]).requires_grad_(True) for n in ("Wd", "bd", "Wo", "bo")]
    x = hdec[k["rows"].long()]
    y = torch.tanh(x @ p[0].t() + p[1])
    lg = y @ p[2].t() + p[3]
    loss = HEAD["factor"] * F.kl_div(torch.log_softmax(lg, dim=1), f64(k["tgt"]), reduction="batchmean")
    loss.backward()
    return dict(loss=loss.detach(), d_dense_w=p[0].grad, d_dense_b=p[1].grad, d_out_w=p[2].grad, d_out_b=p[3].grad,
                d_states=f64(k["dhdec"]) + hdec.grad, y=y.detach(), logits=lg.detach())


def emu_head(k):
    """engine_train.cpp head_run's roundings on float64 arithmetic: y = bf16(tanh); logits fp32; dlogits = bf16; dy = bf16((dlogits Wo)(1 - y^2));
    dx = bf16(dy Wd); scatter-add in fp32; states gradient = bf16(upstream + sum)"""
    n, C, f = HEAD["n"], HEAD["C"], HEAD["factor"]
    x = f64(k["hdec"])[k["rows"].long()]
    y = rb(torch.tanh(x @ f64(k["Wd"]).t() + f64(k["bd"])))
    lg = (y @ f64(k["Wo"]).t() + f64(k["bo"])).to(torch.float32)
    rows, g, _ = kl_ref(lg, k["tgt"], C, f)
    g = rb(g)
    dy = rb((g @ f64(k["Wo"])) * (1.0 - y * y))
    dx = rb(dy @ f64(k["Wd"]))
    acc = torch.zeros_like(f64(k["hdec"]))
    acc.index_add_(0, k["rows"].long(), dx)
    return dict(loss=f * rows.sum() / n, d_out_w=g.t() @ y, d_out_b=g.sum(0), d_dense_w=dy.t() @ x, d_dense_b=dy.sum(0),
                d_states=rb(f64(k["dhdec"]) + acc.to(torch.float32).to(torch.float64)))


def rel_norm(got, ref):
    return float((f64(got) - ref).norm() / ref.norm())
