"""GPU: the per-row weighted cross-entropy kernels op by op through the C-ABI, against float64 (tests/loss_weights_ref.py).

What runs: ce_kernel_reg<13, LS, true> / ce_kernel<LS, true> (fp32 logits) and ce_kernel_reg_bf16<7 | 8, LS, true> (bf16 logits, in place
and out of place) at eps = 0 and 0.1, "mean" and "sum"; the fused chain ce_label_logit -> GEMM act 5 -> [ce_vocab_sum] ->
ce_rows_finish{,_ls}_kernel<true> -> data-gradient GEMM (un-split and split-K) -> finish -> weight gradient, as
test_label_smoothing_ops_gpu.py drives it (its _FusedLS with the weighted row finish).

Bounds -- each is one of:
  * the elementwise rule of test_loss_ops_gpu.py for a bf16 gradient, 2^-8 + 2^-15, times |w_r| times the larger operand of the gradient's
    subtraction;
  * F32_TOL = 1e-4 relative for fp32 results (row losses, the reduced loss, alpha, beta);
  * 2 x a figure of the emulation against float64 with these weights, recorded in loss_weights_ref.EMU_W and re-measured by
    test_loss_weights_cpu.py: eps = 0: dH worst row 4.37e-3 (recorded 4.5e-3 -> bound 9.0e-3), matrix 2.37e-3 (2.45e-3 -> 4.9e-3), dE worst
    row 4.30e-3 (4.45e-3 -> 8.9e-3), matrix 2.39e-3 (2.45e-3 -> 4.9e-3); eps = 0.1: 4.34e-3 / 2.34e-3 / 4.40e-3 / 2.36e-3.  The factor 2
    covers fp32 accumulation order only.
Exact statements (zeros in pad columns and ignored rows whatever their weight holds, untouched poison, the weight-free srow and label
entry, NULL and all-ones weights against the old entry points, in place against out of place) are asserted exactly."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from kmbart import _lib  # noqa: E402
from kmbart._lib import check, ptr  # noqa: E402
from gpu_util import DEV, stream  # noqa: E402
import loss_ref as R  # noqa: E402
import loss_weights_ref as W  # noqa: E402
from test_label_smoothing_ops_gpu import _FusedLS, _bits, _i32, _run_ce  # noqa: E402

F32_TOL = R.F32_TOL
REDUCTIONS = {"mean": 0, "sum": 1}


# ------------------------------------------------------------------------------------------------ (a) the row kernels
def _case_weights(labels, V):
    """the per-row pattern with a negative (row 1), a zero on a valid row (row 2), NaN on the -100 row (3) and on the out-of-range row (4),
    an infinity on the pad-range row (5)"""
    w = W.row_weights(labels.shape[0]).to(DEV)
    w[2] = 0.0
    w[3], w[4], w[5] = float("nan"), float("nan"), float("inf")
    ok = R.valid_labels(labels, V)
    assert float(w[1]) < 0 and bool(ok[1]) and bool(ok[2]) and not bool(ok[3]) and not bool(ok[4]) and not bool(ok[5])
    return w


def _run_w(lib, x, labels, V, ld, scale, eps, w, reduction, inplace=False):
    rows = x.shape[0]
    lg = x.clone()
    loss_rows = torch.full((rows,), 7.0, device=DEV)
    count, loss, status = _i32(), torch.full((1,), 7.0, device=DEV), _i32()
    dl = lg if inplace else torch.full((rows, ld), 7.0, dtype=torch.bfloat16, device=DEV)
    wp = None if w is None else ptr(w)
    if x.dtype == torch.bfloat16:
        check(lib.kmb_op_ce_bf16_weighted(ptr(lg), ld, V, ptr(labels), rows, scale, eps, wp, REDUCTIONS[reduction], ptr(loss_rows), ptr(dl),
                                          ptr(count), ptr(loss), ptr(status), stream()))
    else:
        check(lib.kmb_op_ce_weighted(ptr(lg), ld, V, ptr(labels), rows, scale, eps, wp, REDUCTIONS[reduction], ptr(loss_rows), ptr(dl),
                                     ptr(count), ptr(loss), stream()))
    return dl, loss_rows, count, loss


def _check_w(V, labels, logits, w, loss_rows, dl, count, loss, scale, eps, reduction, what):
    ref_rows, ok = W.w_rows(logits, labels, V, eps, w)
    assert int(count[0]) == int(ok.sum()), (what, int(count[0]))
    err = (R.f64(loss_rows) - ref_rows).abs()
    nz = ref_rows != 0
    print("%s: row loss worst relative %.3e (bound %.1e)" % (what, float((err[nz] / ref_rows[nz].abs()).max()), F32_TOL))
    assert bool((err <= F32_TOL * ref_rows.abs()).all()), (what, "loss_rows", float(err.max()))
    assert bool((loss_rows[~ok] == 0).all()) and float(loss_rows[2]) == 0.0, what + ": ignored rows and the zero-weight row"
    un_rows = W.w_rows(logits, labels, V, eps, torch.ones_like(w))[0]
    assert float((ref_rows - un_rows).abs().max()) > 1.0, "the rows must see the weights"
    want = float(W.w_loss(ref_rows, ok, reduction))
    assert abs(float(loss) - want) <= F32_TOL * abs(want), (what, float(loss), want)
    ref, big = W.w_grad(logits, labels, V, scale, eps, w, reduction)
    ex, (r, c, g, wv) = R.elementwise_excess(dl[:, :V], ref, R.ELEM_RULE * big)
    assert ex <= 0.0, "%s gradient: element (%d, %d) got %.9g want %.9g exceeds its bound by %.3g" % (what, r, c, g, wv, ex)
    assert float(dl[:, V:].float().abs().max()) == 0.0, what + ": pad columns of the gradient"
    assert float(dl[~ok].float().abs().max()) == 0.0, what + ": ignored / out-of-range rows (NaN and infinite weights)"
    assert float(dl[2].float().abs().max()) == 0.0, what + ": the zero-weight row"
    live = ok.clone()
    live[2] = False
    assert bool((dl[live][:, :V] != 0).any(dim=1).all())
    # the sign: a negative weight turns the row around (the label's entry of softmax - target is negative, so w < 0 makes it positive)
    assert float(dl[1, int(labels[1])]) > 0 and float(dl[0, int(labels[0])]) < 0


def _identity(lib, x, labels, V, ld, eps):
    """a NULL weights pointer and all-ones weights through the new entry: the old entry's bits"""
    old = _run_ce(lib, x, labels, V, ld, 3.0, eps, smooth=eps > 0)
    for w in (None, torch.ones(x.shape[0], device=DEV)):
        new = _run_w(lib, x, labels, V, ld, 3.0, eps, w, "mean")
        for a, b, name in zip(new, old, ("dlogits", "loss_rows", "count", "loss")):
            assert torch.equal(_bits(a), _bits(b)), (name, "NULL" if w is None else "ones", eps)


@pytest.mark.parametrize("V,ld", [(50320, 50432), (60000, 60032), (1601, 1608)])
def test_ce_fp32_weighted(V, ld):
    """kmb_op_ce_weighted: ce_kernel_reg<13, LS, true> up to ld = 53248, the 256-thread ce_kernel<LS, true> above; pad columns hold NaN"""
    lib = _lib.load()
    x, labels = R.ce_case(V, ld, 9, seed=V, bf16=False, pad_value=float("nan"))
    x, labels = x.to(DEV), labels.to(DEV)
    w = _case_weights(labels, V)
    for eps in (0.0, 0.1):
        for reduction in ("mean", "sum"):
            dl, loss_rows, count, loss = _run_w(lib, x, labels, V, ld, 3.0, eps, w, reduction)
            _check_w(V, labels, x, w, loss_rows, dl, count, loss, 3.0, eps, reduction, "fp32 ce V=%d eps=%.1f %s" % (V, eps, reduction))
        _identity(lib, x, labels, V, ld, eps)


@pytest.mark.parametrize("V,ld", [(50320, 50432), (57345, 57352), (129, 136)])
def test_ce_bf16_weighted(V, ld):
    """kmb_op_ce_bf16_weighted: ce_kernel_reg_bf16<7, LS, true> up to ld = 57344, <8, LS, true> above; out of place and in place; pad
    columns hold the largest finite bf16"""
    lib = _lib.load()
    x, labels = R.ce_case(V, ld, 9, seed=V, bf16=True, pad_value=R.BF16_MAX)
    x, labels = x.to(DEV), labels.to(DEV)
    w = _case_weights(labels, V)
    for eps in (0.0, 0.1):
        for reduction in ("mean", "sum"):
            dl, loss_rows, count, loss = _run_w(lib, x, labels, V, ld, 3.0, eps, w, reduction)
            _check_w(V, labels, x, w, loss_rows, dl, count, loss, 3.0, eps, reduction, "bf16 ce V=%d eps=%.1f %s" % (V, eps, reduction))
            dli, rowsi, counti, lossi = _run_w(lib, x, labels, V, ld, 3.0, eps, w, reduction, inplace=True)
            assert torch.equal(_bits(dli), _bits(dl)) and torch.equal(rowsi, loss_rows) and torch.equal(lossi, loss), "in place and out of place differ"
        _identity(lib, x, labels, V, ld, eps)


def test_sum_without_a_valid_label_is_exactly_zero():
    """"sum": loss exactly 0 and a zero gradient; "mean" stays NaN (loss_finish_kernel); NaN weights everywhere"""
    lib = _lib.load()
    V, ld = 129, 136
    x, _ = R.ce_case(V, ld, 9, seed=V, bf16=True, pad_value=0.0)
    x = x.to(DEV)
    labels = torch.full((9,), R.IGNORE, dtype=torch.int64, device=DEV)
    w = torch.full((9,), float("nan"), device=DEV)
    for src in (x, x.float()):
        dl, rows, count, loss = _run_w(lib, src, labels, V, ld, 3.0, 0.0, w, "sum")
        assert int(count[0]) == 0 and float(loss) == 0.0 and bool((rows == 0).all()) and float(dl.float().abs().max()) == 0.0
        dl, rows, count, loss = _run_w(lib, src, labels, V, ld, 3.0, 0.0, w, "mean")
        assert bool(torch.isnan(loss).all()) and bool((rows == 0).all()) and float(dl.float().abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ (b) the fused chain
class _FusedW(_FusedLS):
    """_FusedLS with kmb_op_ce_rows_finish_weighted as its row finish (eps = 0: the plain instance, whose beta and u do not exist -- they are
    set to zero here so that the smoothing forms of the two finishes behind it run as the plain ones)"""

    def __init__(self, eps, w, reduction="mean", all_ignored=False):
        self.w, self.reduction = w, reduction
        super().__init__(eps=eps, all_ignored=all_ignored)

    def finish(self, lmf, eps, smooth=True):
        lib = _lib.load()
        M, d = self.M, self.d
        o = dict(loss_rows=torch.full((M,), 7.0, device=DEV), srow=torch.full((M,), 7.0, device=DEV), alpha=torch.full((M,), 7.0, device=DEV),
                 beta=torch.full((M,), 7.0, device=DEV), ah=torch.full((M, d), 7.0, dtype=torch.bfloat16, device=DEV),
                 neg_u=torch.full((d,), float("nan"), device=DEV))
        scratch = torch.full((int(lib.kmb_op_ce_rows_finish_smooth_scratch(M, d)),), float("nan"), device=DEV)
        check(lib.kmb_op_ce_rows_finish_weighted(ptr(self.sums), self.nparts, self.nparts, None, ptr(self.shift), ptr(self.labels), ptr(self.count),
                                                 lmf, eps, None if self.w is None else ptr(self.w), REDUCTIONS[self.reduction], M, d, self.V,
                                                 ptr(self.H), d, ptr(self.wsum), ptr(o["loss_rows"]), ptr(o["srow"]), ptr(o["alpha"]),
                                                 ptr(o["beta"]), ptr(o["ah"]), ptr(self.P), self.Vpad, ptr(o["neg_u"]), ptr(scratch), stream()))
        if eps == 0.0:
            assert bool((o["beta"] == 7.0).all()) and bool(torch.isnan(o["neg_u"]).all()), "eps = 0 runs the plain instance: no beta, no u"
            o["beta"].zero_()
            o["neg_u"].zero_()
        return o


def _weights(all_nan_on_ignored=True):
    c = R.FUSED
    labels = R.fused_case()[3]
    w = W.row_weights(c["M"])
    if all_nan_on_ignored:
        w[~R.valid_labels(labels, c["V"])] = float("nan")
    return w.to(DEV)


@pytest.fixture(scope="module", params=[0.0, 0.1])
def runs(request):
    eps = request.param
    c = R.FUSED
    H, E, bias, labels = (t.to(DEV) for t in R.fused_case())
    w = _weights()
    return dict(eps=eps, w=w, weighted=_FusedW(eps, w), plain=_FusedLS(eps=eps),
                ref=W.fused_w_ref(H, E, bias, labels, c["V"], c["lm_factor"], eps, w))


def test_fused_weight_free_parts(runs):
    """srow and the label's entry of P' (the whole stored matrix) carry no weight: the unweighted run's bits"""
    f, p = runs["weighted"], runs["plain"]
    assert torch.equal(_bits(f.fin["srow"]), _bits(p.fin["srow"]))
    assert torch.equal(_bits(f.P), _bits(p.P)) and not torch.equal(_bits(f.P), _bits(f.P_gemm))
    assert not torch.equal(_bits(f.fin["alpha"]), _bits(p.fin["alpha"]))


def test_fused_row_factors_and_losses(runs):
    f, ref, ok = runs["weighted"], runs["ref"], runs["ref"]["ok"]
    for k in ("alpha", "beta", "loss_rows"):
        if k == "beta" and runs["eps"] == 0.0:
            continue
        err = (R.f64(f.fin[k]) - ref[k]).abs()
        print("weighted fused %s against float64: worst relative %.3e (bound %.1e)" % (k, float((err[ok] / ref[k][ok].abs()).max()), F32_TOL))
        assert bool((err <= F32_TOL * ref[k].abs()).all()), (k, float(err.max()))
        assert bool((f.fin[k][~ok] == 0).all()), k + ": ignored rows, whose weights are NaN"
    assert bool((f.fin["alpha"][ok] < 0).any()) and bool((f.fin["alpha"][ok] > 0).any())
    assert torch.equal(_bits(f.fin["ah"]), _bits((f.fin["alpha"][:, None] * f.H.float()).to(torch.bfloat16))), "ah != bf16(alpha H)"
    want = float(W.w_loss(ref["loss_rows"], ok, "mean"))
    assert abs(float(f.loss) - want) <= F32_TOL * abs(want)


def test_fused_gradients(runs):
    f, ref, fig = runs["weighted"], runs["ref"], W.EMU_W[runs["eps"]]
    for what, dH in (("un-split", f.dH1), ("split_k = 3", f.dH3)):
        worst, whole = R.row_rel_norms(dH, ref["dH"])
        print("weighted dH %s eps %.1f against float64: worst row %.3e (bound %.3e), whole matrix %.3e (bound %.3e)"
              % (what, runs["eps"], worst, 2 * fig["dH_worst"], whole, 2 * fig["dH_matrix"]))
        assert worst <= 2 * fig["dH_worst"] and whole <= 2 * fig["dH_matrix"], (what, worst, whole)
        assert float(dH[~ref["ok"]].float().abs().max()) == 0.0
    for what, dE in (("un-split", f.dE), ("split_k = 3", f.dE3)):
        assert bool((dE[f.V:] == 7.0).all()), "rows beyond V are not the launch's to write: the poison stays"
        worst, whole = R.row_rel_norms(dE[: f.V], ref["dE"])
        print("weighted dE %s eps %.1f against float64: worst row %.3e (bound %.3e), whole matrix %.3e (bound %.3e)"
              % (what, runs["eps"], worst, 2 * fig["dE_worst"], whole, 2 * fig["dE_matrix"]))
        assert worst <= 2 * fig["dE_worst"] and whole <= 2 * fig["dE_matrix"], (what, worst, whole)
    # the weights are visible: the unweighted run's gradients miss by far
    p = runs["plain"]
    assert R.row_rel_norms(p.dH1, ref["dH"])[1] > 0.3 and R.row_rel_norms(p.dE[: f.V], ref["dE"])[1] > 0.3


def test_fused_sum_is_mean_times_the_valid_count(runs):
    f, eps = runs["weighted"], runs["eps"]
    s = _FusedW(eps, runs["w"], reduction="sum")
    n = int(f.count[0])
    assert int(s.count[0]) == n and int(s.count[1]) == 1 and n > 1
    assert torch.equal(_bits(s.fin["loss_rows"]), _bits(f.fin["loss_rows"])) and torch.equal(_bits(s.P), _bits(f.P))
    for k in ("alpha", "beta"):
        a, b = R.f64(s.fin[k]), R.f64(f.fin[k]) * n
        assert bool(((a - b).abs() <= F32_TOL * b.abs()).all()), k
    for a, b in ((s.dH3, f.dH3), (s.dE3[: f.V], f.dE3[: f.V])):
        assert R.rel_norm(a, R.f64(b) * n) <= 2 * 2.0 ** -8     # dH: each side is one bf16 rounding; dE: fp32


def test_fused_unit_and_null_weights_are_the_unweighted_chain(runs):
    p, eps = runs["plain"], runs["eps"]
    for w in (None, torch.ones(R.FUSED["M"], device=DEV)):
        f = _FusedW(eps, w)
        for k in ("loss_rows", "srow", "alpha", "ah") + (("beta", "neg_u") if eps > 0 else ()):
            assert torch.equal(_bits(f.fin[k]), _bits(p.fin[k])), k
        assert torch.equal(_bits(f.P), _bits(p.P)) and torch.equal(_bits(f.dH3), _bits(p.dH3)) and torch.equal(_bits(f.dE), _bits(p.dE))


@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_fused_all_labels_ignored(reduction):
    w = torch.full((R.FUSED["M"],), float("nan"), device=DEV)
    f = _FusedW(0.1, w, reduction=reduction, all_ignored=True)
    assert int(f.count[0]) == 0 and (reduction == "mean" or int(f.count[1]) == 0)
    assert float(f.P.float().abs().max()) == 0.0
    assert bool((f.fin["alpha"] == 0).all()) and bool((f.fin["beta"] == 0).all()) and float(f.fin["ah"].float().abs().max()) == 0.0
    assert bool((f.fin["neg_u"] == 0).all()) and bool((f.fin["loss_rows"] == 0).all()) and bool((f.fin["srow"] == 0).all())
    for t in (f.dH1, f.dH3, f.dE[: f.V], f.dE3[: f.V]):
        assert not bool(torch.isnan(t.float()).any()) and float(t.float().abs().max()) == 0.0
    assert bool((f.dE[f.V:] == 7.0).all()) and bool((f.dE3[f.V:] == 7.0).all()), "untouched poison stays"
