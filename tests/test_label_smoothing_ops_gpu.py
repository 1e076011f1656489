"""GPU: the label-smoothing kernels op by op through the C-ABI, against float64 (references and emulations: tests/label_smoothing_ref.py).

What runs: ce_kernel_reg<13, true> / ce_kernel<true> (fp32 logits) and ce_kernel_reg_bf16<7 | 8, true> (bf16 logits, in place) at eps = 0.1;
the fused chain ce_label_logit -> GEMM act 5 -> ce_vocab_sum -> ce_rows_finish_ls -> data-gradient GEMM (un-split and split-K) ->
ce_dgrad_finish_ls, and the weight gradient over V rows with -u as the un-split launch's bias operand and as the slab reduction's row vector.

Bounds -- each is one of:
  * the elementwise rule of test_loss_ops_gpu.py for a bf16 gradient, 2^-8 + 2^-15, times the LARGER operand of the gradient's subtraction
    (softmax against (1 - eps) onehot + eps / V: the two meet within a factor of a few all over a row, a bound relative to the difference
    cannot hold even for the float64 row rounded once -- test_label_smoothing_cpu.py shows that);
  * a tolerance the project already has: F32_TOL = 1e-4 relative for fp32 results, 3e-4 absolute on a fused row loss (test_fused_loss_rows);
  * an fp32 summation bound written out where it is used (wsum, bsum, u);
  * 2 x a figure of the emulation against float64, re-measured by test_label_smoothing_cpu.py at this module's shape (loss_ref.FUSED):
    eps = 0.1: dH worst row 4.22e-3 (recorded 4.3e-3 -> bound 8.6e-3), matrix 2.33e-3 (2.4e-3 -> 4.8e-3), dE worst row 4.29e-3
    (4.3e-3 -> 8.6e-3), matrix 2.34e-3 (2.4e-3 -> 4.8e-3).  The factor 2 covers fp32 accumulation order only.
Exact statements (zeros in pad columns and ignored rows, untouched poison, the label entry's bits, eps = 0 against the old entry points) are
asserted exactly."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from kmbart import _lib  # noqa: E402
from kmbart._lib import check, ptr  # noqa: E402
from gpu_util import DEV, gemm, stream  # noqa: E402
import label_smoothing_ref as L  # noqa: E402
import loss_ref as R  # noqa: E402

F32_TOL = R.F32_TOL
U32 = 2.0 ** -24   # fp32 unit roundoff
EPS = 0.1


def _i32(n=4, fill=0):
    return torch.full((n,), fill, dtype=torch.int32, device=DEV)


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


# ------------------------------------------------------------------------------------------------ (a) the two-kernel forms
def _run_ce(lib, x, labels, V, ld, scale, eps, smooth=True, inplace=False):
    rows = x.shape[0]
    bf16 = x.dtype == torch.bfloat16
    lg = x.clone()
    loss_rows = torch.full((rows,), 7.0, device=DEV)
    count, loss, status = _i32(), torch.zeros(1, device=DEV), _i32()
    dl = lg if inplace else torch.full((rows, ld), 7.0, dtype=torch.bfloat16, device=DEV)
    if bf16 and smooth:
        check(lib.kmb_op_ce_bf16_smooth(ptr(lg), ld, V, ptr(labels), rows, scale, eps, ptr(loss_rows), ptr(dl), ptr(count), ptr(loss), ptr(status),
                                        stream()))
    elif bf16:
        check(lib.kmb_op_ce_bf16(ptr(lg), ld, V, ptr(labels), rows, scale, ptr(loss_rows), ptr(dl), ptr(count), ptr(loss), ptr(status), stream()))
    elif smooth:
        check(lib.kmb_op_ce_smooth(ptr(lg), ld, V, ptr(labels), rows, scale, eps, ptr(loss_rows), ptr(dl), ptr(count), ptr(loss), stream()))
    else:
        check(lib.kmb_op_ce(ptr(lg), ld, V, ptr(labels), rows, scale, ptr(loss_rows), ptr(dl), ptr(count), ptr(loss), stream()))
    return dl, loss_rows, count, loss


def _check_ce_smooth(V, ld, labels, logits, loss_rows, dl, count, loss, scale, eps, what):
    ref_rows, ok = L.ls_rows(logits, labels, V, eps)
    assert int(count[0]) == int(ok.sum()), (what, int(count[0]))
    err = (R.f64(loss_rows) - ref_rows).abs()
    print("%s: row loss worst relative %.3e (bound %.1e)" % (what, float((err[ok] / ref_rows[ok].abs()).max()), F32_TOL))
    assert bool((err <= F32_TOL * ref_rows.abs()).all()), (what, "loss_rows", float(err.max()))
    assert bool((loss_rows[~ok] == 0).all())
    rows0 = R.ce_rows(logits, labels, V)[0]
    assert float((ref_rows - rows0).abs().max()) > 0.05, "the rows must see the smoothing term"
    want = R.ce_mean(ref_rows, ok)
    assert abs(float(loss) - float(want)) <= F32_TOL * abs(float(want)), (what, float(loss), float(want))
    ref, big = L.ls_grad(logits, labels, V, scale, eps)
    ex, (r, c, g, w) = R.elementwise_excess(dl[:, :V], ref, R.ELEM_RULE * big)
    assert ex <= 0.0, "%s gradient: element (%d, %d) got %.9g want %.9g exceeds its bound by %.3g" % (what, r, c, g, w, ex)
    assert float(dl[:, V:].float().abs().max()) == 0.0, what + ": pad columns of the gradient"
    assert float(dl[~ok].float().abs().max()) == 0.0, what + ": ignored / out-of-range rows"
    assert bool((dl[ok][:, :V] != 0).any(dim=1).all())


@pytest.mark.parametrize("V,ld", [(50320, 50432), (60000, 60032), (1601, 1608)])
def test_ce_fp32_smooth(V, ld):
    """kmb_op_ce_smooth: ce_kernel_reg<13, true> up to ld = 53248, the 256-thread ce_kernel<true> above; pad columns hold NaN"""
    lib = _lib.load()
    x, labels = R.ce_case(V, ld, 9, seed=V, bf16=False, pad_value=float("nan"))
    x, labels = x.to(DEV), labels.to(DEV)
    dl, loss_rows, count, loss = _run_ce(lib, x, labels, V, ld, 3.0, EPS)
    _check_ce_smooth(V, ld, labels, x, loss_rows, dl, count, loss, 3.0, EPS, "fp32 ce V=%d" % V)
    # eps = 0 through the new entry point: the old one's bits
    dl0, rows0, count0, loss0 = _run_ce(lib, x, labels, V, ld, 3.0, 0.0)
    dlo, rowso, counto, losso = _run_ce(lib, x, labels, V, ld, 3.0, 0.0, smooth=False)
    assert torch.equal(_bits(dl0), _bits(dlo)) and torch.equal(_bits(rows0), _bits(rowso)) and torch.equal(_bits(loss0), _bits(losso))


@pytest.mark.parametrize("V,ld", [(50320, 50432), (57337, 57344), (57345, 57352), (65530, 65536), (129, 136)])
def test_ce_bf16_smooth(V, ld):
    """kmb_op_ce_bf16_smooth: ce_kernel_reg_bf16<7, true> up to ld = 57344, <8, true> above; out of place and in place; pad columns hold the
    largest finite bf16"""
    lib = _lib.load()
    x, labels = R.ce_case(V, ld, 9, seed=V, bf16=True, pad_value=R.BF16_MAX)
    x, labels = x.to(DEV), labels.to(DEV)
    dl, loss_rows, count, loss = _run_ce(lib, x, labels, V, ld, 3.0, EPS)
    _check_ce_smooth(V, ld, labels, x, loss_rows, dl, count, loss, 3.0, EPS, "bf16 ce V=%d" % V)
    dli, rowsi, counti, lossi = _run_ce(lib, x, labels, V, ld, 3.0, EPS, inplace=True)
    assert torch.equal(_bits(dli), _bits(dl)) and torch.equal(rowsi, loss_rows) and torch.equal(lossi, loss), "in place and out of place differ"
    dl0, rows0, count0, loss0 = _run_ce(lib, x, labels, V, ld, 3.0, 0.0)
    dlo, rowso, counto, losso = _run_ce(lib, x, labels, V, ld, 3.0, 0.0, smooth=False)
    assert torch.equal(_bits(dl0), _bits(dlo)) and torch.equal(_bits(rows0), _bits(rowso)) and torch.equal(_bits(loss0), _bits(losso))


# ------------------------------------------------------------------------------------------------ (b) the fused chain
class _FusedLS:
    """one run of the chain on loss_ref.fused_case() with smoothing; every stage's outputs kept for the stage tests"""

    def __init__(self, eps=EPS, all_ignored=False):
        lib = _lib.load()
        c = R.FUSED
        M, V, Vpad, d = c["M"], c["V"], c["Vpad"], c["d"]
        self.M, self.V, self.Vpad, self.d, self.lmf, self.eps = M, V, Vpad, d, c["lm_factor"], eps
        H, E, bias, labels = (t.to(DEV) for t in R.fused_case(all_ignored))
        self.H, self.E, self.bias, self.labels = H, E, bias, labels
        self.nparts = Vpad // 64
        self.shift = torch.full((M,), 7.0, device=DEV)
        self.bias_pad = torch.full((Vpad,), 7.0, device=DEV)
        check(lib.kmb_op_ce_label_logit(ptr(H), d, ptr(E), d, ptr(bias), ptr(labels), M, d, V, Vpad, ptr(self.shift), ptr(self.bias_pad), stream()))
        self.P = torch.full((M, Vpad), 7.0, dtype=torch.bfloat16, device=DEV)
        self.sums = torch.full((M, self.nparts), float("nan"), device=DEV)
        gemm(H, E, bias=self.bias_pad, act=5, out_bf16=self.P, row_shift=self.shift, row_sums=self.sums)
        self.P_gemm = self.P.clone()
        self.count = _i32()
        check(lib.kmb_op_count_valid(ptr(labels), M, V, ptr(self.count), None, stream()))
        # wsum | bsum: E's rows beyond V hold garbage that must not be summed
        self.wsum = torch.full((d + 8,), float("nan"), device=DEV)
        scratch = torch.full((int(lib.kmb_op_ce_vocab_sum_scratch(V, d)),), float("nan"), device=DEV)
        check(lib.kmb_op_ce_vocab_sum(ptr(E), d, ptr(bias), V, d, ptr(self.wsum), ptr(scratch), stream()))
        self.fin = self.finish(self.lmf, eps)
        self.loss = torch.full((1,), 7.0, device=DEV)
        check(lib.kmb_op_loss_finish(ptr(self.fin["loss_rows"]), M, ptr(self.count), ptr(self.loss), stream()))
        self.acc1 = torch.full((M, d), float("nan"), device=DEV)
        gemm(self.P, E, b_kc=False, out_f32=self.acc1)
        self.slab = torch.full((3, M, d), float("nan"), device=DEV)
        gemm(self.P, E, b_kc=False, split_k=3, slab=self.slab)
        self.dH1, self.dH3 = self.dgrad(self.acc1, 1, self.fin), self.dgrad(self.slab, 3, self.fin)
        self.dE, self.dE3 = self.wgrad(self.fin), self.wgrad(self.fin, split=3)
        torch.cuda.synchronize()

    def finish(self, lmf, eps, smooth=True):
        lib = _lib.load()
        M, d = self.M, self.d
        o = dict(loss_rows=torch.full((M,), 7.0, device=DEV), srow=torch.full((M,), 7.0, device=DEV), alpha=torch.full((M,), 7.0, device=DEV),
                 beta=torch.full((M,), 7.0, device=DEV), ah=torch.full((M, d), 7.0, dtype=torch.bfloat16, device=DEV),
                 neg_u=torch.full((d,), float("nan"), device=DEV))
        if smooth:
            scratch = torch.full((int(lib.kmb_op_ce_rows_finish_smooth_scratch(M, d)),), float("nan"), device=DEV)
            check(lib.kmb_op_ce_rows_finish_smooth(ptr(self.sums), self.nparts, self.nparts, None, ptr(self.shift), ptr(self.labels),
                                                   ptr(self.count), lmf, eps, M, d, self.V, ptr(self.H), d, ptr(self.wsum), ptr(o["loss_rows"]),
                                                   ptr(o["srow"]), ptr(o["alpha"]), ptr(o["beta"]), ptr(o["ah"]), ptr(self.P), self.Vpad,
                                                   ptr(o["neg_u"]), ptr(scratch), stream()))
        else:
            check(lib.kmb_op_ce_rows_finish(ptr(self.sums), self.nparts, self.nparts, None, ptr(self.labels), ptr(self.count), lmf, M, d, self.V,
                                            ptr(self.H), d, ptr(o["loss_rows"]), ptr(o["srow"]), ptr(o["alpha"]), ptr(o["ah"]), ptr(self.P),
                                            self.Vpad, stream()))
        return o

    def dgrad(self, buf, nslabs, fin):
        out = torch.full((self.M, self.d), 7.0, dtype=torch.bfloat16, device=DEV)
        check(_lib.load().kmb_op_ce_dgrad_finish_smooth(ptr(buf), nslabs, self.M * self.d, ptr(fin["alpha"]), ptr(fin["beta"]), ptr(self.wsum),
                                                        ptr(out), self.M, self.d, stream()))
        return out

    def wgrad(self, fin, split=0):
        """dE[:V] = P'^T (a . H) - u over V rows, as the engine runs it (lin_wgrad with M = V): un-split with -u as the launch's bias operand,
        split with -u as the slab reduction's row vector; rows V.. of the destination keep their poison"""
        out = torch.full((self.Vpad, self.d), 7.0, device=DEV)
        if split:
            slab = torch.full((split, self.V, self.d), float("nan"), device=DEV)
            gemm(self.P, fin["ah"], a_kc=False, b_kc=False, M=self.V, split_k=split, slab=slab)
            check(_lib.load().kmb_op_reduce_slabs_rowvec(ptr(slab), split, self.V * self.d, ptr(out), self.V, self.d, 0.0, ptr(fin["neg_u"]), stream()))
        else:
            gemm(self.P, fin["ah"], a_kc=False, b_kc=False, M=self.V, bias=fin["neg_u"], out_f32=out)
        return out


@pytest.fixture(scope="module")
def fused():
    return _FusedLS()


@pytest.fixture(scope="module")
def ref():
    c = R.FUSED
    H, E, bias, labels = (t.to(DEV) for t in R.fused_case())
    return L.fused_ls_ref(H, E, bias, labels, c["V"], c["lm_factor"], EPS)


def test_vocab_sums(fused):
    f = fused
    Ed, bd = R.f64(f.E[: f.V]), R.f64(f.bias)
    want_w, want_b = Ed.sum(0), bd.sum()
    # fp32 sums of values that are exact in fp32.  wsum: a row lane chains at most 32 additions (510 rows of a workgroup over 16 row lanes), 16
    # lanes meet in LDS, kmb_reduce_parts adds 16 slots as 2 per part-lane and 8 part-lanes: at most 58 roundings on any path, each
    # <= 2^-24 of a partial sum that sum_j |E_j| bounds -> 64 * 2^-24 * sum|E|.  bsum: 8 per lane, a 6-level butterfly, the same 10: 24.
    err_w = (R.f64(f.wsum[: f.d]) - want_w).abs()
    bound_w = 64 * U32 * Ed.abs().sum(0)
    assert bool((err_w <= bound_w).all()), float((err_w - bound_w).max())
    assert abs(float(f.wsum[f.d]) - float(want_b)) <= 64 * U32 * float(bd.abs().sum())
    # the garbage rows V.. of E (mean 1, sigma 2) would move every column by tens
    assert float((R.f64(f.E).sum(0) - want_w).abs().min()) > 1.0


def test_fused_loss_rows(fused, ref):
    f = fused
    err = (R.f64(f.fin["loss_rows"]) - ref["loss_rows"]).abs()
    print("smoothed fused row loss against float64: worst %.3e absolute (bound 3e-4)" % float(err.max()))
    assert float(err.max()) <= 3e-4, float(err.max())
    assert bool((f.fin["loss_rows"][~ref["ok"]] == 0).all())
    rows0 = L.ls_rows(ref["v"], f.labels, f.V, 0.0)[0]
    assert float((ref["loss_rows"] - rows0).abs().max()) > 0.05, "the check must see the smoothing term"
    want = float(R.ce_mean(ref["loss_rows"], ref["ok"]))
    assert abs(float(f.loss) - want) <= F32_TOL * abs(want)
    assert int(f.count[0]) == int(ref["ok"].sum())


def test_fused_rows_finish(fused, ref):
    f, ok, fin = fused, ref["ok"], fused.fin
    n = int(ok.sum())
    S = R.f64(f.sums).sum(1)
    assert bool(((R.f64(fin["srow"]) - S).abs()[ok] <= 8 * U32 * S[ok]).all())
    want_alpha = f.lmf / (n * R.f64(fin["srow"]))
    assert bool(((R.f64(fin["alpha"]) - want_alpha).abs()[ok] <= 4 * U32 * want_alpha[ok]).all())
    want_beta = f.eps * f.lmf / (n * f.V)
    assert bool(((R.f64(fin["beta"]) - want_beta).abs()[ok] <= 4 * U32 * want_beta).all())      # two products and a quotient
    assert bool((fin["srow"][~ok] == 0).all()) and bool((fin["alpha"][~ok] == 0).all()) and bool((fin["beta"][~ok] == 0).all())
    assert torch.equal(_bits(fin["ah"]), _bits((fin["alpha"][:, None] * f.H.float()).to(torch.bfloat16))), "ah != bf16(alpha H)"
    # the stored matrix changed only at the labels, and there it holds bf16(1 - (1 - eps) srow), formed in fp32 as the kernel forms it
    changed = _bits(f.P) != _bits(f.P_gemm)
    onehot = torch.zeros_like(changed)
    rix = torch.arange(f.M, device=DEV)[ok]
    onehot[rix, f.labels[ok]] = True
    assert bool((changed & ~onehot).sum() == 0)
    one_minus = torch.tensor(1.0, device=DEV) - torch.tensor(f.eps, dtype=torch.float32, device=DEV)
    want_entry = (torch.tensor(1.0, device=DEV) - one_minus * fin["srow"][ok]).to(torch.bfloat16)
    assert torch.equal(_bits(f.P[rix, f.labels[ok]]), _bits(want_entry))
    assert float(f.P[:, f.V:].float().abs().max()) == 0.0 and float(f.P[~ok].float().abs().max()) == 0.0
    # u: 1024 rows as 256 workgroups x 4 waves of one row each, the waves meet in LDS (3 additions), kmb_reduce_parts adds 256 slots as 8 per
    # part-lane and 32 part-lanes: at most 44 roundings, each <= 2^-24 of a partial sum that sum_r beta_r |h_r| bounds (the products are
    # rounded too: one more) -> 48 * 2^-24 * sum_r beta |h|
    want_u = (R.f64(fin["beta"])[:, None] * R.f64(f.H)).sum(0)
    bound_u = 48 * U32 * (R.f64(fin["beta"])[:, None] * R.f64(f.H).abs()).sum(0)
    err_u = (-R.f64(fin["neg_u"]) - want_u).abs()
    assert bool((err_u <= bound_u).all()), float((err_u - bound_u).max())


def _check_dH(f, dH, ref_dH, what):
    fig = L.EMU_LS[f.eps]
    worst, whole = R.row_rel_norms(dH, ref_dH)
    print("%s against float64: worst row %.3e (bound %.3e), whole matrix %.3e (bound %.3e)"
          % (what, worst, 2 * fig["dH_worst"], whole, 2 * fig["dH_matrix"]))
    assert worst <= 2 * fig["dH_worst"], (what, worst)
    assert whole <= 2 * fig["dH_matrix"], (what, whole)


def test_fused_data_gradient(fused, ref):
    f = fused
    _check_dH(f, f.dH1, ref["dH"], "smoothed dH un-split")
    _check_dH(f, f.dH3, ref["dH"], "smoothed dH split_k = 3")
    assert float(f.dH1[~ref["ok"]].float().abs().max()) == 0.0 and float(f.dH3[~ref["ok"]].float().abs().max()) == 0.0
    # one rounding: against its own operands in float64, elementwise
    own = (R.f64(f.fin["alpha"])[:, None] * R.f64(f.P)) @ R.f64(f.E) - R.f64(f.fin["beta"])[:, None] * R.f64(f.wsum[: f.d])[None, :]
    R.assert_elementwise(f.dH3, own, extra_abs=1e-5 * own.norm(dim=1, keepdim=True), what="smoothed dH against its own operands")


def test_data_gradient_finish_with_a_large_vector_term(fused):
    """At this shape beta wsum is 0.2 % of dH, inside every bound above; here beta is a thousand times larger, so that the two operands of
    out = bf16(alpha * sum of slabs - beta * wsum) are of one size: every element within the one-rounding rule of |a| + |b| (which bounds
    the result), plus the fp32 sum of three slabs and the two products (4 roundings of at most the operands' magnitudes)."""
    f = fused
    fin = dict(f.fin, beta=f.fin["beta"] * 1000.0)
    a = R.f64(f.fin["alpha"])[:, None] * R.f64(f.slab).sum(0)
    b = R.f64(fin["beta"])[:, None] * R.f64(f.wsum[: f.d])[None, :]
    big = R.f64(f.fin["alpha"])[:, None] * R.f64(f.slab).abs().sum(0) + b.abs()   # wsum has both signs: |a - b| reaches |a| + |b|
    for buf, ns in ((f.slab, 3), (f.acc1, 1)):
        got = f.dgrad(buf, ns, fin)
        want = a if ns == 3 else R.f64(f.fin["alpha"])[:, None] * R.f64(f.acc1)
        ex, (r, c, g, w) = R.elementwise_excess(got, want - b, (R.ELEM_RULE + 4 * U32) * big)
        assert ex <= 0.0, "nslabs %d: element (%d, %d) got %.9g want %.9g exceeds its bound by %.3g" % (ns, r, c, g, w, ex)
    ok = R.valid_labels(f.labels, f.V)
    assert float(b[ok].abs().min()) > 0 and R.rel_norm(a[ok], (a - b)[ok]) > 0.5, "the vector term must matter here"
    assert float(got[~ok].float().abs().max()) == 0.0


@pytest.mark.parametrize("which", ["dE", "dE3"])
def test_fused_weight_gradient(fused, ref, which):
    f = fused
    dE = getattr(f, which)
    assert bool((dE[f.V:] == 7.0).all()), "rows beyond V are not the launch's to write: the poison stays"
    fig = L.EMU_LS[f.eps]
    worst, whole = R.row_rel_norms(dE[: f.V], ref["dE"])
    print("smoothed %s against float64: worst row %.3e (bound %.3e), whole matrix %.3e (bound %.3e)"
          % (which, worst, 2 * fig["dE_worst"], whole, 2 * fig["dE_matrix"]))
    assert worst <= 2 * fig["dE_worst"], worst
    assert whole <= 2 * fig["dE_matrix"], whole
    # -u is visible in the rows that are nobody's label (the whole matrix is dominated by the label rows): without it the worst row misses by far
    assert R.row_rel_norms(R.f64(dE[: f.V]) - R.f64(f.fin["neg_u"])[None, :], ref["dE"])[0] > 10 * 2 * fig["dE_worst"]


def test_fused_lm_factor_scales(fused, ref):
    """the same sums finished with lm_factor = 1: losses and the stored matrix are unchanged, alpha, beta, u and both gradients are 1 / 5"""
    f = fused
    P_before = f.P.clone()
    fin1 = f.finish(1.0, f.eps)
    assert torch.equal(_bits(f.P), _bits(P_before))
    assert torch.equal(fin1["loss_rows"], f.fin["loss_rows"]) and torch.equal(fin1["srow"], f.fin["srow"])
    a5, b5 = R.f64(f.fin["alpha"]), R.f64(f.fin["beta"])
    assert bool(((R.f64(fin1["alpha"]) * f.lmf - a5).abs() <= 8 * U32 * a5).all())
    assert bool(((R.f64(fin1["beta"]) * f.lmf - b5).abs() <= 8 * U32 * b5).all())
    _check_dH(f, f.dgrad(f.slab, 3, fin1), ref["dH"] / f.lmf, "smoothed dH at lm_factor = 1")
    fig = L.EMU_LS[f.eps]
    for split in (0, 3):
        dE1 = f.wgrad(fin1, split=split)
        worst, whole = R.row_rel_norms(dE1[: f.V], ref["dE"] / f.lmf)
        assert worst <= 2 * fig["dE_worst"] and whole <= 2 * fig["dE_matrix"], (split, worst, whole)


def test_fused_all_labels_ignored():
    f = _FusedLS(all_ignored=True)
    assert int(f.count[0]) == 0
    assert float(f.P.float().abs().max()) == 0.0 and float(f.sums.abs().max()) == 0.0
    assert bool((f.fin["alpha"] == 0).all()) and bool((f.fin["beta"] == 0).all()) and float(f.fin["ah"].float().abs().max()) == 0.0
    assert bool((f.fin["neg_u"] == 0).all()), "u = 0"
    assert bool((f.fin["loss_rows"] == 0).all())
    for t in (f.dH1, f.dH3, f.dE[: f.V], f.dE3[: f.V]):
        assert not bool(torch.isnan(t.float()).any()) and float(t.float().abs().max()) == 0.0
    assert bool(torch.isnan(f.loss).all())


def test_eps_zero_is_the_old_chain(fused):
    """the new row finish and data-gradient finish at eps = 0: the bits of kmb_op_ce_rows_finish / kmb_op_ce_dgrad_finish"""
    f = fused
    lib = _lib.load()
    P_keep = f.P.clone()
    f.P.copy_(f.P_gemm)
    new = f.finish(f.lmf, 0.0)
    P_new = f.P.clone()
    f.P.copy_(f.P_gemm)
    old = f.finish(f.lmf, 0.0, smooth=False)
    P_old = f.P.clone()
    assert torch.equal(_bits(P_new), _bits(P_old))
    for k in ("loss_rows", "srow", "alpha", "ah"):
        assert torch.equal(_bits(new[k]), _bits(old[k])), k
    assert bool((new["beta"] == 0).all()) and bool((new["neg_u"] == 0).all())
    for buf, ns in ((f.acc1, 1), (f.slab, 3)):
        want = torch.full((f.M, f.d), 7.0, dtype=torch.bfloat16, device=DEV)
        check(lib.kmb_op_ce_dgrad_finish(ptr(buf), ns, f.M * f.d, ptr(old["alpha"]), ptr(want), f.M, f.d, stream()))
        assert torch.equal(_bits(f.dgrad(buf, ns, new)), _bits(want)), ns
    f.P.copy_(P_keep)
