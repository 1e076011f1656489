"""GPU: the kernels that produce the training loss and its first gradients, op by op through the C-ABI, against float64.

What runs: ce_kernel_reg<13> and the 256-thread ce_kernel (fp32 logits), ce_kernel_reg_bf16<7> / <8> (the training head, in place),
count_valid / loss_finish, and the fused tied-head chain ce_label_logit -> ce_pad_bias -> GEMM act 5 -> ce_rows_finish -> data-gradient
GEMM (un-split and split-K) -> ce_dgrad_finish, plus the weight gradient P'^T (a . H).  References and emulations: tests/loss_ref.py.

Bounds -- each is one of three things:
  * the elementwise rule for a bf16 gradient: |got - ref| <= (2^-8 + 2^-15) |ref| for EVERY element (2^-8: one round-to-nearest bf16
    rounding; 2^-15: fp32 exp / log-sum-exp at arguments below 32).  The inputs keep the label's probability below 0.9.
  * a tolerance the project already has: F32_TOL = 1e-4 of test_ops_gpu.py (fp32 results, relative); 2e-4, the row-sum tolerance of
    test_ce_fused_gpu.py (the fused chain's S; + 1e-4 for the shift = 3e-4 absolute on a fused row loss);
  * 2 x a figure of the emulation against float64, re-measured by test_loss_emulation_cpu.py at this module's shapes and seeds
    (M = 1024, V = 8150, d = 128, lm_factor = 5): dH worst row 4.12e-3 (recorded 4.2e-3 -> bound 8.4e-3), whole matrix 2.34e-3
    (2.4e-3 -> 4.8e-3); dE worst row 4.38e-3 (4.4e-3 -> 8.8e-3), whole matrix 2.37e-3 (2.4e-3 -> 4.8e-3).  The factor 2 covers fp32
    accumulation order only; a real fault (a dropped pad column, a wrong count, a skipped label correction) is an order of magnitude larger.
Exact statements (zeros in pad columns and ignored rows, bit-identical in-place / out-of-place results, ah == bf16(alpha H)) are asserted
exactly."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from kmbart import _lib  # noqa: E402
from kmbart._lib import KmbError, check, ptr  # noqa: E402
from gpu_util import DEV, gemm, rel_err, stream  # noqa: E402
import loss_ref as R  # noqa: E402

F32_TOL = R.F32_TOL
U32 = 2.0 ** -24   # fp32 unit roundoff


def _i32(n=4, fill=0):
    return torch.full((n,), fill, dtype=torch.int32, device=DEV)


def _check_ce(V, ld, labels, logits, loss_rows, dl, count, loss, scale, what):
    """shared by the fp32 and the bf16 form: everything against float64 on the values the kernel was given"""
    ref_rows, ok = R.ce_rows(logits, labels, V)
    n = int(ok.sum())
    assert int(count[0]) == n, (what, int(count[0]), n)
    err = (R.f64(loss_rows) - ref_rows).abs()
    assert bool((err <= F32_TOL * ref_rows.abs()).all()), (what, "loss_rows", float(err.max()))
    assert bool((loss_rows[~ok] == 0).all())
    want = R.ce_mean(ref_rows, ok)
    assert abs(float(loss) - float(want)) <= F32_TOL * abs(float(want)), (what, float(loss), float(want))
    if dl is None:
        return
    R.assert_elementwise(dl[:, :V], R.ce_grad(logits, labels, V, scale), what=what + " gradient")
    assert float(dl[:, V:].float().abs().max()) == 0.0, what + ": pad columns of the gradient"
    assert float(dl[~ok].float().abs().max()) == 0.0, what + ": ignored / out-of-range rows"
    assert bool((dl[ok][:, :V] != 0).any(dim=1).all())


# ------------------------------------------------------------------------------------------------ (a) fp32 logits
@pytest.mark.parametrize("V,ld", [(50320, 50432), (60000, 60032), (1601, 1608)])
def test_ce_fp32(V, ld):
    """kmb_op_ce: ce_kernel_reg<13> up to ld = 53248, the 256-thread ce_kernel above; the logits' pad columns hold NaN"""
    lib = _lib.load()
    rows, scale = 9, 3.0
    x, labels = R.ce_case(V, ld, rows, seed=V, bf16=False, pad_value=float("nan"))
    x, labels = x.to(DEV), labels.to(DEV)
    loss_rows = torch.full((rows,), 7.0, device=DEV)
    dl = torch.full((rows, ld), 7.0, dtype=torch.bfloat16, device=DEV)
    count, loss = _i32(), torch.zeros(1, device=DEV)
    check(lib.kmb_op_ce(ptr(x), ld, V, ptr(labels), rows, scale, ptr(loss_rows), ptr(dl), ptr(count), ptr(loss), stream()))
    assert float(torch.softmax(x[:, :V].double(), 1).max()) < 0.9
    _check_ce(V, ld, labels, x, loss_rows, dl, count, loss, scale, "fp32 ce V=%d" % V)


# ------------------------------------------------------------------------------------------------ (b) bf16 logits
def _run_bf16(lib, x, labels, V, ld, scale, mode):
    rows = x.shape[0]
    lg = x.clone()
    loss_rows = torch.full((rows,), 7.0, device=DEV)
    count, loss, status = _i32(), torch.zeros(1, device=DEV), _i32()
    dl = {"out": torch.full((rows, ld), 7.0, dtype=torch.bfloat16, device=DEV), "inplace": lg, "none": None}[mode]
    check(lib.kmb_op_ce_bf16(ptr(lg), ld, V, ptr(labels), rows, scale, ptr(loss_rows), ptr(dl), ptr(count), ptr(loss), ptr(status), stream()))
    return lg, dl, loss_rows, count, loss, status


@pytest.mark.parametrize("V,ld", [(50320, 50432), (57337, 57344), (57345, 57352), (65530, 65536), (129, 136)])
def test_ce_bf16(V, ld):
    """kmb_op_ce_bf16: ce_kernel_reg_bf16<7> up to ld = 57344, <8> above; out of place, in place and without a gradient; the logits'
    pad columns hold the largest finite bf16"""
    lib = _lib.load()
    scale = 3.0
    x, labels = R.ce_case(V, ld, 9, seed=V, bf16=True, pad_value=R.BF16_MAX)
    x, labels = x.to(DEV), labels.to(DEV)
    assert float(torch.softmax(x[:, :V].double(), 1).max()) < 0.9
    lg_o, dl_o, rows_o, count_o, loss_o, st_o = _run_bf16(lib, x, labels, V, ld, scale, "out")
    _check_ce(V, ld, labels, x, rows_o, dl_o, count_o, loss_o, scale, "bf16 ce V=%d out of place" % V)
    assert torch.equal(lg_o.view(torch.int16), x.view(torch.int16))            # the logits survive an out-of-place run
    assert int(st_o[0]) & 2, "labels V and a pad-range value are out of range: bit 1 of status"
    bad = (labels != R.IGNORE) & ~R.valid_labels(labels, V)
    assert int(bad.sum()) == 2 and bool((rows_o[bad] == 0).all()) and float(dl_o[bad].float().abs().max()) == 0.0
    lg_i, dl_i, rows_i, count_i, loss_i, _ = _run_bf16(lib, x, labels, V, ld, scale, "inplace")
    assert torch.equal(dl_i.view(torch.int16), dl_o.view(torch.int16)), "in place and out of place differ"
    assert torch.equal(rows_i, rows_o) and torch.equal(loss_i, loss_o) and int(count_i[0]) == int(count_o[0])
    lg_n, _, rows_n, count_n, loss_n, _ = _run_bf16(lib, x, labels, V, ld, scale, "none")
    assert torch.equal(lg_n.view(torch.int16), x.view(torch.int16)), "dlogits == nullptr must leave the logits untouched"
    assert torch.equal(rows_n, rows_o) and torch.equal(loss_n, loss_o)


def test_ce_bf16_refuses_what_it_cannot_run():
    """ld above 65536 or not a multiple of 8: an error before any launch (count, loss rows and logits keep their sentinels)"""
    lib = _lib.load()
    for V, ld in ((65540, 65544), (129, 132)):
        lg = torch.full((2, ld), 1.0, dtype=torch.bfloat16, device=DEV)
        labels = torch.zeros(2, dtype=torch.int64, device=DEV)
        loss_rows = torch.full((2,), 7.0, device=DEV)
        count, loss, status = _i32(fill=-5), torch.full((1,), 7.0, device=DEV), _i32()
        with pytest.raises(KmbError):
            check(lib.kmb_op_ce_bf16(ptr(lg), ld, V, ptr(labels), 2, 1.0, ptr(loss_rows), ptr(lg), ptr(count), ptr(loss), ptr(status), stream()))
        torch.cuda.synchronize()
        assert int(count[0]) == -5 and float(loss) == 7.0 and bool((loss_rows == 7.0).all()) and bool((lg == 1.0).all())
        assert int(status[0]) == 0


def test_ce_bf16_many_rows_mean():
    """9000 rows: count_valid and loss_finish go through their eight-way unrolled loops (8192 labels per trip) and their tails"""
    lib = _lib.load()
    V, ld, rows = 129, 136, 9000
    g = torch.Generator(device="cpu").manual_seed(9000)
    x = (torch.randn(rows, ld, generator=g) * 1.5).to(torch.bfloat16)   # sigma 1.5: no probability reaches 0.9 in 9000 rows of 129
    x[:, V:] = R.BF16_MAX
    assert float(torch.softmax(x[:, :V].double(), 1).max()) < 0.9
    labels = torch.randint(0, V, (rows,), generator=g)
    labels[::11] = R.IGNORE
    labels[8191], labels[8192], labels[8999] = R.IGNORE, V - 1, 0
    x, labels = x.to(DEV), labels.to(DEV)
    lg, dl, loss_rows, count, loss, status = _run_bf16(lib, x, labels, V, ld, 1.0, "inplace")
    ref_rows, ok = R.ce_rows(x, labels, V)
    assert int(count[0]) == int(ok.sum()) and int(status[0]) == 0
    want = float(R.ce_mean(ref_rows, ok))
    assert abs(float(loss) - want) <= F32_TOL * abs(want), (float(loss), want)
    R.assert_elementwise(dl[:, :V], R.ce_grad(x, labels, V, 1.0), what="9000 rows gradient")
    assert float(dl[:, V:].float().abs().max()) == 0.0
    cnt2, st2 = _i32(fill=-1), _i32()
    check(lib.kmb_op_count_valid(ptr(labels), rows, V, ptr(cnt2), ptr(st2), stream()))
    assert int(cnt2[0]) == int(ok.sum()) and int(st2[0]) == 0
    labels[8500] = V + 3
    check(lib.kmb_op_count_valid(ptr(labels), rows, V, ptr(cnt2), ptr(st2), stream()))
    assert int(cnt2[0]) == int(R.valid_labels(labels, V).sum()) and int(st2[0]) == 2


def test_ce_bf16_all_ignored():
    lib = _lib.load()
    V, ld = 129, 136
    x, labels = R.ce_case(V, ld, 9, seed=5, bf16=True, pad_value=R.BF16_MAX)
    labels[:] = R.IGNORE
    lg, dl, loss_rows, count, loss, status = _run_bf16(lib, x.to(DEV), labels.to(DEV), V, ld, 1.0, "inplace")
    assert int(count[0]) == 0 and int(status[0]) == 0
    assert bool(torch.isnan(loss).all()), "CrossEntropyLoss(mean) over no targets is NaN"
    assert float(dl.float().abs().max()) == 0.0 and bool((loss_rows == 0).all())


# ------------------------------------------------------------------------------------------------ (c) the fused chain
class _Fused:
    """one run of the chain on loss_ref.fused_case(); every stage's outputs kept for the stage tests"""

    def __init__(self, all_ignored=False):
        lib = _lib.load()
        c = R.FUSED
        M, V, Vpad, d = c["M"], c["V"], c["Vpad"], c["d"]
        self.M, self.V, self.Vpad, self.d, self.lmf = M, V, Vpad, d, c["lm_factor"]
        H, E, bias, labels = (t.to(DEV) for t in R.fused_case(all_ignored))
        self.H, self.E, self.bias, self.labels = H, E, bias, labels
        self.nparts = Vpad // 64
        self.shift = torch.full((M,), 7.0, device=DEV)
        self.bias_pad = torch.full((Vpad,), 7.0, device=DEV)
        check(lib.kmb_op_ce_label_logit(ptr(H), d, ptr(E), d, ptr(bias), ptr(labels), M, d, V, Vpad, ptr(self.shift), ptr(self.bias_pad), stream()))
        self.P = torch.full((M, Vpad), 7.0, dtype=torch.bfloat16, device=DEV)
        self.sums = torch.full((M, self.nparts), float("nan"), device=DEV)
        gemm(H, E, bias=self.bias_pad, act=5, out_bf16=self.P, row_shift=self.shift, row_sums=self.sums)   # no pick: as the engine runs it
        self.P_gemm = self.P.clone()
        self.count = _i32()
        check(lib.kmb_op_count_valid(ptr(labels), M, V, ptr(self.count), None, stream()))
        self.fin = self.finish(self.lmf)
        self.loss = torch.full((1,), 7.0, device=DEV)
        check(lib.kmb_op_loss_finish(ptr(self.fin["loss_rows"]), M, ptr(self.count), ptr(self.loss), stream()))
        # data gradient: P' E un-split into fp32, and with split_k = 3 into slabs (K = Vpad: E's garbage rows meet P's zero pad columns)
        self.acc1 = torch.full((M, d), float("nan"), device=DEV)
        gemm(self.P, E, b_kc=False, out_f32=self.acc1)
        self.slab = torch.full((3, M, d), float("nan"), device=DEV)
        gemm(self.P, E, b_kc=False, split_k=3, slab=self.slab)
        self.dH1, self.dH3 = self.dgrad(self.acc1, 1, self.fin["alpha"]), self.dgrad(self.slab, 3, self.fin["alpha"])
        self.dE = self.wgrad(self.fin["ah"])
        torch.cuda.synchronize()

    def finish(self, lmf):
        lib = _lib.load()
        M, d = self.M, self.d
        o = dict(loss_rows=torch.full((M,), 7.0, device=DEV), srow=torch.full((M,), 7.0, device=DEV), alpha=torch.full((M,), 7.0, device=DEV),
                 ah=torch.full((M, d), 7.0, dtype=torch.bfloat16, device=DEV))
        check(lib.kmb_op_ce_rows_finish(ptr(self.sums), self.nparts, self.nparts, None, ptr(self.labels), ptr(self.count), lmf, M, d, self.V,
                                        ptr(self.H), d, ptr(o["loss_rows"]), ptr(o["srow"]), ptr(o["alpha"]), ptr(o["ah"]), ptr(self.P),
                                        self.Vpad, stream()))
        return o

    def dgrad(self, buf, nslabs, alpha):
        out = torch.full((self.M, self.d), 7.0, dtype=torch.bfloat16, device=DEV)
        check(_lib.load().kmb_op_ce_dgrad_finish(ptr(buf), nslabs, self.M * self.d, ptr(alpha), ptr(out), self.M, self.d, stream()))
        return out

    def wgrad(self, ah):
        """dE = P'^T (a . H) over all Vpad rows of the tied matrix (the engine stops at V)"""
        out = torch.full((self.Vpad, self.d), float("nan"), device=DEV)
        gemm(self.P, ah, a_kc=False, b_kc=False, out_f32=out)
        return out


@pytest.fixture(scope="module")
def fused():
    return _Fused()


@pytest.fixture(scope="module")
def fused_ref():
    c = R.FUSED
    H, E, bias, labels = (t.to(DEV) for t in R.fused_case())
    return R.fused_ref(H, E, bias, labels, c["V"], c["lm_factor"])


def test_fused_shift_and_pad_bias(fused, fused_ref):
    f, ok = fused, fused_ref["ok"]
    lab = f.labels.clamp(0, f.V - 1)
    hh, ee = R.f64(f.H), R.f64(f.E)[lab]
    want = (hh * ee).sum(1) + R.f64(f.bias)[lab]
    # fp32 dot product of 128 bf16 x bf16 terms (each product exact in fp32): a lane chains 8 fma, the wave butterfly adds 6 levels, the
    # bias one more -- at most 15 roundings on any path, each <= 2^-24 of a partial sum that sum|h e| + |b| bounds: 16 * 2^-24 * (...)
    bound = 16 * U32 * ((hh * ee).abs().sum(1) + R.f64(f.bias)[lab].abs())
    err = (R.f64(f.shift) - want).abs()
    assert bool((err[ok] <= bound[ok]).all()), float((err[ok] - bound[ok]).max())
    assert bool((f.shift[~ok] == torch.tensor(1e30, dtype=torch.float32)).all()) and int((~ok).sum()) >= f.M // 7
    assert torch.equal(f.bias_pad[: f.V], f.bias)
    assert bool((f.bias_pad[f.V:] == torch.tensor(-1e30, dtype=torch.float32)).all())


def test_fused_loss_rows(fused, fused_ref):
    f = fused
    err = (R.f64(f.fin["loss_rows"]) - fused_ref["loss_rows"]).abs()
    # 2e-4: test_ce_fused_gpu's tolerance on the row sum S (loss = log S); 1e-4: the shift
    print("fused row loss against float64: worst %.3e absolute (bound 3e-4)" % float(err.max()))
    assert float(err.max()) <= 3e-4, float(err.max())
    assert bool((f.fin["loss_rows"][~fused_ref["ok"]] == 0).all())
    want = float(R.ce_mean(fused_ref["loss_rows"], fused_ref["ok"]))
    assert abs(float(f.loss) - want) <= F32_TOL * abs(want)
    assert int(f.count[0]) == int(fused_ref["ok"].sum())


def test_fused_rows_finish(fused, fused_ref):
    f, ok, fin = fused, fused_ref["ok"], fused.fin
    n = int(ok.sum())
    S = R.f64(f.sums).sum(1)
    # srow: 128 positive fp32 partial sums, two per lane and a 6-level butterfly: 8 roundings; alpha: a product and a quotient (4 ulp
    # leaves room for a quotient formed through the reciprocal)
    assert bool(((R.f64(fin["srow"]) - S).abs()[ok] <= 8 * U32 * S[ok]).all())
    want_alpha = f.lmf / (n * R.f64(fin["srow"]))
    assert bool(((R.f64(fin["alpha"]) - want_alpha).abs()[ok] <= 4 * U32 * want_alpha[ok]).all())
    assert bool((fin["srow"][~ok] == 0).all()) and bool((fin["alpha"][~ok] == 0).all())
    assert torch.equal(fin["ah"].view(torch.int16), (fin["alpha"][:, None] * f.H.float()).to(torch.bfloat16).view(torch.int16)), "ah != bf16(alpha H)"
    assert float(fin["ah"][~ok].float().abs().max()) == 0.0
    # only the label's entry of the stored matrix changed; the pad columns and the ignored rows are zero
    changed = f.P.view(torch.int16) != f.P_gemm.view(torch.int16)
    onehot = torch.zeros_like(changed)
    onehot[torch.arange(f.M, device=DEV)[ok], f.labels[ok]] = True
    assert bool((changed & ~onehot).sum() == 0)
    assert float(f.P[:, f.V:].float().abs().max()) == 0.0 and float(f.P[~ok].float().abs().max()) == 0.0
    # alpha P' IS the gradient row, label entry included: the one-rounding rule widened by the 2e-4 of S
    aP = R.f64(fin["alpha"])[:, None] * R.f64(f.P[:, : f.V])
    R.assert_elementwise(aP, fused_ref["G"], rel=R.ELEM_RULE + 2e-4, what="alpha P'")
    assert float(torch.softmax(fused_ref["v"], 1).max()) < 0.9


def _check_dH(f, dH, alpha, ref_dH, what):
    own = (R.f64(alpha)[:, None] * R.f64(f.P)) @ R.f64(f.E)          # from the kernel's own P' and alpha, all Vpad columns
    R.assert_elementwise(dH, own, extra_abs=1e-5 * own.norm(dim=1, keepdim=True), what=what + " against its own operands")
    worst, whole = R.row_rel_norms(dH, ref_dH)
    print("%s against float64: worst row %.3e (bound %.3e), whole matrix %.3e (bound %.3e)"
          % (what, worst, 2 * R.EMU_DH_WORST_ROW, whole, 2 * R.EMU_DH_MATRIX))
    assert worst <= 2 * R.EMU_DH_WORST_ROW, (what, worst)
    assert whole <= 2 * R.EMU_DH_MATRIX, (what, whole)


def test_fused_data_gradient(fused, fused_ref):
    f = fused
    _check_dH(f, f.dH1, f.fin["alpha"], fused_ref["dH"], "dH un-split")
    _check_dH(f, f.dH3, f.fin["alpha"], fused_ref["dH"], "dH split_k = 3")
    assert float(f.dH1[~fused_ref["ok"]].float().abs().max()) == 0.0 and float(f.dH3[~fused_ref["ok"]].float().abs().max()) == 0.0
    # the two runs differ by fp32 summation order only
    assert rel_err(f.slab.sum(0), f.acc1) < F32_TOL


def test_fused_weight_gradient(fused, fused_ref):
    f = fused
    assert float(f.dE[f.V:].abs().max()) == 0.0, "rows of the padded vocabulary must get an exactly zero gradient"
    worst, whole = R.row_rel_norms(f.dE[: f.V], fused_ref["dE"])
    print("dE against float64: worst row %.3e (bound %.3e), whole matrix %.3e (bound %.3e)"
          % (worst, 2 * R.EMU_DE_WORST_ROW, whole, 2 * R.EMU_DE_MATRIX))
    assert worst <= 2 * R.EMU_DE_WORST_ROW, worst
    assert whole <= 2 * R.EMU_DE_MATRIX, whole


def test_fused_lm_factor_scales(fused, fused_ref):
    """the same sums finished with lm_factor = 1: losses and the stored matrix are unchanged, alpha and both gradients are 1 / 5 of before"""
    f, ok = fused, fused_ref["ok"]
    P_before = f.P.clone()
    fin1 = f.finish(1.0)
    assert torch.equal(f.P.view(torch.int16), P_before.view(torch.int16))
    assert torch.equal(fin1["loss_rows"], f.fin["loss_rows"]) and torch.equal(fin1["srow"], f.fin["srow"])
    a5 = R.f64(f.fin["alpha"])
    assert bool(((R.f64(fin1["alpha"]) * f.lmf - a5).abs() <= 8 * U32 * a5).all())
    assert torch.equal(fin1["ah"].view(torch.int16), (fin1["alpha"][:, None] * f.H.float()).to(torch.bfloat16).view(torch.int16))
    _check_dH(f, f.dgrad(f.slab, 3, fin1["alpha"]), fin1["alpha"], fused_ref["dH"] / f.lmf, "dH at lm_factor = 1")
    dE1 = f.wgrad(fin1["ah"])
    worst, whole = R.row_rel_norms(dE1[: f.V], fused_ref["dE"] / f.lmf)
    assert worst <= 2 * R.EMU_DE_WORST_ROW and whole <= 2 * R.EMU_DE_MATRIX, (worst, whole)
    assert float(dE1[f.V:].abs().max()) == 0.0


def test_fused_all_labels_ignored():
    f = _Fused(all_ignored=True)
    assert int(f.count[0]) == 0
    assert bool((f.shift == torch.tensor(1e30, dtype=torch.float32)).all())
    assert float(f.P.float().abs().max()) == 0.0 and float(f.sums.abs().max()) == 0.0
    assert bool((f.fin["alpha"] == 0).all()) and float(f.fin["ah"].float().abs().max()) == 0.0
    assert float(f.dH1.float().abs().max()) == 0.0 and float(f.dH3.float().abs().max()) == 0.0
    assert float(f.dE.abs().max()) == 0.0
    assert bool(torch.isnan(f.loss).all())
