"""GPU: the pre-training heads' kernels (csrc/heads.hip) and the GEMM shapes / epilogues only they request, op by op through the C-ABI,
against float64 at the real class counts (1601 region classes, 129 here for the small heads; logits rows padded to 1608 / 136).

kl_div, gather_rows_bf16, scatter_add_rows, add_f32_into_bf16, mean_rows; KmbGemm act 3 (tanh) and act 4 (times 1 - aux^2); forward
GEMMs with N = 1601 / 129 into fp32 rows of 1608 / 136; the weight gradient with 1601 / 129 output rows; the data gradient that reduces
over the padded class dimension; kmb_op_colsum over 1601 of 1608 columns; and one whole MRM head composed from these calls as
engine_train.cpp head_run composes it, against float64 autograd of the same head (reference src/model/model.py:133-158, :248-258).

Bounds: F32_TOL / BF_TOL of test_ops_gpu.py; for bf16 outputs additionally every element within one bf16 rounding (2^-8 + 2^-15 of the
float64 value) plus the worst-case fp32 accumulation error of its own dot product, K * 2^-24 * sum |a| |b|; for the KL gradient the same
rounding rule relative to the larger operand of its subtraction; for the composed head 2 x the emulation's figure, re-measured by
test_loss_emulation_cpu.py (loss_ref.EMU_HEAD: d_out_w 2.17e-3, d_out_b 1.57e-3, d_dense_w 2.83e-3, d_dense_b 2.81e-3, d_states 2.98e-3,
worst d_states row 4.30e-3 -- recorded there rounded up, doubled here).  Row movers are exact."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from kmbart import _lib  # noqa: E402
from kmbart._lib import KmbError, check, ptr  # noqa: E402
from gpu_util import DEV, gemm, rel_err, stream  # noqa: E402
import loss_ref as R  # noqa: E402

BF_TOL = 4e-3     # tests/test_ops_gpu.py
F32_TOL = R.F32_TOL
U32 = 2.0 ** -24


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def bfr(*shape, scale=1.0, seed=0):
    return rnd(*shape, scale=scale, seed=seed).to(torch.bfloat16)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


# ------------------------------------------------------------------------------------------------ kl_div
def _targets(rows, C, ldt, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    t = torch.softmax(torch.randn(rows, C, generator=g) * 2.0, dim=1)     # dense soft labels
    if rows >= 5:
        t[1] = 0.0
        t[1, C // 2] = 1.0                                                 # one-hot
        t[2, ::3] = 0.0                                                    # exact zeros among soft labels
        t[2] /= t[2].sum()
        t[3] *= 0.6                                                        # sums to 0.6
    out = torch.full((rows, ldt), float("nan"))
    out[:, :C] = t
    return out.to(DEV)


@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("C,ldd", [(1601, 1608), (129, 136), (7, 8), (256, 256), (257, 264)])
def test_kl_div(C, ldd, rows):
    lib = _lib.load()
    ldt, scale = C + 3, 2.0
    x = torch.full((rows, ldd), float("nan"), device=DEV)
    x[:, :C] = rnd(rows, C, scale=2.0, seed=C + rows)
    t = _targets(rows, C, ldt, seed=C)
    loss_rows = torch.full((rows,), 7.0, device=DEV)
    dl = torch.full((rows, ldd), 7.0, dtype=torch.bfloat16, device=DEV)
    check(lib.kmb_op_kl_div(ptr(x), ldd, C, ptr(t), ldt, rows, scale, ptr(loss_rows), ptr(dl), ldd, stream()))
    ref_rows, ref_grad, big = R.kl_ref(x, t, C, scale)
    err = (R.f64(loss_rows) - ref_rows).abs()
    assert bool((err <= F32_TOL * ref_rows.abs()).all()), (float(err.max()), ref_rows.tolist())
    # the subtraction sum(t) p - t may cancel: one rounding relative to the larger operand
    ex, where = R.elementwise_excess(dl[:, :C], ref_grad, R.ELEM_RULE * big)
    assert ex <= 0.0, ("kl gradient (row, col, got, want)", where, ex)
    if ldd > C:
        assert float(dl[:, C:].float().abs().max()) == 0.0
    loss2 = torch.full((rows,), 7.0, device=DEV)
    check(lib.kmb_op_kl_div(ptr(x), ldd, C, ptr(t), ldt, rows, scale, ptr(loss2), None, ldd, stream()))
    assert torch.equal(loss2, loss_rows)


# ------------------------------------------------------------------------------------------------ row movers
@pytest.mark.parametrize("rows,cols,src_rows", [(5, 72, 3), (203, 768, 640), (11000, 768, 500)])
def test_gather_rows_bf16(rows, cols, src_rows):
    """exact, repeated indices; written into one half of rows twice as wide (the relation head's object | subject layout); 11000 x 768 is
    more than 4096 workgroups of 256 chunks: the grid-stride loop"""
    lib = _lib.load()
    src_ld = cols + 8
    src = bfr(src_rows, src_ld, seed=rows)
    g = torch.Generator(device="cpu").manual_seed(rows)
    idx = torch.randint(0, src_rows, (rows,), generator=g).to(torch.int32)
    idx[: min(4, rows)] = src_rows - 1
    idx = idx.to(DEV)
    dst = torch.full((rows, 2 * cols), 7.0, dtype=torch.bfloat16, device=DEV)
    right = dst[:, cols:]
    check(lib.kmb_op_gather_rows_bf16(ptr(src), src_ld, ptr(idx), ptr(right), 2 * cols, rows, cols, stream()))
    want = src[idx.long()][:, :cols]
    assert _same_bits(dst[:, cols:], want)
    assert bool((dst[:, :cols] == 7.0).all()), "columns outside the written half must survive"
    check(lib.kmb_op_gather_rows_bf16(ptr(src), src_ld, ptr(idx), ptr(dst), 2 * cols, rows, cols, stream()))
    assert _same_bits(dst[:, :cols], want) and _same_bits(dst[:, cols:], want)


def test_gather_rows_bf16_refuses_ragged_columns():
    lib = _lib.load()
    src, dst = bfr(4, 80, seed=1), torch.full((4, 80), 7.0, dtype=torch.bfloat16, device=DEV)
    idx = torch.zeros(4, dtype=torch.int32, device=DEV)
    with pytest.raises(KmbError):
        check(lib.kmb_op_gather_rows_bf16(ptr(src), 80, ptr(idx), ptr(dst), 80, 4, 76, stream()))
    torch.cuda.synchronize()
    assert bool((dst == 7.0).all())


@pytest.mark.parametrize("cols", [768, 72])
@pytest.mark.parametrize("rows", [1, 4, 5, 203])
def test_scatter_add_rows(rows, cols):
    """fp32 atomics onto a non-zero accumulator; heavy repeats (forty source rows into one target at 203 rows)"""
    lib = _lib.load()
    targets, src_ld = 64, cols + 8
    src = bfr(rows, src_ld, seed=rows + cols)
    g = torch.Generator(device="cpu").manual_seed(rows)
    idx = torch.randint(0, targets, (rows,), generator=g).to(torch.int32)
    idx[: min(40, rows)] = 17
    idx = idx.to(DEV)
    acc0 = rnd(targets, cols, seed=3)
    acc = acc0.clone()
    check(lib.kmb_op_scatter_add_rows(ptr(src), src_ld, ptr(idx), ptr(acc), rows, cols, stream()))
    want = R.f64(acc0).index_add_(0, idx.long(), R.f64(src[:, :cols]))
    mag = R.f64(acc0).abs().index_add_(0, idx.long(), R.f64(src[:, :cols]).abs())
    assert bool(((R.f64(acc) - want).abs() <= 1e-5 * mag).all())
    untouched = torch.ones(targets, dtype=torch.bool, device=DEV)
    untouched[idx.long()] = False
    assert torch.equal(acc[untouched], acc0[untouched])


@pytest.mark.parametrize("n", [8, 8 * 4096 * 256 + 8000])
def test_add_f32_into_bf16(n):
    """exact; the larger size is past 4096 workgroups x 256 threads x 8 elements: the grid-stride loop"""
    lib = _lib.load()
    y0, a = bfr(n, seed=1), rnd(n, scale=0.3, seed=2)
    y = y0.clone()
    check(lib.kmb_op_add_f32_into_bf16(ptr(y), ptr(a), n, stream()))
    assert _same_bits(y, (y0.float() + a).to(torch.bfloat16))


def test_add_f32_into_bf16_refuses_ragged_length():
    lib = _lib.load()
    y, a = torch.full((16,), 7.0, dtype=torch.bfloat16, device=DEV), torch.ones(16, device=DEV)
    with pytest.raises(KmbError):
        check(lib.kmb_op_add_f32_into_bf16(ptr(y), ptr(a), 12, stream()))
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())


@pytest.mark.parametrize("n", [1, 4, 257, 5000])
def test_mean_rows(n):
    lib = _lib.load()
    x = rnd(n, seed=n).abs() + 0.1
    out = torch.full((1,), 7.0, device=DEV)
    check(lib.kmb_op_mean_rows(ptr(x), n, 0.25, float(n), ptr(out), stream()))
    want = 0.25 * float(R.f64(x).sum()) / n
    assert abs(float(out) - want) <= F32_TOL * abs(want)


# ------------------------------------------------------------------------------------------------ head GEMM shapes and epilogues
def _acc_bound(A, B, bias=None):
    """worst-case fp32 accumulation error of A B^T (+ bias), whatever the order: K roundings of partial sums bounded by sum |a| |b|"""
    m = R.f64(A).abs() @ R.f64(B).abs().t()
    if bias is not None:
        m = m + R.f64(bias).abs()
    return A.shape[1] * U32 * m


@pytest.mark.parametrize("n,din", [(203, 768), (5, 1536)])
def test_gemm_tanh_epilogue(n, din):
    """act 3: the heads' dense layer (d_in = 2 d for the relation head)"""
    d = 768
    x, W, b = bfr(n, din, seed=1), bfr(d, din, scale=0.03, seed=2), rnd(d, scale=0.02, seed=3)
    out = torch.full((n, d), 7.0, dtype=torch.bfloat16, device=DEV)
    gemm(x, W, bias=b, act=3, out_bf16=out)
    ref = torch.tanh(R.f64(x) @ R.f64(W).t() + R.f64(b))
    assert rel_err(out, ref) < BF_TOL
    R.assert_elementwise(out, ref, extra_abs=_acc_bound(x, W, b), what="tanh epilogue")


@pytest.mark.parametrize("C,Cpad", [(1601, 1608), (129, 136)])
def test_gemm_tanh_backward_epilogue_over_padded_classes(C, Cpad):
    """act 4 on the data gradient that reduces over K = Cpad: dlogits' pad columns are zero, the weight rows they meet are not"""
    n, d = 203, 768
    dl = torch.zeros((n, Cpad), dtype=torch.bfloat16, device=DEV)
    dl[:, :C] = bfr(n, C, scale=1e-3, seed=4)
    W = bfr(Cpad, d, scale=0.05, seed=5)
    W[C:] = 3.0
    y = torch.tanh(rnd(n, d, seed=6)).to(torch.bfloat16)
    out = torch.full((n, d), 7.0, dtype=torch.bfloat16, device=DEV)
    gemm(dl, W, b_kc=False, act=4, aux=y, out_bf16=out)
    ref = (R.f64(dl[:, :C]) @ R.f64(W[:C])) * (1.0 - R.f64(y) ** 2)
    assert rel_err(out, ref) < BF_TOL
    R.assert_elementwise(out, ref, extra_abs=_acc_bound(dl, W.t()), what="act 4 epilogue")


@pytest.mark.parametrize("C,Cpad", [(1601, 1608), (129, 136)])
def test_head_gemm_shapes(C, Cpad):
    """out_proj forward into padded fp32 rows (pad untouched), its weight gradient with C output rows, the bias gradient's column sums"""
    lib = _lib.load()
    n, d = 203, 768
    y, W, b = bfr(n, d, scale=0.5, seed=7), bfr(C, d, scale=0.05, seed=8), rnd(C, scale=0.02, seed=9)
    lg = torch.full((n, Cpad), 7.0, device=DEV)
    gemm(y, W, bias=b, out_f32=lg)
    assert rel_err(lg[:, :C], R.f64(y) @ R.f64(W).t() + R.f64(b)) < F32_TOL
    assert bool((lg[:, C:] == 7.0).all()), "the pad columns of the logits rows are not the GEMM's to write"
    dl = torch.zeros((n, Cpad), dtype=torch.bfloat16, device=DEV)
    dl[:, :C] = bfr(n, C, scale=1e-3, seed=10)
    dW = torch.full((C + 1, d), 7.0, device=DEV)
    gemm(dl, y, a_kc=False, b_kc=False, M=C, out_f32=dW)
    assert rel_err(dW[:C], R.f64(dl[:, :C]).t() @ R.f64(y)) < F32_TOL
    assert bool((dW[C] == 7.0).all()), "row C of the gradient buffer belongs to the next parameter"
    db = torch.full((Cpad,), 7.0, device=DEV)
    scratch = torch.empty(int(lib.kmb_op_colsum_scratch(n, C)), device=DEV)
    check(lib.kmb_op_colsum(ptr(dl), Cpad, n, C, ptr(db), ptr(scratch), stream()))
    assert rel_err(db[:C], R.f64(dl[:, :C]).sum(0)) < F32_TOL
    assert bool((db[C:] == 7.0).all())


# ------------------------------------------------------------------------------------------------ one whole head
def test_mrm_head_composed_like_head_run():
    """gather -> dense + tanh -> out_proj -> kl_div + mean -> bias / weight gradients -> act 4 data gradient -> dense gradients -> scatter-add
    -> add into the decoder-state gradient, n = 203, d = 768, C = 1601, against float64 autograd of the same head on the same weights"""
    lib = _lib.load()
    c = R.HEAD
    n, d, C, Cpad, T, factor = c["n"], c["d"], c["C"], c["Cpad"], c["rows_total"], c["factor"]
    k = {name: t.to(DEV) for name, t in R.head_case().items()}
    ref = R.head_ref(k)
    Wo = torch.full((Cpad, d), 3.0, dtype=torch.bfloat16, device=DEV)      # rows C.. : what follows the matrix in memory, finite
    Wo[:C] = k["Wo"]
    hx = torch.full((n, d), 7.0, dtype=torch.bfloat16, device=DEV)
    check(lib.kmb_op_gather_rows_bf16(ptr(k["hdec"]), d, ptr(k["rows"]), ptr(hx), d, n, d, stream()))
    hy = torch.empty((n, d), dtype=torch.bfloat16, device=DEV)
    gemm(hx, k["Wd"], bias=k["bd"], act=3, out_bf16=hy)
    hlg = torch.full((n, Cpad), float("nan"), device=DEV)
    gemm(hy, Wo[:C], bias=k["bo"], out_f32=hlg)
    hloss, loss = torch.empty(n, device=DEV), torch.empty(1, device=DEV)
    hdlg = torch.full((n, Cpad), 7.0, dtype=torch.bfloat16, device=DEV)
    check(lib.kmb_op_kl_div(ptr(hlg), Cpad, C, ptr(k["tgt"]), C, n, factor, ptr(hloss), ptr(hdlg), Cpad, stream()))
    check(lib.kmb_op_mean_rows(ptr(hloss), n, factor, float(n), ptr(loss), stream()))
    got = {}
    scratch = torch.empty(int(lib.kmb_op_colsum_scratch(n, max(C, d))), device=DEV)
    got["d_out_b"] = torch.empty(C, device=DEV)
    check(lib.kmb_op_colsum(ptr(hdlg), Cpad, n, C, ptr(got["d_out_b"]), ptr(scratch), stream()))
    got["d_out_w"] = torch.empty((C, d), device=DEV)
    gemm(hdlg, hy, a_kc=False, b_kc=False, M=C, out_f32=got["d_out_w"])
    hdy = torch.empty((n, d), dtype=torch.bfloat16, device=DEV)
    gemm(hdlg, Wo, b_kc=False, act=4, aux=hy, out_bf16=hdy)
    got["d_dense_b"] = torch.empty(d, device=DEV)
    check(lib.kmb_op_colsum(ptr(hdy), d, n, d, ptr(got["d_dense_b"]), ptr(scratch), stream()))
    got["d_dense_w"] = torch.empty((d, d), device=DEV)
    gemm(hdy, hx, a_kc=False, b_kc=False, out_f32=got["d_dense_w"])
    hdx = torch.empty((n, d), dtype=torch.bfloat16, device=DEV)
    gemm(hdy, k["Wd"], b_kc=False, out_bf16=hdx)
    dhead = torch.zeros((T, d), device=DEV)
    check(lib.kmb_op_scatter_add_rows(ptr(hdx), d, ptr(k["rows"]), ptr(dhead), n, d, stream()))
    got["d_states"] = k["dhdec"].clone()
    check(lib.kmb_op_add_f32_into_bf16(ptr(got["d_states"]), ptr(dhead), T * d, stream()))
    torch.cuda.synchronize()
    assert abs(float(loss) - float(ref["loss"])) <= F32_TOL * abs(float(ref["loss"])), (float(loss), float(ref["loss"]))
    assert rel_err(hlg[:, :C], ref["logits"]) < BF_TOL        # carries tanh's bf16 rounding
    for name, figure in R.EMU_HEAD.items():
        err = R.rel_norm(got[name], ref[name])
        print("MRM head %-10s kernel against float64 %.3e (emulation %.3e, bound %.3e)" % (name, err, figure, 2 * figure))
        assert err <= 2 * figure, (name, err)
    worst, _ = R.row_rel_norms(got["d_states"], ref["d_states"])
    print("MRM head d_states worst row %.3e (bound %.3e)" % (worst, 2 * R.EMU_HEAD_STATES_WORST_ROW))
    assert worst <= 2 * R.EMU_HEAD_STATES_WORST_ROW, worst
    untouched = torch.ones(T, dtype=torch.bool, device=DEV)
    untouched[k["rows"].long()] = False
    assert _same_bits(got["d_states"][untouched], k["dhdec"][untouched])
