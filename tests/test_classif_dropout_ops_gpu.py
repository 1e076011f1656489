"""GPU: what classification-head dropout adds below the engine, op by op through the C-ABI.

1. kmb_op_gather_rows_drop_bf16 (csrc/heads.hip) is exact: every destination element is bf16_rne(fp32(src) * scale) where the read-back mask
   (kmb_op_dropout_mask at the DESTINATION coordinate) keeps it and +0 elsewhere; one index array, two (the relation head's object | subject
   halves of one row, one launch), identity rows (into another buffer and in place); with thr16 = 0 the bits of kmb_op_gather_rows_bf16.
2. The two GEMM launches head_run requests with dropout, through kmb_op_gemm against float64 at M = 203: act 4 (times 1 - aux^2) with the mask
   behind it, K = 1608 and 136; the data-gradient layout with the mask and no residual, N = 768 and 1536.  Element rule of
   test_heads_ops_gpu.py: one bf16 rounding (2^-8 + 2^-15 of the float64 value) plus K * 2^-24 * sum |a| |b|; dropped elements exactly zero.
3. One whole head composed from these calls as engine_train.cpp head_run composes it under dropout, against float64 autograd of
   out_proj(m_h . tanh(dense(m_in . x))) under the read-back masks: the MRM shape (n = 203, d = 768, C = 1601, KL divergence) and a
   relation-shaped head (d_in = 1536, C = 129, cross-entropy).  Bounds: 2 x the emulation's figure (head_dropout_ref.EMU*, re-measured by
   test_head_dropout_emulation_cpu.py) for every quantity, the loss included (kernels against float64, measured: MRM loss 2.9e-5 relative
   against a bound of 5.6e-5, relation loss 4.1e-5 against 1.42e-4)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from kmbart import _lib  # noqa: E402
from kmbart._lib import KmbDrop, KmbError, check, ptr  # noqa: E402
from gpu_util import DEV, dropout_mask, gemm, rel_err, stream  # noqa: E402
import head_dropout_ref as HD  # noqa: E402
import loss_ref as R  # noqa: E402

BF_TOL = 4e-3     # tests/test_ops_gpu.py
U32 = 2.0 ** -24
P = HD.THR16 / 65536.0     # exactly representable: kmb_op_dropout_mask's lrintf(p * 65536) gives THR16 back


def bfr(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV).to(torch.bfloat16)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def _drop(seed, thr16=HD.THR16):
    return KmbDrop(thr16, seed, HD.SCALE if thr16 else 1.0)


def _gather_drop(src, src_ld, idx_a, idx_b, dst, dst_ld, rows, cols, drop):
    lib = _lib.load()
    check(lib.kmb_op_gather_rows_drop_bf16(ptr(src), src_ld, ptr(idx_a), ptr(idx_b), ptr(dst), dst_ld, rows, cols,
                                           C.byref(drop) if drop is not None else None, stream()))


def _expected(gathered, keep):
    """bf16_rne(fp32(v) * scale) where kept, +0 elsewhere"""
    scaled = (gathered.float() * torch.tensor(HD.SCALE, dtype=torch.float32, device=DEV)).to(torch.bfloat16)
    return torch.where(keep, scaled, torch.zeros_like(scaled))


def _indices(rows, src_rows, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    idx = torch.randint(0, src_rows, (rows,), generator=g).to(torch.int32)
    idx[: min(4, rows)] = src_rows - 1        # repeats, and the last source row
    return idx.to(DEV)


# ------------------------------------------------------------------------------------------------ the row kernel
@pytest.mark.parametrize("rows,cols,src_rows", [(5, 72, 3), (203, 768, 640), (11000, 768, 500)])
def test_gather_rows_drop_one_index_array(rows, cols, src_rows):
    """11000 x 768 is more than 4096 workgroups of 256 chunks: the grid-stride loop"""
    src_ld, dst_ld, seed = cols + 8, cols + 16, 0x1234567 + rows
    src = bfr(src_rows, src_ld, seed=rows)
    idx = _indices(rows, src_rows, rows)
    dst = torch.full((rows, dst_ld), 7.0, dtype=torch.bfloat16, device=DEV)
    _gather_drop(src, src_ld, idx, None, dst, dst_ld, rows, cols, _drop(seed))
    keep = dropout_mask(seed, P, rows, cols)
    assert _same_bits(dst[:, :cols], _expected(src[idx.long()][:, :cols], keep))
    assert bool((dst[:, cols:] == 7.0).all()), "columns outside the written ones must survive"
    assert abs(float(keep.float().mean()) - 0.9) < 0.05


@pytest.mark.parametrize("rows,cols,src_rows", [(5, 72, 3), (203, 768, 640)])
def test_gather_rows_drop_two_index_arrays_share_one_mask(rows, cols, src_rows):
    """both halves of 2 * cols wide rows in one launch: the mask is the one of a [rows, 2 cols] matrix"""
    src_ld, dst_ld, seed = cols + 8, 2 * cols + 16, 0x2345678 + rows
    src = bfr(src_rows, src_ld, seed=rows + 1)
    ia, ib = _indices(rows, src_rows, rows + 2), _indices(rows, src_rows, rows + 3).flip(0).contiguous()
    dst = torch.full((rows, dst_ld), 7.0, dtype=torch.bfloat16, device=DEV)
    _gather_drop(src, src_ld, ia, ib, dst, dst_ld, rows, cols, _drop(seed))
    keep = dropout_mask(seed, P, rows, 2 * cols)
    want = torch.cat([src[ia.long()][:, :cols], src[ib.long()][:, :cols]], dim=1)
    assert _same_bits(dst[:, :2 * cols], _expected(want, keep))
    assert bool((dst[:, 2 * cols:] == 7.0).all())
    assert not torch.equal(keep[:, :cols], keep[:, cols:])


@pytest.mark.parametrize("rows,cols", [(5, 72), (203, 768), (11000, 768)])
def test_gather_rows_drop_identity_rows(rows, cols):
    """no index array: a matrix masked into another buffer, and in place"""
    ld, dst_ld, seed = cols + 8, cols + 16, 0x3456789 + rows
    src = bfr(rows, ld, seed=rows + 5)
    src0 = src.clone()
    dst = torch.full((rows, dst_ld), 7.0, dtype=torch.bfloat16, device=DEV)
    _gather_drop(src, ld, None, None, dst, dst_ld, rows, cols, _drop(seed))
    want = _expected(src0[:, :cols], dropout_mask(seed, P, rows, cols))
    assert _same_bits(dst[:, :cols], want) and bool((dst[:, cols:] == 7.0).all())
    assert _same_bits(src, src0)
    _gather_drop(src, ld, None, None, src, ld, rows, cols, _drop(seed))
    assert _same_bits(src[:, :cols], want) and _same_bits(src[:, cols:], src0[:, cols:])


@pytest.mark.parametrize("rows,cols,src_rows", [(5, 72, 3), (203, 768, 640)])
def test_gather_rows_drop_without_dropout_is_the_plain_gather(rows, cols, src_rows):
    lib = _lib.load()
    src_ld, dst_ld = cols + 8, 2 * cols
    src = bfr(src_rows, src_ld, seed=rows + 7)
    src[src_rows - 1, 0], src[src_rows - 1, 1] = float("nan"), -0.0        # (a row every index array holds) bits a multiply need not preserve
    ia, ib = _indices(rows, src_rows, rows + 8), _indices(rows, src_rows, rows + 9).flip(0).contiguous()
    plain = torch.full((rows, dst_ld), 7.0, dtype=torch.bfloat16, device=DEV)
    check(lib.kmb_op_gather_rows_bf16(ptr(src), src_ld, ptr(ia), ptr(plain), dst_ld, rows, cols, stream()))
    check(lib.kmb_op_gather_rows_bf16(ptr(src), src_ld, ptr(ib), ptr(plain[:, cols:]), dst_ld, rows, cols, stream()))
    for drop in (None, _drop(99, thr16=0)):
        dst = torch.full((rows, dst_ld), 7.0, dtype=torch.bfloat16, device=DEV)
        _gather_drop(src, src_ld, ia, ib, dst, dst_ld, rows, cols, drop)
        assert _same_bits(dst, plain)
        one = torch.full((rows, dst_ld), 7.0, dtype=torch.bfloat16, device=DEV)
        _gather_drop(src, src_ld, ia, None, one, dst_ld, rows, cols, drop)
        assert _same_bits(one[:, :cols], plain[:, :cols]) and bool((one[:, cols:] == 7.0).all())
        same = torch.full((src_rows, dst_ld), 7.0, dtype=torch.bfloat16, device=DEV)       # identity rows: a strided copy ...
        _gather_drop(src, src_ld, None, None, same, dst_ld, src_rows, cols, drop)
        assert _same_bits(same[:, :cols], src[:, :cols]) and bool((same[:, cols:] == 7.0).all())
        before = src.clone()                                                                # ... and nothing at all in place
        _gather_drop(src, src_ld, None, None, src, src_ld, src_rows, cols, drop)
        assert _same_bits(src, before)


def test_gather_rows_drop_refuses_bad_shapes():
    src, dst = bfr(4, 80, seed=1), torch.full((4, 160), 7.0, dtype=torch.bfloat16, device=DEV)
    idx = torch.zeros(4, dtype=torch.int32, device=DEV)
    for args in ((src, 80, idx, None, dst, 160, 4, 76),      # ragged columns
                 (src, 80, idx, idx, dst, 152, 4, 80),       # two halves do not fit the destination row
                 (src, 72, idx, None, dst, 160, 4, 80),      # source rows narrower than the columns
                 (src, 80, idx, None, dst, 160, 0, 80)):
        with pytest.raises(KmbError, match="kmb_op_gather_rows_drop_bf16"):
            _gather_drop(*args, _drop(5))
    with pytest.raises(KmbError, match="kmb_op_gather_rows_drop_bf16"):
        _gather_drop(src, 80, idx, None, dst, 160, 4, 80, KmbDrop(65536, 5, 1.0))
    # in place only with identity rows (a gather in place would race), and no second half beside identity rows: with and without a mask
    wide = torch.full((4, 160), 7.0, dtype=torch.bfloat16, device=DEV)
    for drop in (_drop(5), None):
        for ia, ib in ((idx, None), (idx, idx)):
            with pytest.raises(KmbError, match="identity rows only"):
                _gather_drop(wide, 160, ia, ib, wide, 160, 4, 80, drop)
        with pytest.raises(KmbError, match="idx_b needs idx_a"):
            _gather_drop(src, 80, None, idx, dst, 160, 4, 80, drop)
    torch.cuda.synchronize()
    assert bool((dst == 7.0).all()) and bool((wide == 7.0).all())


# ------------------------------------------------------------------------------------------------ the two GEMM requests
def _acc_bound(A, B):
    """worst-case fp32 accumulation error of A B^T, whatever the order: K roundings of partial sums bounded by sum |a| |b|"""
    return A.shape[1] * U32 * (R.f64(A).abs() @ R.f64(B).abs().t())


@pytest.mark.parametrize("C_,Cpad", [(1601, 1608), (129, 136)])
def test_gemm_tanh_backward_epilogue_with_dropout(C_, Cpad):
    """act 4 on the data gradient that reduces over K = Cpad, then the mask: d_pre = m_h . (dlogits W_o) . (1 - t^2)"""
    n, d, seed = 203, 768, 0x51515 + C_
    dl = torch.zeros((n, Cpad), dtype=torch.bfloat16, device=DEV)
    dl[:, :C_] = bfr(n, C_, scale=1e-3, seed=4)
    W = bfr(Cpad, d, scale=0.05, seed=5)
    W[C_:] = 3.0
    y = torch.tanh(bfr(n, d, seed=6).float()).to(torch.bfloat16)
    out = torch.full((n, d), 7.0, dtype=torch.bfloat16, device=DEV)
    gemm(dl, W, b_kc=False, act=4, aux=y, drop_p=P, drop_seed=seed, out_bf16=out)
    keep = dropout_mask(seed, P, n, d)
    ref = (R.f64(dl[:, :C_]) @ R.f64(W[:C_])) * (1.0 - R.f64(y) ** 2) * (R.f64(keep) * HD.SCALE)
    assert bool((out[~keep].view(torch.int16) == 0).all()), "dropped elements are +0"
    assert rel_err(out, ref) < BF_TOL
    R.assert_elementwise(out, ref, extra_abs=_acc_bound(dl, W.t()), what="act 4 + dropout")
    plain = torch.empty_like(out)
    gemm(dl, W, b_kc=False, act=4, aux=y, out_bf16=plain)
    assert bool((plain[~keep] != 0).float().mean() > 0.99), "the mask, not the data, zeroes them"


@pytest.mark.parametrize("N", [768, 1536])
def test_gemm_data_gradient_with_dropout_and_no_residual(N):
    """d_x = m_in . (d_pre W_d): the data-gradient layout (B stored [K, N]) with the mask and nothing behind it"""
    n, K, seed = 203, 768, 0x61616 + N
    dy, W = bfr(n, K, scale=1e-3, seed=7), bfr(K, N, scale=0.03, seed=8)
    out = torch.full((n, N), 7.0, dtype=torch.bfloat16, device=DEV)
    gemm(dy, W, b_kc=False, drop_p=P, drop_seed=seed, out_bf16=out)
    keep = dropout_mask(seed, P, n, N)
    ref = (R.f64(dy) @ R.f64(W)) * (R.f64(keep) * HD.SCALE)
    assert bool((out[~keep].view(torch.int16) == 0).all()), "dropped elements are +0"
    assert rel_err(out, ref) < BF_TOL
    R.assert_elementwise(out, ref, extra_abs=_acc_bound(dy, W.t()), what="data gradient + dropout")


# ------------------------------------------------------------------------------------------------ one whole head under dropout
@pytest.mark.parametrize("name", ["mrm", "rel"])
def test_head_composed_like_head_run_under_dropout(name):
    """gather with m_in -> dense + tanh -> m_h into a second buffer -> out_proj -> loss -> bias / weight gradients from the masked buffers -> act 4
    data gradient with m_h -> dense gradients -> data gradient with m_in -> scatter-add -> add into the decoder-state gradient"""
    lib = _lib.load()
    k = HD.case(name)
    n, d, din, C_, Cpad, T, factor = (k[x] for x in ("n", "d", "din", "C", "Cpad", "rows_total", "factor"))
    kd = {key: (v.to(DEV) if torch.is_tensor(v) else v) for key, v in k.items()}
    kd["rows"] = [r.to(DEV) for r in k["rows"]]
    seed_in, seed_h = 0x7001 + din, 0x7002 + din
    m_in, m_h = dropout_mask(seed_in, P, n, din), dropout_mask(seed_h, P, n, d)
    ref = HD.head_ref(kd, m_in, m_h)
    Wo = torch.full((Cpad, d), 3.0, dtype=torch.bfloat16, device=DEV)      # rows C.. : what follows the matrix in memory, finite
    Wo[:C_] = kd["Wo"]
    rows_a, rows_b = kd["rows"][0], (kd["rows"][1] if len(kd["rows"]) > 1 else None)
    hx = torch.full((n, din), 7.0, dtype=torch.bfloat16, device=DEV)
    _gather_drop(kd["hdec"], d, rows_a, rows_b, hx, din, n, d, _drop(seed_in))
    hy = torch.empty((n, d), dtype=torch.bfloat16, device=DEV)
    gemm(hx, kd["Wd"], bias=kd["bd"], act=3, out_bf16=hy)
    hyd = torch.full((n, d), 7.0, dtype=torch.bfloat16, device=DEV)
    _gather_drop(hy, d, None, None, hyd, d, n, d, _drop(seed_h))
    hlg = torch.full((n, Cpad), float("nan"), device=DEV)
    gemm(hyd, Wo[:C_], bias=kd["bo"], out_f32=hlg)
    hloss, loss = torch.empty(n, device=DEV), torch.empty(1, device=DEV)
    hdlg = torch.full((n, Cpad), 7.0, dtype=torch.bfloat16, device=DEV)
    if "tgt" in kd:
        check(lib.kmb_op_kl_div(ptr(hlg), Cpad, C_, ptr(kd["tgt"]), C_, n, factor, ptr(hloss), ptr(hdlg), Cpad, stream()))
    else:
        count, unused = torch.zeros(4, dtype=torch.int32, device=DEV), torch.empty(1, device=DEV)
        check(lib.kmb_op_ce(ptr(hlg), Cpad, C_, ptr(kd["labels"]), n, factor, ptr(hloss), ptr(hdlg), ptr(count), ptr(unused), stream()))
    check(lib.kmb_op_mean_rows(ptr(hloss), n, factor, float(n), ptr(loss), stream()))
    got = {}
    scratch = torch.empty(int(lib.kmb_op_colsum_scratch(n, max(C_, d))), device=DEV)
    got["d_out_b"] = torch.empty(C_, device=DEV)
    check(lib.kmb_op_colsum(ptr(hdlg), Cpad, n, C_, ptr(got["d_out_b"]), ptr(scratch), stream()))
    got["d_out_w"] = torch.empty((C_, d), device=DEV)
    gemm(hdlg, hyd, a_kc=False, b_kc=False, M=C_, out_f32=got["d_out_w"])
    hdy = torch.empty((n, d), dtype=torch.bfloat16, device=DEV)
    gemm(hdlg, Wo, b_kc=False, act=4, aux=hy, drop_p=P, drop_seed=seed_h, out_bf16=hdy)
    got["d_dense_b"] = torch.empty(d, device=DEV)
    check(lib.kmb_op_colsum(ptr(hdy), d, n, d, ptr(got["d_dense_b"]), ptr(scratch), stream()))
    got["d_dense_w"] = torch.empty((d, din), device=DEV)
    gemm(hdy, hx, a_kc=False, b_kc=False, out_f32=got["d_dense_w"])
    hdx = torch.empty((n, din), dtype=torch.bfloat16, device=DEV)
    gemm(hdy, kd["Wd"], b_kc=False, drop_p=P, drop_seed=seed_in, out_bf16=hdx)
    dhead = torch.zeros((T, d), device=DEV)
    check(lib.kmb_op_scatter_add_rows(ptr(hdx), din, ptr(rows_a), ptr(dhead), n, d, stream()))
    if rows_b is not None:
        check(lib.kmb_op_scatter_add_rows(ptr(hdx[:, d:]), din, ptr(rows_b), ptr(dhead), n, d, stream()))
    got["d_states"] = kd["dhdec"].clone()
    check(lib.kmb_op_add_f32_into_bf16(ptr(got["d_states"]), ptr(dhead), T * d, stream()))
    torch.cuda.synchronize()
    assert bool((hx[~m_in].view(torch.int16) == 0).all()) and bool((hyd[~m_h].view(torch.int16) == 0).all())
    assert bool((hdy[~m_h].view(torch.int16) == 0).all()) and bool((hdx[~m_in].view(torch.int16) == 0).all())
    loss_err = abs(float(loss) - float(ref["loss"])) / abs(float(ref["loss"]))
    loss_bound = 2 * HD.EMU_LOSS[name]
    print("%s head loss %.6f float64 %.6f relative %.3e (bound %.3e)" % (name, float(loss), float(ref["loss"]), loss_err, loss_bound))
    assert loss_err <= loss_bound, (float(loss), float(ref["loss"]))
    for q, figure in HD.EMU[name].items():
        err = R.rel_norm(got[q], ref[q])
        print("%s head %-10s kernel against float64 %.3e (emulation %.3e, bound %.3e)" % (name, q, err, figure, 2 * figure))
        assert err <= 2 * figure, (q, err)
    worst, _ = R.row_rel_norms(got["d_states"], ref["d_states"])
    print("%s head d_states worst row %.3e (bound %.3e)" % (name, worst, 2 * HD.EMU_WORST_ROW[name]))
    assert worst <= 2 * HD.EMU_WORST_ROW[name], worst
    untouched = torch.ones(T, dtype=torch.bool, device=DEV)
    untouched[torch.cat(kd["rows"]).long()] = False
    assert _same_bits(got["d_states"][untouched], kd["dhdec"][untouched])
