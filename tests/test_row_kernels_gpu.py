"""GPU: the row kernels between the GEMMs -- csrc/norm.hip, csrc/embed.hip, csrc/embed_row.h -- op by op through the C-ABI against float64.

References, bounds and cases: tests/row_ref.py (its docstring derives every bound).  Inputs are bf16-rounded draws of seeded CPU generators;
outputs are pre-filled with NaN and carry 64 guard elements behind their logical end, pad columns of strided operands hold NaN: a read of an
output that must not be read, a read of a pad column or a write outside the logical extent shows.  Bit-exact statements are asserted as bits.

Which case reaches which kernel (template instance):
  ln_fwd_kernel<1>            test_layernorm_forward D = 8, 72, 512 (D = 512 fills the 64 lanes, 8 and 72 leave lanes idle)
  ln_fwd_kernel<2>            D = 520 (second chunk: one lane), 768, 1024 (full)
  ln_fwd_kernel<4>            D = 1032 (third chunk: one lane, fourth idle), 2048 (full); M = 6: a two-row last block
  ln_fwd_stream_kernel<2>     test_layernorm_forward (8197, 520) and (8197, 1024): 1280 blocks, a wave walks one or two rows
  ln_fwd_slabs_kernel<1>      test_layernorm_slabs D = 72, 512;  <2>: D = 520, 1024; nslabs 1, 2, 5, 6 = no tail group, tail only, one
                              unrolled group, group + tail of add_slabs2<4>
  ln_bwd_kernel<1>            test_layernorm_backward D = 8, 72, 256;  <2>: 264;  <3>: 768;  <4>: 1024;  <8>: 1032, 2048
                              (1030, 72): four rows per block, 258 blocks; (4101, 72): five rows per block, a wave's prefetch of a second row
  reduce_parts_kernel<8>      one destination: kmb_op_ln_bwd (twice per call), kmb_op_colsum; two destinations: kmb_op_ln_bwd_sub, M <= 13
  reduce_parts_kernel<32>     (1030, 72) with 258 partial rows and (4101, 72) with 821: one destination through kmb_op_ln_bwd, two through
                              kmb_op_ln_bwd_sub
  reduce_slabs_kernel         test_reduce_slabs (the 8388636-float case: a second trip of the grid-stride loop for seven threads)
  reduce_slabs_bf16_kernel    test_reduce_slabs
  reduce_slabs_epi_kernel     test_reduce_slabs_epilogue, test_split_gemm_chain_equals_the_unsplit_epilogue
  colsum_kernel               test_column_sums: (37, 76, 80) takes the nvalid < 8 tail (76 = 9 * 8 + 4) with ld > N; (33, 64, 72) the 16-byte
                              path with ld > N; (70, 8, 8) three part rows of one chunk; (2100, 72, 72) 64 parts of 33 rows
  embed_ln_fwd_kernel<1>      test_embedding_forward D = 72;  <2>: 520, 768;  <4>: 2048
  embed_bwd_kernel            test_embedding_backward;  pos_bwd_kernel: test_position_backward ((13, 7, 768): 960 of 1024 threads work, a
                              batch stride of 7 rows; (70, 2, 8): 1024 batch lanes for 70 items)

Headroom of the bounds, measured by test_row_kernels_cpu.py (fp32 emulation with strictly sequential sums against float64, worst err / bound
over this module's cases; the fp32 part of a bound must stay <= 0.5):
  LayerNorm forward    mean 0.004   rstd 0.101   fp32 part of y 0.067   (y with its rounding 0.988)
  slabs LayerNorm      mean 0.004   rstd 0.026   fp32 part of y 0.025
  LayerNorm backward   fp32 part of dz 0.067   of out2 0.035   dgamma 0.278   dbeta 0.114   dsub 0.039   (dz, out2 with their rounding 0.994)
  embedding forward    fp32 part of z 0.479   mean 0.015   rstd 0.035   fp32 part of y 0.029   of y under dropout 0.030
  embedding backward   dE 0.363   fp32 part of dimg 0.479
  colsum 0.0001   pos_bwd 0.092   kept value of reduce_slabs_epi under dropout 0.373 (two roundings) / 0.249 (fused)
One slack was widened by its constant, as derived bounds may be when the emulation leaves less than the factor 2: dgamma's sum rule is
(n + 8) u instead of (n + 4) u (a one-row launch measured 0.5005 with n + 4: each term carries the normalised value's two roundings)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from kmbart import _lib  # noqa: E402
from kmbart._lib import KmbDrop, KmbError, check, ptr  # noqa: E402
from gpu_util import DEV, dropout_mask, gemm, stream  # noqa: E402
import row_ref as R  # noqa: E402

GUARD = 64
LN_FWD = [(M, D) for D in (8, 72, 512, 520, 768, 1024, 1032, 2048) for M in (1, 6)] + [(8197, 520), (8197, 1024)]


def dev(t):
    return None if t is None else t.to(DEV)


class Out:
    """an output pre-filled with a sentinel (NaN) with GUARD more elements behind it"""

    def __init__(self, shape, dtype, fill=R.NAN):
        self.n = 1
        for s in shape:
            self.n *= s
        self.full = torch.full((self.n + GUARD,), fill, dtype=dtype, device=DEV)
        self.t = self.full[:self.n].view(*shape)

    def cpu(self, what):
        torch.cuda.synchronize()
        assert bool(torch.isnan(self.full[self.n:].float()).all()), what + ": written behind its logical end"
        return self.t.cpu()


def drop_struct(seed):
    thr, sc = R.drop_params(R.DROP_P)
    return KmbDrop(thr, seed, sc)


def keep_mask(seed, M, N):
    return dropout_mask(seed, R.DROP_P, M, N).cpu()


def refused(call, *needles):
    with pytest.raises(KmbError) as e:
        check(call())
    for n in needles:
        assert n in str(e.value), str(e.value)


# ------------------------------------------------------------------------------------------------ LayerNorm forward
@pytest.mark.parametrize("M,D", LN_FWD)
def test_layernorm_forward(M, D):
    """kmb_op_ln_fwd: mean, rstd and y elementwise; the constant row (variance 0: rstd = eps^-1/2, y = beta) and the large-mean row ride along"""
    lib = _lib.load()
    for kind in (("random", "const", "ramp") if M == 1 else ("mixed",)):
        c = R.ln_fwd_case(M, D, kind)
        z, gamma, beta = dev(c["z"]), dev(c["gamma"]), dev(c["beta"])
        y, mean, rstd = Out((M, D), torch.bfloat16), Out((M,), torch.float32), Out((M,), torch.float32)
        check(lib.kmb_op_ln_fwd(ptr(z), ptr(gamma), ptr(beta), ptr(y.t), ptr(mean.t), ptr(rstd.t), M, D, R.EPS, stream()))
        what = "ln_fwd %dx%d %s" % (M, D, kind)
        R.check_ln_fwd(c["ref"], mean.cpu(what), rstd.cpu(what), y.cpu(what), what)


# ------------------------------------------------------------------------------------------------ LayerNorm backward
def _ln_bwd_run(lib, c, form, sub):
    M, D = c["M"], c["D"]
    d1, o2, d2 = R.form_flags(form)
    dz, out2 = Out((M, D), torch.bfloat16), Out((M, D), torch.bfloat16)
    dgb, dsub = Out((2 * D,), torch.float32), Out((D,), torch.float32)
    scratch = torch.full((int(lib.kmb_op_ln_bwd_scratch(M, D)),), R.NAN, device=DEV)
    s1, s2 = drop_struct(R.SEED_DY), drop_struct(R.SEED_OUT2)
    a = [ptr(c["dy_d"]), ptr(c["z_d"]), ptr(c["mean_d"]), ptr(c["rstd_d"]), ptr(c["gamma_d"]), ptr(dz.t), ptr(out2.t) if o2 else None,
         C.byref(s1) if d1 else None, C.byref(s2) if d2 else None, ptr(dgb.t), ptr(dgb.t[D:])]
    if sub:
        check(lib.kmb_op_ln_bwd_sub(*a, ptr(dsub.t), ptr(scratch), M, D, stream()))
    else:
        check(lib.kmb_op_ln_bwd(*a, ptr(scratch), M, D, stream()))
    what = "ln_bwd %dx%d %s" % (M, D, form)
    return dict(dz=dz.cpu(what), out2=out2.cpu(what), dgb=dgb.cpu(what), dsub=dsub.cpu(what))


@pytest.mark.parametrize("M,D,form", R.LN_BWD_CASES)
def test_layernorm_backward(M, D, form):
    """kmb_op_ln_bwd_sub (one reduce_parts2 launch, as a training step reduces) and kmb_op_ln_bwd (reduce_parts twice): dz elementwise, out2
    zero exactly where the mask drops, dgamma / dbeta / dsub per column, and the two reductions agree bit for bit"""
    lib = _lib.load()
    c = dict(R.ln_bwd_inputs(M, D))
    for k in ("dy", "z", "mean", "rstd", "gamma"):
        c[k + "_d"] = dev(c[k])
    d1, o2, d2 = R.form_flags(form)
    _, sc = R.drop_params(R.DROP_P)
    keep1 = keep_mask(R.SEED_DY, M, D) if d1 else None
    keep2 = keep_mask(R.SEED_OUT2, M, D) if d2 else None
    ref = R.ln_bwd_ref(c["dy"], c["z"], c["mean"], c["rstd"], c["gamma"], keep1=keep1, scale1=sc, with_out2=o2, keep2=keep2, scale2=sc)
    got = _ln_bwd_run(lib, c, form, sub=True)
    what = "ln_bwd %dx%d %s" % (M, D, form)
    R.assert_elementwise(got["dz"], ref["dz"], R.bf16_bound(ref["dz"], ref["dz_slack"]), what + " dz")
    if not o2:
        assert bool(torch.isnan(got["out2"].float()).all()), what + ": out2 written without being asked for"
    elif not d2:
        assert R.same_bits(got["out2"], got["dz"]), what + ": out2 without a mask must have dz's bits"
    else:
        assert bool((got["out2"][~keep2] == 0).all()) and not bool(torch.isnan(got["out2"].float()).any()), what + ": out2 where the mask drops"
        assert bool((got["out2"][keep2] != 0).float().mean() > 0.99), what + ": out2 where the mask keeps"
        R.assert_elementwise(got["out2"], ref["out2"], R.bf16_bound(ref["out2"], ref["out2_slack"]), what + " out2")
    R.assert_elementwise(got["dgb"][:D], ref["dgamma"], ref["dgamma_bound"], what + " dgamma")
    R.assert_elementwise(got["dgb"][D:], ref["dbeta"], ref["dbeta_bound"], what + " dbeta")
    R.assert_elementwise(got["dsub"], ref["dsub"], ref["dsub_bound"], what + " dsub")
    old = _ln_bwd_run(lib, c, form, sub=False)
    assert R.same_bits(old["dgb"], got["dgb"]), what + ": reduce_parts twice and reduce_parts2 once differ in dgamma | dbeta"
    assert R.same_bits(old["dz"], got["dz"]) and bool(torch.isnan(old["dsub"]).all())
    if o2:
        assert R.same_bits(old["out2"], got["out2"])


def test_layernorm_backward_sub_refuses_what_it_cannot_run():
    lib = _lib.load()
    M, D = 5, 72
    c = R.ln_bwd_inputs(M, D)
    dy, z, mean, rstd, gamma = (dev(c[k]) for k in ("dy", "z", "mean", "rstd", "gamma"))
    dz, dgb, dsub = Out((M, D), torch.bfloat16), Out((2 * D + 8,), torch.float32), Out((D,), torch.float32)
    scratch = torch.full((int(lib.kmb_op_ln_bwd_scratch(M, D)),), R.NAN, device=DEV)

    def call(dy_=dy, dsub_=dsub.t, dbeta=dgb.t[D:], D_=D):
        return lambda: lib.kmb_op_ln_bwd_sub(ptr(dy_), ptr(z), ptr(mean), ptr(rstd), ptr(gamma), ptr(dz.t), None, None, None, ptr(dgb.t), ptr(dbeta),
                                             ptr(dsub_), ptr(scratch), M, D_, stream())
    refused(call(dsub_=None), "kmb_op_ln_bwd_sub", "required")
    refused(call(dbeta=dgb.t[D + 8:]), "dgamma + D")
    refused(call(D_=68), "multiple of 8")
    refused(call(dy_=dy.view(-1)[1:]), "aligned")
    for o in (dz, dgb, dsub):
        assert bool(torch.isnan(o.cpu("refused ln_bwd_sub").float()).all())


# ------------------------------------------------------------------------------------------------ slabs LayerNorm
def _ln_slabs_call(lib, c, y, D=None, residual=True):
    bias = dev(c["bias"])
    t = [dev(c["slabs"]), dev(c["res"]), dev(c["gamma"]), dev(c["beta"]), bias]
    return t, lambda: lib.kmb_op_ln_fwd_slabs(ptr(t[0]), c["nslabs"], c["stride"], ptr(bias), ptr(t[1]) if residual else None, c["D"] + 8, ptr(t[2]),
                                              ptr(t[3]), ptr(y.t), c["R"], c["D"] if D is None else D, R.EPS, stream())


@pytest.mark.parametrize("nslabs", (1, 2, 5, 6))
@pytest.mark.parametrize("D", (72, 512, 520, 1024))
def test_layernorm_slabs(D, nslabs):
    """kmb_op_ln_fwd_slabs: stride > R D, ld_res = D + 8, bias null and given; the pre-LayerNorm bf16 row is exact, y takes the forward bounds"""
    lib = _lib.load()
    for with_bias in (False, True):
        c = R.ln_slabs_case(D, nslabs, with_bias)
        y = Out((c["R"], D), torch.bfloat16)
        keep, call = _ln_slabs_call(lib, c, y)
        check(call())
        what = "ln_fwd_slabs D=%d nslabs=%d bias=%d" % (D, nslabs, with_bias)
        R.check_ln_fwd(c["ref"], None, None, y.cpu(what), what)


def test_layernorm_slabs_refuses_what_it_cannot_run():
    lib = _lib.load()
    c = R.ln_slabs_case(1024, 2, True)
    y = Out((c["R"], 1032), torch.bfloat16)
    keep, call = _ln_slabs_call(lib, c, y, D=1032)
    refused(call, "kmb_op_ln_fwd_slabs", "at most 1024")
    keep, call = _ln_slabs_call(lib, c, y, residual=False)
    refused(call, "kmb_op_ln_fwd_slabs", "residual")
    assert bool(torch.isnan(y.cpu("refused ln_fwd_slabs").float()).all())


# ------------------------------------------------------------------------------------------------ slab reducers
RED_N, RED_PAD = 3096, 12      # 387 float4 pairs: two blocks, the second ragged; stride = n + 12


@pytest.mark.parametrize("nslabs", (1, 2, 8, 9, 10))
def test_reduce_slabs(nslabs):
    """kmb_op_reduce_slabs (beta 0, 0.5, 1) and kmb_op_reduce_slabs_bf16: the bits of the sequential fp32 sum in slice order (beta a power of two:
    one possible result); nslabs 1, 2, 8, 9, 10 = nothing to add, tail only, tail of seven, one unrolled group of add_slabs<8>, group + tail"""
    lib = _lib.load()
    c = R.reduce_case(nslabs, RED_N, RED_PAD)
    slabs = dev(c["slabs"])
    for beta in (0.0, 0.5, 1.0):
        out = Out((RED_N,), torch.float32)
        if beta != 0.0:
            out.t.copy_(c["start"])
        check(lib.kmb_op_reduce_slabs(ptr(slabs), nslabs, c["stride"], ptr(out.t), RED_N, beta, stream()))
        assert R.same_bits(out.cpu("reduce_slabs"), R.reduce_expect(c, beta)), "reduce_slabs nslabs=%d beta=%g" % (nslabs, beta)
    ob = Out((RED_N,), torch.bfloat16)
    check(lib.kmb_op_reduce_slabs_bf16(ptr(slabs), nslabs, c["stride"], ptr(ob.t), RED_N, stream()))
    assert R.same_bits(ob.cpu("reduce_slabs_bf16"), c["total"].to(torch.bfloat16)), "reduce_slabs_bf16 nslabs=%d" % nslabs


def test_reduce_slabs_second_trip_and_refusals():
    """n = 8192 * 256 * 4 + 28 floats: the grid is capped at 8192 blocks and seven threads take a second trip; ragged n is refused"""
    lib = _lib.load()
    n = 8192 * 256 * 4 + 28
    slabs = torch.randn(2, n + 4, generator=R.gen(4100))
    want = slabs[0, :n] + slabs[1, :n]
    sd = dev(slabs)
    out = Out((n,), torch.float32)
    check(lib.kmb_op_reduce_slabs(ptr(sd), 2, n + 4, ptr(out.t), n, 0.0, stream()))
    got = out.cpu("reduce_slabs second trip")
    assert R.same_bits(got, want), "first differing element %d" % int(torch.nonzero(got.view(torch.int32) != want.view(torch.int32))[0])
    small, ob = Out((RED_N,), torch.float32), Out((RED_N,), torch.bfloat16)
    refused(lambda: lib.kmb_op_reduce_slabs(ptr(sd), 2, n + 4, ptr(small.t), RED_N - 2, 0.0, stream()), "kmb_op_reduce_slabs", "multiples of 4")
    refused(lambda: lib.kmb_op_reduce_slabs_bf16(ptr(sd), 2, n + 4, ptr(ob.t), RED_N - 4, stream()), "kmb_op_reduce_slabs_bf16", "multiple of 8")
    refused(lambda: lib.kmb_op_reduce_slabs(ptr(sd), 2, n + 3, ptr(small.t), RED_N, 0.0, stream()), "stride")
    refused(lambda: lib.kmb_op_reduce_slabs(ptr(sd.view(-1)[1:]), 2, n + 4, ptr(small.t), RED_N, 0.0, stream()), "aligned")
    assert bool(torch.isnan(small.cpu("refused")).all()) and bool(torch.isnan(ob.cpu("refused").float()).all())


def _epi_run(lib, c, sd, bias_d, res_d, with_bias, csn, drop, with_res):
    M, N = c["M"], c["N"]
    out = Out((M, N + 16), torch.bfloat16)
    check(lib.kmb_op_reduce_slabs_epi(ptr(sd), c["nslabs"], c["stride"], ptr(bias_d) if with_bias else None, R.EPI_SCALE, csn,
                                      C.byref(drop) if drop is not None else None, ptr(res_d) if with_res else None, N + 8, ptr(out.t), N + 16, M, N,
                                      stream()))
    o = out.cpu("reduce_slabs_epi")
    assert bool(torch.isnan(o[:, N:].float()).all()), "reduce_slabs_epi wrote a pad column of its output"
    return o[:, :N]


EPI_SEED = 4242


@pytest.mark.parametrize("nslabs", (1, 3, 5, 6))
@pytest.mark.parametrize("M,N", [(5, 72), (130, 768)])
def test_reduce_slabs_epilogue(M, N, nslabs):
    """kmb_op_reduce_slabs_epi: bias on / off, col_scale = 0.125 over 0, 20 (inside an 8-column chunk) and N columns, residual with
    ld_res = N + 8 and without, ld_out = N + 16.  Without dropout: the bits of ((sum + bias) * scale) + residual rounded to bf16.  With
    p = 0.1: kmb_op_dropout_mask's zero pattern exactly (a dropped element is the residual's bits, or +0 without one) and the bf16 rule
    on the kept values (the compiler may fuse v * scale + residual)"""
    lib = _lib.load()
    c = R.epi_case(M, N, nslabs)
    sd, bias_d, res_d = dev(c["slabs"]), dev(c["bias"]), dev(c["res"])
    keep = keep_mask(EPI_SEED, M, N)
    _, sc = R.drop_params(R.DROP_P)
    res = c["res"][:, :N]
    for with_bias in (False, True):
        for csn in (0, 20, N):
            w = R.epi_pre_drop(c, with_bias, csn)
            for with_res in (True, False):
                what = "reduce_slabs_epi %dx%d nslabs=%d bias=%d csn=%d res=%d" % (M, N, nslabs, with_bias, csn, with_res)
                r32 = res.float() if with_res else torch.zeros(M, N)
                got = _epi_run(lib, c, sd, bias_d, res_d, with_bias, csn, None, with_res)
                assert R.same_bits(got, (w + r32).to(torch.bfloat16)), what
                got = _epi_run(lib, c, sd, bias_d, res_d, with_bias, csn, drop_struct(EPI_SEED), with_res)
                assert R.same_bits(got[~keep], r32.to(torch.bfloat16)[~keep]), what + ": dropped elements"
                if not with_res:
                    assert bool((got[keep] != 0).all()), what + ": a kept element is zero"
                r = torch.where(keep, R.f64(w) * sc, torch.zeros(M, N, dtype=torch.float64)) + R.f64(r32)
                slack = torch.where(keep, 4 * R.U * ((R.f64(w) * sc).abs() + R.f64(r32).abs()), torch.zeros(M, N, dtype=torch.float64))
                R.assert_elementwise(got, r, R.bf16_bound(r, slack), what + " dropout")


def test_reduce_slabs_epilogue_refusals():
    lib = _lib.load()
    c = R.epi_case(5, 72, 3)
    sd, res_d = dev(c["slabs"]), dev(c["res"])
    out = Out((5, 88), torch.bfloat16)

    def call(N=72, stride=c["stride"], ld_res=80, ld_out=88, slabs=sd, o=out.t):
        return lambda: lib.kmb_op_reduce_slabs_epi(ptr(slabs), 3, stride, None, 1.0, 0, None, ptr(res_d), ld_res, ptr(o), ld_out, 5, N, stream())
    refused(call(N=68), "kmb_op_reduce_slabs_epi", "multiples of 8")
    refused(call(stride=c["stride"] + 2), "stride")
    refused(call(ld_res=84), "ld_res")
    refused(call(ld_out=84), "ld_out")
    refused(call(slabs=None), "required")
    refused(call(o=out.t.view(-1)[4:]), "aligned")
    assert bool(torch.isnan(out.cpu("refused").float()).all())


def test_split_gemm_chain_equals_the_unsplit_epilogue():
    """(M, N, K) = (130, 136, 256): a split-K kmb_op_gemm into two slabs + kmb_op_reduce_slabs_epi against the un-split kmb_op_gemm with the
    same bias, q-scale, dropout and residual: both meet the bf16 rule against the float64 product, with the same zero pattern"""
    lib = _lib.load()
    M, N, K, csn, seed = 130, 136, 256, 20, 515
    g = R.gen(5150)
    A, B = torch.randn(M, K, generator=g).to(torch.bfloat16), (torch.randn(N, K, generator=g) * 0.2).to(torch.bfloat16)
    bias = torch.randn(N, generator=g) * 0.3
    res = torch.full((M, N + 8), R.NAN, dtype=torch.bfloat16)
    res[:, :N] = torch.randn(M, N, generator=g).to(torch.bfloat16)
    Ad, Bd, bias_d, res_d = dev(A), dev(B), dev(bias), dev(res)
    one = Out((M, N + 16), torch.bfloat16)
    gemm(Ad, Bd, bias=bias_d, col_scale=R.EPI_SCALE, col_scale_n=csn, drop_p=R.DROP_P, drop_seed=seed, residual=res_d[:, :N], out_bf16=one.t[:, :N])
    slab = torch.full((2, M * N), R.NAN, device=DEV)
    gemm(Ad, Bd, split_k=2, slab=slab)
    two = Out((M, N + 16), torch.bfloat16)
    dr = drop_struct(seed)
    check(lib.kmb_op_reduce_slabs_epi(ptr(slab), 2, M * N, ptr(bias_d), R.EPI_SCALE, csn, C.byref(dr), ptr(res_d), N + 8, ptr(two.t), N + 16, M, N,
                                      stream()))
    keep = keep_mask(seed, M, N)
    _, sc = R.drop_params(R.DROP_P)
    cs = torch.ones(N, dtype=torch.float64)
    cs[:csn] = R.EPI_SCALE
    prod, mag = R.f64(A) @ R.f64(B).t(), R.f64(A).abs() @ R.f64(B).abs().t()
    v = (prod + R.f64(bias)) * cs * sc
    r = torch.where(keep, v, torch.zeros_like(v)) + R.f64(res[:, :N])
    # the fp32 product: the sum rule over K terms (+ the bias), then the epilogue's multiply and add as in the reducer's own test
    slack = torch.where(keep, (K + 4) * R.U * (mag + R.f64(bias).abs()) * cs * sc + 4 * R.U * (v.abs() + R.f64(res[:, :N]).abs()), torch.zeros_like(v))
    for name, o in (("un-split gemm", one), ("split gemm + reduce_slabs_epi", two)):
        got = o.cpu(name)
        assert bool(torch.isnan(got[:, N:].float()).all()), name + ": pad columns"
        R.assert_elementwise(got[:, :N], r, R.bf16_bound(r, slack), name)
        assert R.same_bits(got[:, :N][~keep], res[:, :N][~keep]), name + ": a dropped element is the residual"
        assert bool(((got[:, :N].float() - res[:, :N].float()) != 0)[keep].float().mean() > 0.99), name + ": kept elements"


# ------------------------------------------------------------------------------------------------ colsum, pos_bwd
@pytest.mark.parametrize("M,N,ld", R.COLSUM_CASES)
def test_column_sums(M, N, ld):
    """kmb_op_colsum per column; columns N .. ld of X hold NaN"""
    lib = _lib.load()
    c = R.colsum_case(M, N, ld)
    X = dev(c["X"])
    out = Out((N,), torch.float32)
    scratch = torch.full((int(lib.kmb_op_colsum_scratch(M, N)),), R.NAN, device=DEV)
    check(lib.kmb_op_colsum(ptr(X), ld, M, N, ptr(out.t), ptr(scratch), stream()))
    R.assert_elementwise(out.cpu("colsum"), c["ref"], c["bound"], "colsum %dx%d ld=%d" % (M, N, ld))


@pytest.mark.parametrize("B,S,D", R.POS_CASES)
def test_position_backward(B, S, D):
    """kmb_op_pos_bwd: rows outside [pos_base, pos_base + S) exactly 0, the window per element, two runs the same bits"""
    lib = _lib.load()
    c = R.pos_case(B, S, D)
    dz = dev(c["dz"])
    runs = []
    for _ in range(2):
        dP = Out((c["rows"], D), torch.float32)
        check(lib.kmb_op_pos_bwd(ptr(dz), B, S, D, ptr(dP.t), R.POS_BASE, c["rows"], stream()))
        runs.append(dP.cpu("pos_bwd"))
    got = runs[0]
    assert R.same_bits(got, runs[1]), "pos_bwd: two runs differ"
    zero = torch.zeros(1, D)
    assert R.same_bits(got[:R.POS_BASE], zero.expand(R.POS_BASE, D).contiguous()) and R.same_bits(got[R.POS_BASE + S:], zero.expand(R.POS_EXTRA, D).contiguous())
    R.assert_elementwise(got[R.POS_BASE:R.POS_BASE + S], c["ref"], c["bound"], "pos_bwd %dx%dx%d" % (B, S, D))


# ------------------------------------------------------------------------------------------------ embedding
EMB_SEED = 313


def _embed_fwd(lib, c, t, full, drop):
    M, D = c["M"], c["D"]
    y = Out((M, D), torch.bfloat16)
    z, mean, rstd = (Out((M, D), torch.bfloat16), Out((M,), torch.float32), Out((M,), torch.float32)) if full else (None, None, None)
    check(lib.kmb_op_embed_ln_fwd(ptr(t["ids"]), ptr(t["img_src"]), ptr(t["E"]), ptr(t["img"]), ptr(t["P"]), R.POS_BASE, R.EMB_S, c["scale"],
                                  ptr(t["gamma"]), ptr(t["beta"]), ptr(z.t) if full else None, ptr(y.t), ptr(mean.t) if full else None,
                                  ptr(rstd.t) if full else None, M, D, R.EPS, C.byref(drop) if drop is not None else None, stream()))
    w = "embed_ln_fwd"
    return (y.cpu(w),) + ((z.cpu(w), mean.cpu(w), rstd.cpu(w)) if full else ())


@pytest.mark.parametrize("D", (72, 520, 768, 2048))
def test_embedding_forward(D):
    """kmb_op_embed_ln_fwd at B S = 2 * 5, pos_base = 2, token and region rows.  scale = 1: z is exactly bf16(E + P); scale = sqrt(D): z's bound.
    mean / rstd / y against the statistics of the UNROUNDED row (row_ref.py).  z = mean = rstd = NULL (the decode form): the same y bits.
    Dropout p = 0.1: kmb_op_dropout_mask's zero pattern and the bf16 rule on scale_drop * y"""
    lib = _lib.load()
    _, sc = R.drop_params(R.DROP_P)
    for scaled in (False, True):
        c = R.embed_fwd_case(D, scaled)
        t = {k: dev(c[k]) for k in ("ids", "img_src", "E", "img", "P", "gamma", "beta")}
        ref = c["ref"]
        what = "embed_ln_fwd D=%d scale=%.4g" % (D, c["scale"])
        y, z, mean, rstd = _embed_fwd(lib, c, t, True, None)
        if not scaled:
            assert R.same_bits(z, (c["rows"] + c["prow"]).to(torch.bfloat16)), what + ": z must be exactly bf16(E + P)"
        R.assert_elementwise(z, ref["z"], R.bf16_bound(ref["z"], ref["z_slack"]), what + " z")
        R.check_ln_fwd(ref, mean, rstd, y, what)
        (y2,) = _embed_fwd(lib, c, t, False, None)
        assert R.same_bits(y2, y), what + ": the decode form (z = mean = rstd = NULL) changes y"
        (y3,) = _embed_fwd(lib, c, t, False, drop_struct(EMB_SEED))
        keep = keep_mask(EMB_SEED, c["M"], D)
        assert bool((y3[~keep] == 0).all()) and bool((y3[keep] != 0).all()), what + ": zero pattern under dropout"
        r = torch.where(keep, ref["y"] * sc, torch.zeros_like(ref["y"]))
        slack = torch.where(keep, ref["y_slack"] * sc + 2 * R.U * r.abs(), torch.zeros_like(r))
        R.assert_elementwise(y3, r, R.bf16_bound(r, slack), what + " y under dropout")


@pytest.mark.parametrize("D", (72, 768))
def test_embedding_backward(D):
    """kmb_op_embed_bwd, M = 4 * 37 rows, V = 50: one id 40 times, pad rows, region rows; dE = its random start + the sum (the sum rule with
    n = the id's count); untouched vocabulary rows and dimg rows no position refers to keep their bits; dimg exact at scale = 1"""
    lib = _lib.load()
    for scaled in (False, True):
        c = R.embed_bwd_case(D, scaled)
        what = "embed_bwd D=%d scale=%.4g" % (D, c["scale"])
        dE, dimg = Out((R.EMBB_V, D), torch.float32), Out((R.EMBB_NIMG, D), torch.bfloat16)
        dE.t.copy_(c["dE0"])
        dimg.t.copy_(c["dimg0"])
        dz, ids, img_src = dev(c["dz"]), dev(c["ids"]), dev(c["img_src"])
        check(lib.kmb_op_embed_bwd(ptr(dz), ptr(ids), ptr(img_src), c["scale"], ptr(dE.t), ptr(dimg.t), R.EMBB_PAD, c["M"], D, stream()))
        gE, gI = dE.cpu(what), dimg.cpu(what)
        assert R.same_bits(gE[~c["touched"]], c["dE0"][~c["touched"]]), what + ": a vocabulary row without a token changed"
        assert int((~c["touched"]).sum()) >= 8 and not bool(c["touched"][R.EMBB_PAD])
        R.assert_elementwise(gE, c["dE"], c["dE_bound"], what + " dE")
        other = torch.ones(R.EMBB_NIMG, dtype=torch.bool)
        other[c["dimg_rows"]] = False
        assert int(other.sum()) == 3 and R.same_bits(gI[other], c["dimg0"][other]), what + ": a dimg row no position refers to changed"
        if not scaled:
            assert R.same_bits(gI[c["dimg_rows"]], c["dz"][c["sel"]]), what + ": dimg must be dz's rows exactly at scale = 1"
        R.assert_elementwise(gI[c["dimg_rows"]], c["dimg"], R.bf16_bound(c["dimg"], 2 * R.U * c["dimg"].abs()), what + " dimg")
