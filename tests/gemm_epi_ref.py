"""float64 reference, derived per-element bounds, fp32 emulation and seeded cases of the GEMM epilogues: csrc/gemm.hip
(gemm_epilogue_body, the narrow kernel's epilogue, the persistent kernels' lean and wave epilogues), gemm_lean.hip, gemm_pair.hip.
A helper module of test_gemm_epilogue_cpu.py and test_gemm_epilogue_gpu.py.  The functions are device-agnostic torch: a case is built on
the CPU from a CPU generator seeded by the case's index, the GPU module moves it to the device (to_device) and calls the same exact() there.
The judging helpers are row_ref.py's, so that the row kernels and the GEMMs are judged by one piece of code.

OPERATION ORDER (gemm_epilogue_body), float64 in exact():
    t = (A.B + bias) * scale_j          scale_j = col_scale for j < col_scale_n, else 1
    act 1: v = t Phi(t), stored derivative d = Phi(t) + t phi(t)  (exact erf)       act 2: v = t aux
    act 3: v = tanh t                                                               act 4: v = t (1 - aux^2)
    dropout: v = keep ? v * drop_scale : 0  (the fp32 drop_scale the kernel is handed); GeLU with dropout: d likewise
    v += residual;  column sums are of THIS v (before the output's rounding);  fp32 output = v + beta * old
    split-K: the slabs summed are the product alone.

BOUNDS, derived (u = 2^-24, fp32's unit roundoff; every "further fp32 operation" on a value r adds 2 u |r|: one rounding reaches u just
above a power of two and the slack keeps a factor 2, as in row_ref.py):
    accumulator            s0 = (K + 1) u mag,  mag = sum_k |a_ik b_kj| in float64   (any order of an fp32 sum of K exact products; the rule of
                                                                                      test_gemm_kstep_tail_gpu.py)
    t                      s_t = (s0 + 2 u |A.B + bias|) scale_j + 2 u |t|           (the add, the multiply)
    Phi as computed        dPhi = 0.75e-7 + 24 u h + 2 u,  h = min(Phi, 1 - Phi)     0.75e-7: half of common.h's 1.5e-7 on the A-S 7.1.26 erf.
                           24 u relative on h = poly * t * e / 2: t = rcp(1 + p z) carries z's and the fma's rounding and the 1-ulp
                           v_rcp_f32 (4 u); poly(t) moves at most 2.5 times as fast as t (10 u) and its four fmas round intermediates of at
                           most 1.46 against poly >= 0.23, weighted by the powers of t <= 1 behind them (4.2 u); the 1-ulp v_exp_f32 (2 u); three
                           multiplies (3 u).  2 u absolute: the exponent z z log2(e) carries 4 u relative, so e moves by 4 u ln2 |arg| e, and
                           |arg| 2^-|arg| <= 0.53 (0.74 u after the factor 1/2), plus the rounding of 1 - h (u).
    act 1, v               LIP1 s_t + s_t^2 + |t| dPhi + 2 u |v|                     LIP1 = 1.13 >= max |GeLU'|; |GeLU''| / 2 <= 0.40 < 1
    act 1, derivative      LIP2 s_t + s_t^2 + dPhi + |t phi| (4 u ln2 |arg| + 8 u) + 2 u (|Phi| + |t phi|)
                                                                                     LIP2 = 0.80 >= max |GeLU''|; |GeLU'''| / 2 <= 0.40 < 1
    act 2                  s_t |aux| + 2 u |v|
    act 3                  LIP_TANH s_t + TANH_ULP 2 u |v|                           LIP_TANH = 1; TANH_ULP = 8 ulp of tanhf: an ASSUMPTION (no
                                                                                     device-libs accuracy table ships with the toolchain)
    act 4                  s_t |1 - aux^2| + 4 u |t| + 2 u |v|                       (aux^2 is exact in fp32; 1 - aux^2 rounds once)
    dropout                s drop_scale + 2 u |v| on kept elements, 0 on dropped ones (they are exactly 0)
    residual               s + 2 u |v|
    fp32 output, beta      s + 2 u |beta old| + 2 u |out|
    a bf16 output          bf16_bound(ref, s)            an fp32 output: s itself
    column sums, n rows    sum_bound(n, sum |v|) + the summed slack of the terms     judged per 256-row band: its four 64-row partial rows folded
                                                                                     in float64 (every variant's tile or wave block divides 256)

EMULATION emulate(): the same chain in torch fp32 with a strictly sequential K sum (row_ref.seq_sum), the A-S polynomial with gelu_parts'
constants in explicit fp32 operations, exact division and exp2 in place of v_rcp_f32 / v_exp_f32.  `mut` applies ONE deliberate slip
(MUTATIONS) so that test_gemm_epilogue_cpu.py can show the reference sees it."""
import functools
import math

import torch

from row_ref import U, f64, gen, NAN, drop_params, seq_sum, assert_elementwise, bf16_bound, sum_bound, same_bits  # noqa: F401 (re-exported)

LIP1, LIP2, LIP_TANH, TANH_ULP = 1.13, 0.80, 1.0, 8
AS_PHI = 0.75e-7
COL_SCALE = 0.125
DROP_P = 0.1
BAND = 256

MUTATIONS = ("bias_after_scale", "scale_n_plus1", "scale_n_minus1", "bias_shift_last8", "poly_const", "no_tphi", "drop_after_res",
             "res_row_plus1", "act4_linear", "beta_ignored", "colsum_skip_row", "skip_kstep", "pad_nan")
# what a bf16 output cannot show (below 2^-8 of the value): the argument for running every class with an fp32 output too
BF16_BLIND = ("poly_const",)          # GeLU moves by at most 1.8e-5 (near t = 1): 2^-8 * 0.84 = 3.3e-3 hides it
NO_BF16_FORM = ("beta_ignored", "colsum_skip_row")      # beta and the column sums exist in fp32 only


def up8(v):
    return (v + 7) & ~7


# ------------------------------------------------------------------------------------------------ the case matrix
def _spec(name, M, N, K, layout, **kw):
    s = dict(name=name, M=M, N=N, K=K, layout=layout, bias=False, csn=0, act=0, preact=False, drop=0.0, res=False, cs=False, bf16=True,
             f32=False, ldf32="pad", beta=0.0, split=0, wide=0)
    s.update(kw)
    return s


def _classes(M, N, K, tag):
    """the 21 classes of group S at one shape, each in the layout the engine launches it with"""
    n = lambda c: "%s_%s" % (tag, c)
    kk, kt, tt = "kk", "kt", "tt"
    both = dict(f32=True)
    return [
        _spec(n("c01_plain"), M, N, K, kk),
        _spec(n("c02_bias_ld4"), M, N, K, kk, bias=True, **both),
        _spec(n("c02_bias_ldodd"), M, N, K, kk, bias=True, f32=True, ldf32="odd"),
        _spec(n("c03_scale64"), M, N, K, kk, bias=True, csn=64, **both),
        _spec(n("c03_scale20"), M, N, K, kk, bias=True, csn=20, **both),
        _spec(n("c03_scaleN"), M, N, K, kk, bias=True, csn=N, **both),
        _spec(n("c04_gelu_pre"), M, N, K, kk, bias=True, act=1, preact=True, **both),
        _spec(n("c04_gelu_nopre"), M, N, K, kk, bias=True, act=1, **both),
        _spec(n("c05_gelu_drop"), M, N, K, kk, bias=True, act=1, preact=True, drop=DROP_P),
        _spec(n("c06_drop_res"), M, N, K, kk, bias=True, drop=DROP_P, res=True, **both),
        _spec(n("c07_res"), M, N, K, kk, bias=True, res=True, **both),
        _spec(n("c08_tanh"), M, N, K, kk, bias=True, act=3, **both),
        _spec(n("c09_gelu_res"), M, N, K, kk, bias=True, act=1, res=True, **both),
        _spec(n("c10_kt_plain"), M, N, K, kt, **both),
        _spec(n("c11_kt_res"), M, N, K, kt, res=True, **both),
        _spec(n("c12_kt_cs"), M, N, K, kt, cs=True, **both),
        _spec(n("c13_kt_res_cs"), M, N, K, kt, res=True, cs=True, **both),
        _spec(n("c14_kt_act2"), M, N, K, kt, act=2, **both),
        _spec(n("c15_kt_act2_cs"), M, N, K, kt, act=2, cs=True, **both),
        _spec(n("c16_kt_act2_res_cs"), M, N, K, kt, act=2, res=True, cs=True, **both),
        _spec(n("c17_kt_act4"), M, N, K, kt, act=4, **both),
        _spec(n("c17_kt_act4_drop"), M, N, K, kt, act=4, drop=DROP_P, **both),
        _spec(n("c18_tt_beta0"), M, N, K, tt, bf16=False, f32=True),
        _spec(n("c18_tt_beta1"), M, N, K, tt, bf16=False, f32=True, beta=1.0),
        _spec(n("c18_tt_betah"), M, N, K, tt, bf16=False, f32=True, beta=0.5),
        _spec(n("c19_tt_unpadded"), M, N - 3, K, tt, bf16=False, f32=True, wide=N),    # logical N inside a wider operand of finite values
        _spec(n("c20_tt_split2"), M, N, K, tt, bf16=False, split=2),
        _spec(n("c21_kt_bias_res"), M, N, K, kt, bias=True, res=True, **both),
        _spec(n("c21_tt_bias_res"), M, N, K, tt, bias=True, res=True, **both),
    ]


S_SHAPES = ((256, 256), (200, 132), (300, 268))
S_K = 256
K_EDGES = (8, 72, 136, 200)
FEW_ROWS = (1, 5)
P_WHOLE, P_EDGE, P_GDROP = (2048, 4096, 384), (2040, 4092, 384), (2304, 3840, 384)


def _build():
    out = []
    for M, N in S_SHAPES:
        out += _classes(M, N, S_K, "S%dx%d" % (M, N))
    for K in K_EDGES:                                       # variant 1 whatever is forced: K % 64 != 0
        M, N = 200, 132
        tag = "E%dx%dk%d" % (M, N, K)
        out += [c for c in _classes(M, N, K, tag) if c["name"].split("_", 1)[1] in ("c02_bias_ld4", "c04_gelu_pre", "c10_kt_plain", "c18_tt_beta0")]
    for M in FEW_ROWS:                                      # generation's few-row forward launches: the narrow kernel
        tag = "F%dx268" % M
        out += [c for c in _classes(M, 268, S_K, tag)
                if c["name"].split("_", 1)[1] in ("c02_bias_ld4", "c03_scale20", "c04_gelu_nopre", "c07_res", "c09_gelu_res")]
    out.append(_spec("F5x136_kk_split2", 5, 136, S_K, "kk", bf16=False, split=2))
    M, N, K = P_WHOLE
    w = lambda c: "PW_" + c
    out += [
        _spec(w("bias"), M, N, K, "kk", bias=True),
        _spec(w("scale768"), M, N, K, "kk", bias=True, csn=768),
        _spec(w("scale64"), M, N, K, "kk", bias=True, csn=64),
        _spec(w("gelu_pre"), M, N, K, "kk", bias=True, act=1, preact=True),
        _spec(w("gelu_drop"), M, N, K, "kk", bias=True, act=1, preact=True, drop=DROP_P),
        _spec(w("res"), M, N, K, "kk", bias=True, res=True),
        _spec(w("drop_res"), M, N, K, "kk", bias=True, drop=DROP_P, res=True),
        _spec(w("kt_plain"), M, N, K, "kt"),
        _spec(w("kt_act2_cs"), M, N, K, "kt", act=2, cs=True),
    ]
    M, N, K = P_EDGE
    e = lambda c: "PE_" + c
    out += [
        _spec(e("res"), M, N, K, "kk", bias=True, res=True),
        _spec(e("kt_act2_cs"), M, N, K, "kt", act=2, cs=True),
        _spec(e("kt_res_cs"), M, N, K, "kt", res=True, cs=True),
        _spec(e("tanh"), M, N, K, "kk", bias=True, act=3),
        _spec(e("f32"), M, N, K, "kk", bias=True, bf16=False, f32=True),
    ]
    # (appended behind the rest: a case's seed is its index)
    # GeLU with dropout where 192 divides N too: whole tiles for 11, 12, 13 (9 x 20 tiles of 256 x 192), 6 and 9
    M, N, K = P_GDROP
    out.append(_spec("PG_gelu_drop", M, N, K, "kk", bias=True, act=1, preact=True, drop=DROP_P))
    # beta on a K-contiguous launch: the narrow kernel's fp32 store with beta != 0 (the tt classes 18 never reach it)
    for M, N in ((5, 268), (200, 132)):
        out.append(_spec("F%dx%d_kk_bias_betah" % (M, N), M, N, S_K, "kk", bias=True, bf16=False, f32=True, beta=0.5))
    return out


SPECS = _build()
INDEX = {s["name"]: i for i, s in enumerate(SPECS)}
assert len(INDEX) == len(SPECS)


def names(prefix):
    return [s["name"] for s in SPECS if s["name"].startswith(prefix)]


def gelu_grad64(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def _padded(rows, cols, ld, dtype, values):
    t = torch.full((rows, ld), NAN, dtype=dtype)
    t[:, :cols] = values.to(dtype)
    return t


@functools.lru_cache(maxsize=4)
def _case(name, K):
    s = dict(SPECS[INDEX[name]])
    g = gen(11000 + INDEX[name])
    M, N = s["M"], s["N"]
    K = s["K"] if K is None else K
    s["K"] = K
    s["a_kc"], s["b_kc"] = s["layout"] != "tt", s["layout"] == "kk"
    bf = torch.bfloat16
    Nop = s["wide"] or N                                     # the operand's finite width (class 19: wider than the logical N)
    a = 0.5 * torch.randn(M, K, generator=g)
    b = 0.5 * torch.randn(Nop, K, generator=g)
    s["A"] = a.to(bf) if s["a_kc"] else _padded(K, M, up8(M) + 8, bf, a.t())
    s["B"] = b.to(bf) if s["b_kc"] else _padded(K, Nop, up8(Nop) + 8, bf, b.t())
    ld = up8(N) + 8
    s["bias_t"] = 0.3 * torch.randn(N, generator=g) if s["bias"] else None
    s["residual"] = _padded(M, N, ld, bf, torch.randn(M, N, generator=g)) if s["res"] else None
    s["aux"] = None
    if s["act"] == 2:
        d = gelu_grad64(f64(4.0 * torch.randn(M, N, generator=g)))
        d = torch.where(d.abs() < 1e-30, torch.zeros_like(d), d)      # no subnormal products: 2^-8 relative is a normal number's rounding
        s["aux"] = _padded(M, N, ld, bf, d)
    elif s["act"] == 4:
        s["aux"] = _padded(M, N, ld, bf, torch.tanh(torch.randn(M, N, generator=g)))
    s["old"] = torch.randn(M, N, generator=g) if s["beta"] != 0.0 else None
    s["col_scale"] = COL_SCALE if s["csn"] else 1.0
    s["drop_seed"] = 1234 + INDEX[name]
    s["drop_thr"], s["drop_scale"] = drop_params(s["drop"]) if s["drop"] else (0, 1.0)
    return s


def case(name, K=None):
    """seeded operands of a case (CPU).  K: a shorter reduction for the CPU module (same seed, same classes)"""
    return dict(_case(name, K))


TENSORS = ("A", "B", "bias_t", "residual", "aux", "old")


def to_device(c, dev):
    c = dict(c)
    for k in TENSORS:
        if c[k] is not None:
            c[k] = c[k].to(dev)
    return c


def bernoulli_keep(c):
    """a stand-in mask for the CPU module (the GPU module takes the kernels' own from kmb_op_dropout_mask)"""
    return torch.rand(c["M"], c["N"], generator=gen(c["drop_seed"])) >= c["drop"]


def logical(c):
    """A [M, K] and B [N, K] as views of the storage"""
    a = c["A"] if c["a_kc"] else c["A"][:, :c["M"]].t()
    b = c["B"][:c["N"]] if c["b_kc"] else c["B"][:, :c["N"]].t()
    return a, b


def _scale_vec(c, n, like):
    sc = torch.ones(c["N"], dtype=like.dtype, device=like.device)
    sc[:max(0, min(n, c["N"]))] = c["col_scale"]
    return sc


# ------------------------------------------------------------------------------------------------ float64 reference and bounds
def exact(c, keep=None):
    """dict of float64 [M, N]: v (the value before the output's rounding and before beta) with v_slack; f32 (v + beta * old) with f32_slack;
    pre (the stored derivative) with pre_slack when the case stores one.  keep: the bool keep mask of a dropout case"""
    M, N, K = c["M"], c["N"], c["K"]
    a, b = logical(c)
    a, b = f64(a), f64(b)
    p = a @ b.t()
    s = (K + 1) * U * (a.abs() @ b.abs().t())
    if c["split"] > 1:
        return dict(v=p, v_slack=s, f32=p, f32_slack=s)
    r = {}
    pre = p + f64(c["bias_t"]) if c["bias"] else p
    sc = _scale_vec(c, c["csn"], p)
    t = pre * sc
    s = (s + 2 * U * pre.abs()) * sc + 2 * U * t.abs()
    act = c["act"]
    if act == 1:
        Phi = 0.5 * (1.0 + torch.erf(t / math.sqrt(2.0)))
        phi = torch.exp(-0.5 * t * t) / math.sqrt(2.0 * math.pi)
        dPhi = AS_PHI + 24 * U * torch.minimum(Phi, 1.0 - Phi) + 2 * U
        v = t * Phi
        if c["preact"]:
            arg = 0.5 * t * t * math.log2(math.e)
            d = Phi + t * phi
            sd = LIP2 * s + s * s + dPhi + (t * phi).abs() * (4 * U * math.log(2.0) * arg + 8 * U) + 2 * U * (Phi + (t * phi).abs())
            if c["drop"]:
                d = torch.where(keep, d * c["drop_scale"], torch.zeros_like(d))
                sd = torch.where(keep, sd * c["drop_scale"] + 2 * U * d.abs(), torch.zeros_like(d))
            r.update(pre=d, pre_slack=sd)
        s = LIP1 * s + s * s + t.abs() * dPhi + 2 * U * v.abs()
    elif act == 2:
        f = f64(c["aux"][:, :N])
        v = t * f
        s = s * f.abs() + 2 * U * v.abs()
    elif act == 3:
        v = torch.tanh(t)
        s = LIP_TANH * s + TANH_ULP * 2 * U * v.abs()
    elif act == 4:
        f = 1.0 - f64(c["aux"][:, :N]) ** 2
        v = t * f
        s = s * f.abs() + 4 * U * t.abs() + 2 * U * v.abs()
    else:
        v = t
    if c["drop"]:
        v = torch.where(keep, v * c["drop_scale"], torch.zeros_like(v))
        s = torch.where(keep, s * c["drop_scale"] + 2 * U * v.abs(), torch.zeros_like(v))
    if c["res"]:
        v = v + f64(c["residual"][:, :N])
        s = s + 2 * U * v.abs()
    r.update(v=v, v_slack=s, f32=v, f32_slack=s)
    if c["beta"] != 0.0:
        bo = c["beta"] * f64(c["old"])
        o = v + bo
        r.update(f32=o, f32_slack=s + 2 * U * bo.abs() + 2 * U * o.abs())
    return r


def colsum_bands(ex, M):
    """(reference, bound), each [ceil(M / 256), N] float64: the column sums of rows 256 t .. 256 t + 255 of v"""
    refs, bounds = [], []
    for r0 in range(0, M, BAND):
        v, s = ex["v"][r0:r0 + BAND], ex["v_slack"][r0:r0 + BAND]
        refs.append(v.sum(0))
        bounds.append(sum_bound(v.shape[0], v.abs().sum(0)) + s.sum(0))
    return torch.stack(refs), torch.stack(bounds)


def fold_bands(partial, M):
    """partial rows [ceil(M / 64), N] (one per 64 rows of C) -> [ceil(M / 256), N] float64, four at a time"""
    p = f64(partial[:(M + 63) // 64])
    return torch.stack([p[4 * t:4 * t + 4].sum(0) for t in range((M + BAND - 1) // BAND)])


# ------------------------------------------------------------------------------------------------ fp32 emulation
def gelu_parts_emu(x, c3=1.421413741):
    """(cdf, e) in fp32: common.h gelu_parts with exact division and exp2"""
    z = x.abs() * 0.70710678118654752
    t = 1.0 / (z * 0.3275911 + 1.0)
    e = torch.exp2(z * z * -1.4426950408889634)
    poly = t * 1.061405429 + -1.453152027
    poly = poly * t + c3
    poly = poly * t + -0.284496736
    poly = poly * t + 0.254829592
    h = 0.5 * poly * t * e
    return torch.where(x >= 0, 1.0 - h, h), e


def emulate(c, keep=None, mut=None):
    """dict of fp32: v32 (before the output's rounding and beta), f32, pre32, colsum (partial rows, one per 64 rows, each summed
    sequentially).  mut: one of MUTATIONS"""
    assert mut is None or mut in MUTATIONS
    f = torch.float32
    M, N, K = c["M"], c["N"], c["K"]
    a, b = logical(c)
    a, b = a.to(f), b.to(f)
    if mut == "skip_kstep":
        assert K >= 128
        ks = [k for k in range(K) if not 64 <= k < 128]
        a, b = a[:, ks], b[:, ks]
    acc = seq_sum(a.t()[:, :, None] * b.t()[:, None, :], 0)          # the products of bf16 values are exact in fp32
    if c["split"] > 1:
        return dict(v32=acc, f32=acc)
    r = {}
    bias = c["bias_t"] if c["bias"] else torch.zeros(N)
    if mut == "bias_shift_last8":
        g0 = ((N - 1) // 8) * 8
        bias = bias.clone()
        bias[g0:N - 1] = c["bias_t"][g0 + 1:N]
    sc = _scale_vec(c, c["csn"] + (1 if mut == "scale_n_plus1" else -1 if mut == "scale_n_minus1" else 0), acc)
    t = acc * sc + bias if mut == "bias_after_scale" else (acc + bias) * sc
    ds = torch.tensor(c["drop_scale"], dtype=f)
    act = c["act"]
    if act == 1:
        cdf, e = gelu_parts_emu(t, 1.4213 if mut == "poly_const" else 1.421413741)
        v = t * cdf
        if c["preact"]:
            d = cdf if mut == "no_tphi" else cdf + t * 0.39894228040143268 * e
            if c["drop"]:
                d = torch.where(keep, d * ds, torch.zeros_like(d))
            r["pre32"] = d
    elif act == 2:
        v = t * c["aux"][:, :N].to(f)
    elif act == 3:
        v = torch.tanh(t)
    elif act == 4:
        u = c["aux"][:, :N].to(f)
        v = t * (1.0 - u) if mut == "act4_linear" else t * (1.0 - u * u)
    else:
        v = t
    res = None
    if c["res"]:
        res = c["residual"][:, :N].to(f)
        if mut == "res_row_plus1":
            res = torch.roll(res, -1, 0)
    if mut == "drop_after_res":
        v = torch.where(keep, (v + res) * ds, torch.zeros_like(v))
    else:
        if c["drop"]:
            v = torch.where(keep, v * ds, torch.zeros_like(v))
        if res is not None:
            v = v + res
    if mut == "pad_nan":                                             # a pad column's NaN in the place of the last element's operand
        v = v.clone()
        pad = c["residual"][M - 1, N] if c["res"] else c["A"][0, M] if not c["a_kc"] else c["B"][0, N] if not c["b_kc"] else torch.tensor(NAN)
        v[M - 1, N - 1] = v[M - 1, N - 1] + pad.to(f) * 0.0
    r["v32"] = v
    r["f32"] = v if c["beta"] == 0.0 or mut == "beta_ignored" else v + torch.tensor(c["beta"], dtype=f) * c["old"]
    if c["cs"]:
        rows = []
        for r0 in range(0, M, 64):
            blk = v[r0:min(M, r0 + 64)]
            if mut == "colsum_skip_row":
                blk = blk[:-1]
            rows.append(seq_sum(blk, 0))
        r["colsum"] = torch.stack(rows)
    return r
