"""float64 references, derived bounds, fp32 emulations and seeded cases of the row kernels between the GEMMs: csrc/norm.hip (LayerNorm
forward / backward, the slab reducers, colsum), csrc/embed.hip and csrc/embed_row.h.  A helper module of test_row_kernels_cpu.py and
test_row_kernels_gpu.py.  Everything here is CPU torch: the GPU module moves a case's inputs to the device, runs the kernel through the
C-ABI and brings the outputs back, so both modules judge with the same code.

Three kinds of code:

* REFERENCES: the operation in float64 on the values the kernel was given (bf16 / fp32 inputs widened exactly).  LayerNorm backward takes
  the fp32 `mean` and `rstd` it is handed: they are inputs of that op.  The embedding's LayerNorm takes its statistics from the UNROUNDED row
  E * scale + P (embed_row.h keeps the fp32 row in registers), although the z it stores -- which LayerNorm backward later normalises with
  those statistics -- is that row rounded to bf16: embed_fwd_case() below does the same, on purpose.
* BOUNDS, derived (u = 2^-24 is fp32's unit roundoff, x^ the float64 normalised value, g = dy * gamma):
    mean                      D u mean_i |z_i|                     (any summation order of D terms)
    rstd                      relative (D + 8) u                   (the squares are non-negative; the mean's error enters at second order)
    a bf16 output, value r    2^-8 |r| + 1.01 slack                (2^-8: one round-to-nearest; the slack bounds |fp32 value - r|; 1.01 >= 1 + 2^-8
                                                                    because the rounding's relative error applies to the fp32 value, not to r)
    slack of y                2^-15 (|x^ gamma| + |beta|)
    slack of dz               (D + 16) u rstd (|g_i| + mean|g| + |x^_i| mean|g x^|)
    slack of the embedding z  2^-22 (|E scale| + |P|)
    a sum of n fp32 terms     (n + 4) u sum_k |t_k|                (dbeta, colsum, pos_bwd, a dE row with n = the id's count)
    dgamma                    (n + 8) u sum_k |t_k|                (WIDENED by its constant: a term dy x^ carries x^'s two roundings and its own, so a
                                                                    one-row launch reaches 2.5 u of the rule's 5 u -- the emulation measured 0.5005)
    dsub                      the sum bound + the column's summed slack of the terms
  A value that is one more fp32 multiply away from a bounded one (out2 = dz * dropout scale, the embedding's y * dropout scale, dimg =
  dz * scale) adds 2 u |r| to its slack: one rounding reaches u just above a power of two, and the slack is to keep a factor 2; the kept
  values of reduce_slabs_epi under dropout, two roundings (or one fused) behind exactly known fp32 operands, take 4 u (|w scale| + |residual|).
  y's slack has no term for the mean's error, which is absolute (rstd |gamma| |mean error|, some 3e-7 at these inputs): the cases keep
  |beta| >= 0.05 so that the slack never falls below 2^-15 * 0.05 = 1.5e-6 (the emulation's worst fp32 part of y is 0.07 of its slack).
* EMULATIONS: the same operation in torch fp32 with STRICTLY SEQUENTIAL sums (the unfavourable order: the kernels add lane partials pairwise),
  returning the fp32 values before any bf16 rounding.  test_row_kernels_cpu.py measures emulation against reference in units of each bound:
  the fp32 part of every bound must keep a factor 2 (ratio <= 0.5).
"""
import functools
import math

import torch

U = 2.0 ** -24
BF16_ROUND = 2.0 ** -8
EPS = float(torch.tensor(1e-5, dtype=torch.float32))      # the eps the kernels receive (a float argument)
NAN = float("nan")


def f64(x):
    return x.to(torch.float64)


def gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def away_from_zero(x, floor):
    return torch.where(x >= 0, x + floor, x - floor)


def drop_params(p):
    """(thr16, fp32 scale as a Python float) of a dropout probability, as KmbDrop carries them"""
    thr = int(round(p * 65536))
    return thr, float(torch.tensor(1.0 / (1.0 - thr / 65536.0), dtype=torch.float32))


def seq_sum(t, dim):
    """strictly sequential fp32 (or whatever dtype t has) sum along dim: ((t0 + t1) + t2) + ..."""
    t = t.movedim(dim, 0)
    acc = t[0].clone()
    for k in range(1, t.shape[0]):
        acc = acc + t[k]
    return acc


# ------------------------------------------------------------------------------------------------ the one judging helper
def worst(got, ref, bound):
    """(worst err / bound over all elements, its flat index); an element with bound 0 passes only when it is exact"""
    err = (f64(got) - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)      # a NaN sentinel left in an output
    i = int(torch.argmax(ratio.reshape(-1)))
    return float(ratio.reshape(-1)[i]), i


def assert_elementwise(got, ref, bound, what, limit=1.0):
    """|got - ref| <= limit * bound for EVERY element; reports the worst element and its err / bound.  Returns that ratio."""
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(ref)
    r, i = worst(got, ref, bound)
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ref.shape)) if ref.dim() else ()
    print("%-58s worst err / bound %.4f at %s" % (what, r, idx))
    assert r <= limit, "%s: element %s got %.9g want %.9g bound %.3g: err / bound = %.4g (limit %.3g)" % (
        what, idx, float(f64(got).reshape(-1)[i]), float(ref.reshape(-1)[i]), float(bound.reshape(-1)[i]), r, limit)
    return r


def bf16_bound(ref, slack):
    return BF16_ROUND * ref.abs() + 1.01 * slack


def sum_bound(n, abs_sum):
    return (n + 4) * U * abs_sum


def same_bits(a, b):
    if a.dtype == torch.bfloat16:
        return torch.equal(a.view(torch.int16), b.view(torch.int16))
    if a.dtype == torch.float32:
        return torch.equal(a.view(torch.int32), b.view(torch.int32))
    return torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ LayerNorm forward
def ln_fwd_ref(x, gamma, beta, eps=EPS):
    """x [M, D] float64 (or anything widened exactly).  dict of float64: mean, rstd, xh, y and the bounds of mean, rstd (absolute), y's slack"""
    x = f64(x)
    D = x.shape[1]
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    rstd = (var + eps) ** -0.5
    xh = (x - mean[:, None]) * rstd[:, None]
    y = xh * f64(gamma) + f64(beta)
    return dict(mean=mean, rstd=rstd, xh=xh, y=y, mean_bound=D * U * x.abs().mean(1), rstd_bound=(D + 8) * U * rstd,
                y_slack=2.0 ** -15 * ((xh * f64(gamma)).abs() + f64(beta).abs()))


def ln_fwd_emu(x, gamma, beta, eps=EPS):
    """fp32, sequential sums, the kernel's operations: mu = s / D; q = sum (v - mu)^2; rs = rsqrt(q / D + eps); y = (v - mu) rs gamma + beta"""
    x = x.to(torch.float32)
    D = x.shape[1]
    mu = seq_sum(x, 1) / D
    d = x - mu[:, None]
    rs = torch.rsqrt(seq_sum(d * d, 1) / D + eps)
    return dict(mean=mu, rstd=rs, y32=d * rs[:, None] * gamma + beta)


CONST_ROW = 1.5


def ramp_row(D):
    """64 + k / 2, k = column mod 128: bf16-exact, every fp32 partial sum exact, mean near 96 against a deviation near 18"""
    return 64.0 + (torch.arange(D) % 128).to(torch.float32) / 2.0


def ln_params(D, g):
    gamma = 1.0 + 0.1 * torch.randn(D, generator=g)
    beta = away_from_zero(0.1 * torch.randn(D, generator=g), 0.05)
    return gamma, beta


@functools.lru_cache(maxsize=None)
def ln_fwd_case(M, D, kind="mixed"):
    """z bf16 [M, D], gamma, beta fp32.  kind "mixed" (M >= 3): row 1 is the constant row, row M - 1 the large-mean row (the last block's
    last row); a one-row launch cannot carry them, so M = 1 runs once per kind "random" / "const" / "ramp\""""
    g = gen(1000 + 7 * M + D)
    z = (torch.randn(M, D, generator=g) * 2.0 + 0.3).to(torch.bfloat16)
    gamma, beta = ln_params(D, g)
    edges = {}
    if kind == "mixed":
        assert M >= 3
        edges = {"const": 1, "ramp": M - 1}
    elif kind != "random":
        edges = {kind: 0}
    for k, r in edges.items():
        z[r] = CONST_ROW if k == "const" else ramp_row(D).to(torch.bfloat16)
    ref = ln_fwd_ref(z, gamma, beta)
    return dict(M=M, D=D, z=z, gamma=gamma, beta=beta, edges=edges, ref=ref)


def check_ln_fwd(case_ref, mean, rstd, y, what):
    """mean, rstd (fp32, may be None), y (bf16) against a forward reference; returns the ratios"""
    out = {}
    if mean is not None:
        out["mean"] = assert_elementwise(mean, case_ref["mean"], case_ref["mean_bound"], what + " mean")
        out["rstd"] = assert_elementwise(rstd, case_ref["rstd"], case_ref["rstd_bound"], what + " rstd")
    out["y"] = assert_elementwise(y, case_ref["y"], bf16_bound(case_ref["y"], case_ref["y_slack"]), what + " y")
    return out


# ------------------------------------------------------------------------------------------------ LayerNorm backward
MASK_FORMS = ("none", "dy_drop", "out2", "out2_drop", "both")
DROP_P = 0.1
SEED_DY, SEED_OUT2 = 77, 99


def ln_bwd_ref(dy, z, mean, rstd, gamma, keep1=None, scale1=1.0, with_out2=False, keep2=None, scale2=1.0):
    """float64 LayerNorm backward from the fp32 statistics handed to the kernel.  keep1 / keep2: bool masks [M, D] or None"""
    M, D = z.shape
    d = f64(dy)
    if keep1 is not None:
        d = torch.where(keep1, d * scale1, torch.zeros_like(d))
    rs = f64(rstd)[:, None]
    xh = (f64(z) - f64(mean)[:, None]) * rs
    g = d * f64(gamma)
    c1, c2 = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
    dz = (g - c1 - xh * c2) * rs
    dz_slack = (D + 16) * U * rs * (g.abs() + g.abs().mean(1, keepdim=True) + xh.abs() * (g * xh).abs().mean(1, keepdim=True))
    r = dict(dz=dz, dz_slack=dz_slack, dgamma=(d * xh).sum(0), dgamma_bound=sum_bound(M + 4, (d * xh).abs().sum(0)),
             dbeta=d.sum(0), dbeta_bound=sum_bound(M, d.abs().sum(0)))
    sub, sub_slack = dz, dz_slack          # what the kernel's third partial sums: out2's fp32 values when out2 is given, dz's otherwise
    if with_out2:
        if keep2 is not None:
            sub = torch.where(keep2, dz * scale2, torch.zeros_like(dz))
            sub_slack = torch.where(keep2, dz_slack * scale2 + 2 * U * sub.abs(), torch.zeros_like(dz))
        r.update(out2=sub, out2_slack=sub_slack)
    r.update(dsub=sub.sum(0), dsub_bound=sum_bound(M, sub.abs().sum(0)) + sub_slack.sum(0))
    return r


def ln_bwd_emu(dy, z, mean, rstd, gamma, keep1=None, scale1=1.0, with_out2=False, keep2=None, scale2=1.0):
    """fp32, the kernel's operations (csrc/norm.hip ln_bwd_kernel), sequential row and column sums; values before the bf16 rounding"""
    f = torch.float32
    D = z.shape[1]
    d = dy.to(f)
    if keep1 is not None:
        d = torch.where(keep1, d * torch.tensor(scale1, dtype=f), torch.zeros_like(d))
    rs = rstd.to(f)[:, None]
    xh = (z.to(f) - mean.to(f)[:, None]) * rs
    g = d * gamma.to(f)
    inv_d = torch.tensor(1.0 / D, dtype=f)
    c1, c2 = seq_sum(g, 1)[:, None] * inv_d, seq_sum(g * xh, 1)[:, None] * inv_d
    dz = ((g - c1) - xh * c2) * rs
    r = dict(dz32=dz, dgamma=seq_sum(d * xh, 0), dbeta=seq_sum(d, 0))
    sub = dz
    if with_out2:
        if keep2 is not None:
            sub = torch.where(keep2, dz * torch.tensor(scale2, dtype=f), torch.zeros_like(dz))
        r["out2_32"] = sub
    r["dsub"] = seq_sum(sub, 0)
    return r


LN_BWD_SHAPES = [(M, D) for D in (8, 72, 256, 264, 768, 1024, 1032, 2048) for M in (1, 5, 13)] + [(1030, 72), (4101, 72)]
LN_BWD_MASK_SHAPES = [(13, 72), (13, 768), (1030, 72), (4101, 72)]
LN_BWD_CASES = [(M, D, "none") for M, D in LN_BWD_SHAPES] + [(M, D, f) for M, D in LN_BWD_MASK_SHAPES for f in MASK_FORMS[1:]]


@functools.lru_cache(maxsize=None)
def ln_bwd_inputs(M, D):
    g = gen(2000 + 3 * M + D)
    z = (torch.randn(M, D, generator=g) * 2.0 + 0.3).to(torch.bfloat16)
    dy = torch.randn(M, D, generator=g).to(torch.bfloat16)
    gamma = 1.0 + 0.1 * torch.randn(D, generator=g)
    st = ln_fwd_ref(z, gamma, torch.zeros(D))
    return dict(M=M, D=D, z=z, dy=dy, gamma=gamma, mean=st["mean"].to(torch.float32), rstd=st["rstd"].to(torch.float32))


def form_flags(form):
    """(dy_drop, out2, out2_drop) of a mask form"""
    return form in ("dy_drop", "both"), form in ("out2", "out2_drop", "both"), form in ("out2_drop", "both")


def bernoulli_keep(M, D, seed):
    """a stand-in mask for the CPU module (the GPU module takes the kernels' own mask from kmb_op_dropout_mask)"""
    return torch.rand(M, D, generator=gen(seed)) >= DROP_P


# ------------------------------------------------------------------------------------------------ slabs
def slab_sum(slabs):
    """fp32 sum of slabs [nslabs, ...] in slice order: the one result the kernels' additions admit"""
    return seq_sum(slabs.to(torch.float32), 0)


@functools.lru_cache(maxsize=None)
def ln_slabs_case(D, nslabs, with_bias, R=5):
    """slabs [nslabs][stride] fp32 with stride = R D + 8 (the pad holds NaN), residual bf16 with ld_res = D + 8 (pad NaN).  The
    pre-LayerNorm row is exact: ((slab 0 + slab 1 + ...) + bias) + residual in fp32, then bf16"""
    g = gen(3000 + 11 * D + nslabs + (100 if with_bias else 0))
    stride = R * D + 8
    slabs = torch.full((nslabs, stride), NAN)
    slabs[:, :R * D] = torch.randn(nslabs, R * D, generator=g)
    bias = torch.randn(D, generator=g) * 0.3 if with_bias else None
    res = torch.full((R, D + 8), NAN, dtype=torch.bfloat16)
    res[:, :D] = torch.randn(R, D, generator=g).to(torch.bfloat16)
    gamma, beta = ln_params(D, g)
    t = slab_sum(slabs[:, :R * D]).view(R, D)
    if with_bias:
        t = t + bias
    pre = (t + res[:, :D].to(torch.float32)).to(torch.bfloat16)
    return dict(D=D, R=R, nslabs=nslabs, stride=stride, slabs=slabs, bias=bias, res=res, gamma=gamma, beta=beta, pre=pre,
                ref=ln_fwd_ref(pre, gamma, beta))


@functools.lru_cache(maxsize=None)
def reduce_case(nslabs, n, pad, seed=0):
    g = gen(4000 + nslabs + seed)
    slabs = torch.full((nslabs, n + pad), NAN)
    slabs[:, :n] = torch.randn(nslabs, n, generator=g)
    start = torch.randn(n, generator=g)
    return dict(nslabs=nslabs, n=n, stride=n + pad, slabs=slabs, start=start, total=slab_sum(slabs[:, :n]))


def reduce_expect(case, beta):
    """a = the slabs in slice order; beta != 0: a += beta * out (beta a power of two: the product is exact)"""
    a = case["total"]
    return a if beta == 0.0 else a + torch.tensor(beta, dtype=torch.float32) * case["start"]


EPI_SCALE = 0.125


@functools.lru_cache(maxsize=None)
def epi_case(M, N, nslabs):
    g = gen(5000 + M + N + nslabs)
    stride = M * N + 4
    slabs = torch.full((nslabs, stride), NAN)
    slabs[:, :M * N] = torch.randn(nslabs, M * N, generator=g)
    bias = torch.randn(N, generator=g) * 0.3
    res = torch.full((M, N + 8), NAN, dtype=torch.bfloat16)
    res[:, :N] = torch.randn(M, N, generator=g).to(torch.bfloat16)
    return dict(M=M, N=N, nslabs=nslabs, stride=stride, slabs=slabs, bias=bias, res=res, total=slab_sum(slabs[:, :M * N]).view(M, N))


def epi_pre_drop(case, with_bias, col_scale_n):
    """fp32 (sum + bias) * scale, exact bits: 0.125 is a power of two"""
    w = case["total"]
    if with_bias:
        w = w + case["bias"]
    sc = torch.ones(case["N"])
    sc[:col_scale_n] = EPI_SCALE
    return w * sc


# ------------------------------------------------------------------------------------------------ colsum, pos_bwd
COLSUM_CASES = [(37, 76, 80), (70, 8, 8), (33, 64, 72), (2100, 72, 72)]


@functools.lru_cache(maxsize=None)
def colsum_case(M, N, ld):
    X = torch.full((M, ld), NAN, dtype=torch.bfloat16)
    X[:, :N] = torch.randn(M, N, generator=gen(6000 + M + N)).to(torch.bfloat16)
    x = f64(X[:, :N])
    return dict(X=X, ref=x.sum(0), bound=sum_bound(M, x.abs().sum(0)))


POS_CASES = [(13, 7, 768), (5, 3, 2048), (70, 2, 8)]
POS_BASE, POS_EXTRA = 2, 3


@functools.lru_cache(maxsize=None)
def pos_case(B, S, D):
    dz = torch.randn(B * S, D, generator=gen(7000 + B + S + D)).to(torch.bfloat16)
    x = f64(dz).view(B, S, D)
    return dict(dz=dz, rows=POS_BASE + S + POS_EXTRA, ref=x.sum(0), bound=sum_bound(B, x.abs().sum(0)))


# ------------------------------------------------------------------------------------------------ embedding
EMB_B, EMB_S, EMB_V, EMB_NIMG = 2, 5, 40, 3


@functools.lru_cache(maxsize=None)
def embed_fwd_case(D, scaled):
    """B * S = 2 * 5 rows at pos_base = 2: token rows (one id twice) and three region rows (img_src >= 0 takes row img_src of img_emb)"""
    g = gen(8000 + D + (1 if scaled else 0))
    M = EMB_B * EMB_S
    ids = torch.randint(0, EMB_V, (M,), generator=g)
    ids[7] = ids[0]
    img_src = torch.full((M,), -1, dtype=torch.int32)
    img_src[1], img_src[2], img_src[8] = 0, 2, 1
    E = torch.randn(EMB_V, D, generator=g) * 0.05
    img = torch.randn(EMB_NIMG, D, generator=g) * 0.05
    P = torch.randn(POS_BASE + EMB_S, D, generator=g) * 0.05
    gamma, beta = ln_params(D, g)
    scale = float(torch.tensor(math.sqrt(D), dtype=torch.float32)) if scaled else 1.0
    rows = E[ids].clone()
    sel = img_src >= 0
    rows[sel] = img[img_src[sel].long()]
    prow = P[POS_BASE + torch.arange(M) % EMB_S]
    v = f64(rows) * scale + f64(prow)                                  # the unrounded row: the statistics' source (module docstring)
    ref = ln_fwd_ref(v, gamma, beta)
    ref.update(z=v, z_slack=2.0 ** -22 * ((f64(rows) * scale).abs() + f64(prow).abs()))
    return dict(M=M, D=D, ids=ids, img_src=img_src, E=E, img=img, P=P, gamma=gamma, beta=beta, scale=scale, rows=rows, prow=prow, ref=ref)


def embed_fwd_emu(case):
    """fp32: v = e * scale + p (two roundings), statistics and y from v"""
    v = case["rows"] * torch.tensor(case["scale"], dtype=torch.float32) + case["prow"]
    r = ln_fwd_emu(v, case["gamma"], case["beta"])
    r["z32"] = v
    return r


EMBB_M, EMBB_V, EMBB_NIMG, EMBB_PAD, EMBB_HOT = 4 * 37, 50, 9, 1, 5


@functools.lru_cache(maxsize=None)
def embed_bwd_case(D, scaled):
    """M = 4 * 37 rows over V = 50 ids: id 5 occurs 40 times, pad rows (no gradient), six region rows into a dimg of nine rows (three never
    referred to), ids 44 .. 49 never drawn; dE and dimg start from random values"""
    g = gen(9000 + D + (1 if scaled else 0))
    M = EMBB_M
    ids = torch.randint(2, 44, (M,), generator=g)
    ids[ids == EMBB_HOT] = 6
    img_src = torch.full((M,), -1, dtype=torch.int32)
    for k, r in enumerate((0, 9, 60, 61, 100, 146)):
        img_src[r] = (0, 2, 3, 5, 6, 8)[k]
    pads = [3, 50, 147]
    free = torch.tensor([r for r in range(M) if int(img_src[r]) < 0 and r not in pads])
    ids[free[torch.randperm(len(free), generator=g)[:40]]] = EMBB_HOT
    ids[pads] = EMBB_PAD
    dz = torch.randn(M, D, generator=g).to(torch.bfloat16)
    dE0 = torch.randn(EMBB_V, D, generator=g)
    dimg0 = torch.randn(EMBB_NIMG, D, generator=g).to(torch.bfloat16)
    scale = float(torch.tensor(math.sqrt(D), dtype=torch.float32)) if scaled else 1.0
    tok = (img_src < 0) & (ids != EMBB_PAD)
    t = f64(dz) * scale
    ref = f64(dE0).clone()
    ref.index_add_(0, ids[tok], t[tok])
    mag = f64(dE0).abs()
    mag.index_add_(0, ids[tok], t[tok].abs())
    count = torch.bincount(ids[tok], minlength=EMBB_V)
    touched = count > 0
    sel = img_src >= 0
    return dict(M=M, D=D, ids=ids, img_src=img_src, dz=dz, dE0=dE0, dimg0=dimg0, scale=scale, tok=tok, sel=sel, touched=touched, count=count,
                dE=ref, dE_bound=sum_bound(count[:, None], mag),       # n = the id's count; the terms: the start value and the products
                dimg=t[sel], dimg_rows=img_src[sel].long())


def embed_bwd_emu(case):
    """fp32 products added to the start value in row order"""
    f = torch.float32
    dE = case["dE0"].clone()
    t = case["dz"].to(f) * torch.tensor(case["scale"], dtype=f)
    for r in torch.nonzero(case["tok"]).flatten().tolist():
        dE[case["ids"][r]] += t[r]
    return dE
