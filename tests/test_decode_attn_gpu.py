"""GPU: the three attention kernels of a decode step, pinned to float64 per (row, head):

  * decode_attn_kernel<SELF>   (csrc/decode.hip, KmbDecodeBlock kind 1) with a non-identity history index;
  * decode_attn_kernel<cross>  (kind 2), the vector form and the KVLDS matrix-core form -- each case asserts, through
    kmb_debug_decode_route, that it ran the kernel its id names;
  * attn_decode_kernel         (csrc/attention.hip), with and without new_k / new_v / Kw / Vw, with and without hist.

References come from tests/decode_attn_ref.py and are built from the INPUTS only (bf16 activations / caches, fp32 parameters).

Bounds.  `out`, per (row, head), norm-wise against exact float64: 2 x the worst error of the ROUNDING MODEL (the same computation with the
kernel's bf16 storage roundings and nothing else) over that family's cases; `python tests/test_decode_attn_gpu.py` measures the model on the
CPU from the same seeds, tests/test_decode_attn_cpu.py keeps the recorded constants from drifting.  The factor 2 covers fp32 accumulation
order and __expf.  A fully masked item is zeros and must be matched exactly.
ln_out and the appended k / v rows, elementwise: |got - bf16(ref)| <= ulp_bf16(ref) + K 2^-24 sum_i |term_i| -- one rounding flip plus the
fp32 accumulation allowance (LayerNorm: terms n gamma and beta; k / v: the 768 products x_i w_i and the bias, ref = the float64 projection of
the bf16-rounded float64 LayerNorm, which is what the projection is specified to consume).  The k / v allowance also carries a flip of the
LayerNorm's own storage rounding into the projection: ulp_bf16(x_i) |w_i| for the elements whose float64 LayerNorm lies within the
LayerNorm's fp32 allowance of a bf16 rounding boundary, zero for every other element (2.8 % of them are near one).  Measured on an MI355X
without that term: 20 of the 6.9 M appended elements of the self cases exceed the allowance, by up to 1.43 x, each in a row whose stored
LayerNorm has such a flipped element; with it the worst is 0.92.
History / cache bookkeeping and the isolation checks are bitwise.
"""
import ctypes as C
import os
import sys

import pytest
import torch

if __name__ == "__main__":   # the CPU measurement of the rounding model: no pytest, no conftest
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(_root, "km-bart_amd"), os.path.join(_root, "tests")]

pytestmark = pytest.mark.gpu

import decode_attn_ref as REF  # noqa: E402
from kmbart import _lib  # noqa: E402
from kmbart._lib import DECODE_ROUTES, KmbAttnDecode, KmbDecodeBlock, check, ptr  # noqa: E402

DEV = "cuda:0"
HD, D = 64, 768
EPS = 1e-5
Q_SCALE = 0.125
U24 = 2.0 ** -24

# ---- rounding-model measurements (`python tests/test_decode_attn_gpu.py`, CPU, the seeds below): worst per-(row, head) norm-wise error of
# the model against exact float64 over all cases of the family; the bounds are MARGIN x these.
# GPU-measured worst error / bound on an MI355X: 0.500 in all four families -- the worst (row, head) is one whose error IS the storage
# rounding (the kernels round the same values at the same places as the model), so the kernels sit at the model's error, half the bound.
# Elementwise on the same run: ln_out 0.994 of its allowance (one ulp), appended k / v rows 0.916.
MODEL_HEAD_ERR = {"self": 1.85e-02, "cross_vec": 9.63e-03, "cross_kvlds": 9.63e-03, "attn_decode": 2.31e-03}
MARGIN = 2.0
HEAD_BOUND = {k: MARGIN * v for k, v in MODEL_HEAD_ERR.items()}
GPU_WORST_RATIO = {}

# ------------------------------------------------------------------------------------------------ cases
SELF_TKS = (1, 2, 10, 11, 12, 20, 21, 22, 64)   # both edges of the VU = 10 value and 4 * KU = 20 key prefetch windows
SELF_CASES = [dict(R=R, Tk=Tk, H=12) for R in (37, 320) for Tk in SELF_TKS]
SELF_CASES += [dict(R=1290, Tk=19, H=12),        # more row tiles than one round of workgroups
               dict(R=37, Tk=12, H=3)]           # N = 576


def self_id(c):
    return "R%d-Tk%d-H%d" % (c["R"], c["Tk"], c["H"])


CROSS_SHAPES = [(3, 4, 37), (64, 5, 100), (7, 5, 104), (7, 5, 105), (7, 6, 120), (2, 5, 130), (5, 3, 50), (3, 7, 40), (2, 16, 33), (2, 17, 33)]


def cross_route(nb, S, grouped):
    """the kernel the case is meant to run: KVLDS needs >= 4 beams per item and fits 104 keys at K = 768"""
    return "attn_cross_kvlds" if grouped and nb >= 4 and S <= 104 else "attn_cross"


CROSS_CASES = [dict(B=B, nb=nb, S=S, grouped=g, H=12, layers=1, layer=0) for (B, nb, S) in CROSS_SHAPES for g in (True, False)]
CROSS_CASES += [dict(B=3, nb=4, S=37, grouped=g, H=12, layers=6, layer=4) for g in (True, False)]     # ldc = 6 * 2 * d, layer offset
CROSS_CASES += [dict(B=3, nb=5, S=41, grouped=g, H=3, layers=1, layer=0) for g in (True, False)]      # N = 192


def cross_id(c):
    return "B%d-nb%d-S%d-H%d-L%d-%s-%s" % (c["B"], c["nb"], c["S"], c["H"], c["layers"], "grouped" if c["grouped"] else "ungrouped",
                                           cross_route(c["nb"], c["S"], c["grouped"]))


AD_SHAPES = [(6, 2, 37), (5, 3, 1), (7, 3, 65), (9, 12, 130)]      # R * H % 4 != 0, Tk == 1, Tk > 64
AD_CASES = [dict(R=R, H=H, Tk=Tk, style="self", new=new, hist=hist) for (R, H, Tk) in AD_SHAPES for new in (False, True) for hist in (False, True)]
AD_CASES += [dict(R=R, H=H, Tk=Tk, style="cross", new=False, hist=False) for (R, H, Tk) in AD_SHAPES]
AD_CASES += [dict(R=7, H=3, Tk=65, style="cross_maskrow", new=False, hist=False)]                    # mask_row != kv_row


def ad_id(c):
    return "R%d-H%d-Tk%d-%s-new%d-hist%d" % (c["R"], c["H"], c["Tk"], c["style"], c["new"], c["hist"])


# ------------------------------------------------------------------------------------------------ inputs (CPU generator: the same on every machine)
def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _bf(x):
    return x.to(torch.bfloat16).contiguous()


def _proj_inputs(g, R, N, dev):
    z = _bf(torch.randn(R, D, generator=g) * 1.3 + 0.2)
    gamma = torch.rand(D, generator=g) + 0.5
    beta = torch.randn(D, generator=g) * 0.1
    W = _bf(torch.randn(N, D, generator=g) * 0.05)
    bias = torch.randn(N, generator=g) * 0.1
    return dict(z=z.to(dev), gamma=gamma.to(dev), beta=beta.to(dev), W=W.to(dev), bias=bias.to(dev))


def _poison(rows, T, d, t0):
    """large finite values, different per (row, position): a stray read shows as a wrong number"""
    r = torch.arange(rows, dtype=torch.float32)[:, None, None]
    t = (torch.arange(T, dtype=torch.float32) + t0)[None, :, None]
    c = torch.arange(d, dtype=torch.float32)[None, None, :]
    sign = 1.0 - 2.0 * ((r + t) % 2)
    return _bf((600.0 + 4.0 * ((r * 31 + t * 17) % 97)) * sign * (1.0 - 2.0 * (c % 2)) + 8.0 * (c % 5))


def _history(g, R, Tk, Tmax):
    """hist[r][t < Tk-1]: random rows, drawn per (r, t); hist[r][t >= Tk-1]: a valid but wrong row"""
    hist = ((torch.arange(R)[:, None] + 7) % R).expand(R, Tmax).contiguous().to(torch.int32)
    if Tk > 1:
        hist[:, :Tk - 1] = torch.randint(0, R, (R, Tk - 1), generator=g).to(torch.int32)
    return hist


def _self_cache(g, R, Tk, Tmax, d):
    def one():
        c = _poison(R, Tmax, d, 0)
        if Tk > 1:
            c[:, :Tk - 1] = _bf(torch.randn(R, Tk - 1, d, generator=g))
        return c
    return one(), one()


def self_inputs(c, dev):
    R, Tk, H = c["R"], c["Tk"], c["H"]
    d = H * HD
    Tmax = 24 if Tk <= 24 else 70
    g = _gen(1000 + R * 131 + Tk * 7 + H)
    p = _proj_inputs(g, R, 3 * d, dev)
    Kc, Vc = _self_cache(g, R, Tk, Tmax, d)
    p.update(Kc=Kc.to(dev), Vc=Vc.to(dev), hist=_history(g, R, Tk, Tmax).to(dev), R=R, Tk=Tk, H=H, Tmax=Tmax)
    return p


def key_mask_for(B, S):
    """ragged right padding, holes (key 0 among them) in every second item, and the LAST item without any key"""
    m = torch.ones(B, S, dtype=torch.int64)
    for b in range(B):
        m[b, S - (3 * b + 1) % (S // 2 + 1):] = 0
        if b % 2 == 0:
            m[b, 0] = 0
            m[b, S // 3] = 0
    m[B - 1] = 0
    return m


def cross_inputs(c, dev):
    B, nb, S, H, L, layer = c["B"], c["nb"], c["S"], c["H"], c["layers"], c["layer"]
    d, R = H * HD, B * nb
    g = _gen(2000 + B * 977 + nb * 53 + S * 3 + H + L)
    p = _proj_inputs(g, R, d, dev)
    ckv = _bf(torch.randn(B, S, L * 2 * d, generator=g)).to(dev)
    p.update(ckv=ckv, Kc=ckv[:, :, layer * 2 * d: layer * 2 * d + d], Vc=ckv[:, :, layer * 2 * d + d: (layer + 1) * 2 * d],
             mask=key_mask_for(B, S).to(dev), kv_row=(torch.arange(R) // nb).to(torch.int32).to(dev), R=R, Tk=S, H=H, ldc=L * 2 * d)
    return p


def ad_inputs(c, dev):
    R, H, Tk, style = c["R"], c["H"], c["Tk"], c["style"]
    d = H * HD
    g = _gen(3000 + R * 71 + H * 13 + Tk + 5 * c["new"] + 11 * c["hist"] + len(style))
    qkv = _bf(torch.randn(R, 3 * d, generator=g) * 0.8).to(dev)
    p = dict(qkv=qkv, R=R, H=H, Tk=Tk)
    if style == "self":
        Tmax = Tk + 3
        Tc = Tk - 1 if c["new"] else Tk
        Kc, Vc = _self_cache(g, R, Tc + 1, Tmax, d)      # positions >= Tc poisoned
        p.update(Kc=Kc.to(dev), Vc=Vc.to(dev), Tmax=Tmax, hist=_history(g, R, Tc + 1, Tmax).to(dev) if c["hist"] else None)
    else:
        B = (R + 1) // 2
        ckv = _bf(torch.randn(B, Tk, 2 * d, generator=g)).to(dev)
        kv_row = (torch.arange(R) // 2).to(torch.int32)
        p.update(Kc=ckv[:, :, :d], Vc=ckv[:, :, d:], Tmax=Tk, kv_row=kv_row.to(dev), ckv=ckv)
        if style == "cross":
            p.update(mask=key_mask_for(B, Tk).to(dev), mask_row=kv_row.to(dev))
        else:   # one mask row per query row, in another order than the cache rows
            p.update(mask=key_mask_for(R, Tk).to(dev), mask_row=torch.arange(R - 1, -1, -1).to(torch.int32).to(dev))
    return p


# ------------------------------------------------------------------------------------------------ references
def self_ref(p, fn=REF.exact, **kw):
    return fn(p["z"], p["H"], W=p["W"], bias=p["bias"], q_scale=Q_SCALE, gamma=p["gamma"], beta=p["beta"], eps=EPS, Kc=p["Kc"], Vc=p["Vc"],
              Tk=p["Tk"], hist=p["hist"], self_attn=True, **kw)


def cross_ref(p, fn=REF.exact, **kw):
    return fn(p["z"], p["H"], W=p["W"], bias=p["bias"], q_scale=Q_SCALE, gamma=p["gamma"], beta=p["beta"], eps=EPS, Kc=p["Kc"], Vc=p["Vc"],
              Tk=p["Tk"], kv_row=p["kv_row"], key_mask=p["mask"], self_attn=False, **kw)


def ad_ref(c, p, fn=REF.exact, **kw):
    d = p["H"] * HD
    q = p["qkv"][:, :d]
    if c["style"] == "self":
        new = dict(k_new=p["qkv"][:, d:2 * d], v_new=p["qkv"][:, 2 * d:]) if c["new"] else {}
        return fn(q, p["H"], Kc=p["Kc"], Vc=p["Vc"], Tk=p["Tk"], hist=p["hist"], self_attn=True, **new, **kw)
    return fn(q, p["H"], Kc=p["Kc"], Vc=p["Vc"], Tk=p["Tk"], kv_row=p["kv_row"], key_mask=p["mask"], mask_row=p["mask_row"], self_attn=False, **kw)


def model_head_errors(dev="cpu"):
    """{family: worst per-(row, head) error of the rounding model against exact} over the cases above"""
    worst = {k: 0.0 for k in MODEL_HEAD_ERR}

    def take(fam, model, ex, H):
        e = float(REF.head_rel_err(model["out"], ex["out"], H).max())
        worst[fam] = max(worst[fam], e)

    for c in SELF_CASES:
        p = self_inputs(c, dev)
        take("self", self_ref(p, REF.rounding_model), self_ref(p), c["H"])
    for c in CROSS_CASES:
        p = cross_inputs(c, dev)
        kvlds = cross_route(c["nb"], c["S"], c["grouped"]) == "attn_cross_kvlds"
        take("cross_kvlds" if kvlds else "cross_vec", cross_ref(p, REF.rounding_model, weights="hi_lo" if kvlds else "fp32"), cross_ref(p), c["H"])
    for c in AD_CASES:
        p = ad_inputs(c, dev)
        take("attn_decode", ad_ref(c, p, REF.rounding_model), ad_ref(c, p), c["H"])
    return worst


# ------------------------------------------------------------------------------------------------ calling the kernels
def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


_packed = {}


def _pack(W):
    key = (W.data_ptr(), tuple(W.shape))
    if key not in _packed:
        out = torch.empty_like(W)
        check(_lib.load().kmb_op_decode_pack(ptr(W), W.stride(0), W.shape[0], W.shape[1], ptr(out), _stream()))
        _packed.clear()
        _packed[key] = (W, out)
    return _packed[key][1]


def block_struct(p, kind, out, ln_out, **extra):
    d = p["H"] * HD
    b = KmbDecodeBlock()
    b.kind, b.in_, b.ld_in, b.gamma, b.beta, b.eps, b.ln_out = kind, ptr(p["z"]), D, ptr(p["gamma"]), ptr(p["beta"]), EPS, ptr(ln_out)
    b.W, b.bias, b.R, b.K, b.N = ptr(_pack(p["W"])), ptr(p["bias"]), p["R"], D, (3 if kind == 1 else 1) * d
    b.out, b.ld_out, b.H, b.q_scale = ptr(out), d, p["H"], Q_SCALE
    b.Kc, b.Vc, b.Tk = ptr(p["Kc"]), ptr(p["Vc"]), p["Tk"]
    for k, v in extra.items():
        setattr(b, k, ptr(v) if torch.is_tensor(v) else v)
    return b


def run_block(b, want_route):
    lib = _lib.load()
    route = lib.kmb_debug_decode_route(C.byref(b))
    assert route >= 0 and DECODE_ROUTES[route] == want_route, (route, want_route)
    check(lib.kmb_op_decode_block(C.byref(b), _stream()))
    torch.cuda.synchronize()


def run_self(p, Kc=None, Vc=None, hist=None):
    """-> out, ln_out, Kc, Vc, hist after the call (clones of the inputs unless given)"""
    d = p["H"] * HD
    Kc = p["Kc"].clone() if Kc is None else Kc
    Vc = p["Vc"].clone() if Vc is None else Vc
    hist = p["hist"].clone() if hist is None else hist
    out = torch.full((p["R"], d), 7.0, dtype=torch.bfloat16, device=DEV)
    ln_out = torch.full((p["R"], D), 7.0, dtype=torch.bfloat16, device=DEV)
    q = dict(p, Kc=Kc, Vc=Vc)
    run_block(block_struct(q, 1, out, ln_out, Tmax=p["Tmax"], ldc=d, hist=hist), "attn_self")
    return out, ln_out, Kc, Vc, hist


def run_cross(c, p, Kc=None, Vc=None, mask=None):
    d = p["H"] * HD
    out = torch.full((p["R"], d), 7.0, dtype=torch.bfloat16, device=DEV)
    ln_out = torch.full((p["R"], D), 7.0, dtype=torch.bfloat16, device=DEV)
    q = dict(p, Kc=p["Kc"] if Kc is None else Kc, Vc=p["Vc"] if Vc is None else Vc)
    b = block_struct(q, 2, out, ln_out, Tmax=p["Tk"], ldc=p["ldc"], kv_row=p["kv_row"], key_mask=p["mask"] if mask is None else mask,
                     mask_ld=p["Tk"], kv_group=c["nb"] if c["grouped"] else 0)
    run_block(b, cross_route(c["nb"], c["S"], c["grouped"]))
    return out, ln_out


def run_attn_decode(c, p, Kc=None, Vc=None, hist=None):
    d = p["H"] * HD
    out = torch.full((p["R"], d), 7.0, dtype=torch.bfloat16, device=DEV)
    a = KmbAttnDecode()
    a.Q, a.ldq, a.Tmax, a.R, a.H, a.Tk, a.O, a.ldo = ptr(p["qkv"]), 3 * d, p["Tmax"], p["R"], p["H"], p["Tk"], ptr(out), d
    if c["style"] == "self":
        Kc = p["Kc"].clone() if Kc is None else Kc
        Vc = p["Vc"].clone() if Vc is None else Vc
        hist = (p["hist"].clone() if p["hist"] is not None else None) if hist is None else hist
        a.Kc, a.Vc, a.ldc, a.hist = ptr(Kc), ptr(Vc), d, ptr(hist)
        if c["new"]:
            a.new_k, a.new_v, a.ld_new, a.Kw, a.Vw = ptr(p["qkv"][:, d:]), ptr(p["qkv"][:, 2 * d:]), 3 * d, ptr(Kc), ptr(Vc)
    else:
        a.Kc, a.Vc, a.ldc, a.kv_row = ptr(p["Kc"]), ptr(p["Vc"]), 2 * d, ptr(p["kv_row"])
        a.key_mask, a.mask_ld, a.mask_row = ptr(p["mask"]), p["mask"].stride(0), ptr(p["mask_row"])
    check(_lib.load().kmb_op_attn_decode(C.byref(a), _stream()))
    torch.cuda.synchronize()
    return out, Kc, Vc, hist


# ------------------------------------------------------------------------------------------------ checks
def check_heads(tag, fam, out, ex, H):
    err = REF.head_rel_err(out, ex["out"], H)
    worst = float(err.max())
    ratio = worst / HEAD_BOUND[fam] if HEAD_BOUND[fam] > 0 else float("inf")
    GPU_WORST_RATIO[fam] = max(GPU_WORST_RATIO.get(fam, 0.0), ratio)
    r, h = divmod(int(err.argmax()), H)
    print("[%s %s] worst (row, head) = (%d, %d): err %.3e, bound %.3e, ratio %.3f; family worst ratio so far %.3f"
          % (fam, tag, r, h, worst, HEAD_BOUND[fam], ratio, GPU_WORST_RATIO[fam]))
    assert worst <= HEAD_BOUND[fam], (tag, r, h, worst)


def check_ln(tag, ln_out, p, ex):
    n_g = ex["ln"] - p["beta"].double()
    ref = REF.bf16_round(ex["ln"])
    allow = REF.ulp_bf16(ref) + D * U24 * (n_g.abs() + p["beta"].double().abs())
    ratio = float(((ln_out.double() - ref).abs() / allow).max())
    print("[%s] ln_out: worst |got - bf16(exact)| / allowance %.3f" % (tag, ratio))
    assert ratio <= 1.0, (tag, ratio)


def check_new_rows(tag, got_k, got_v, p, ex, model, ln_out=None):
    """the appended rows against bf16(float64 projection of the bf16-rounded float64 LayerNorm); ln_out is only printed about"""
    d = p["H"] * HD
    x, W = model["x"], p["W"].double()
    sum_abs = x.abs() @ W.abs().t() + p["bias"].double().abs()
    # a LayerNorm element within its fp32 allowance of a bf16 rounding boundary may be stored one ulp off: that flip, through the weights
    ln = ex["ln"]
    ln_allow = D * U24 * ((ln - p["beta"].double()).abs() + p["beta"].double().abs())
    tie = (REF.ulp_bf16(x) / 2 - (ln - x).abs()) <= ln_allow
    flip = (tie.double() * REF.ulp_bf16(x)) @ W.abs().t()
    worst = {}
    flipped = (ln_out.double() != x) if ln_out is not None else None
    for name, got, cols in (("k", got_k, slice(d, 2 * d)), ("v", got_v, slice(2 * d, 3 * d))):
        ref = REF.bf16_round(model["y"][:, cols])
        diff = (got.double() - ref).abs()
        base = REF.ulp_bf16(ref) + D * U24 * sum_abs[:, cols]
        if flipped is not None and bool((diff > base).any()):
            rows = (diff > base).any(-1)
            print("[%s] %s rows over the allowance without the LayerNorm-flip term: %d, of which %d have a flipped LayerNorm element (all of "
                  "them inside the near-boundary set: %s)" % (tag, name, int(rows.sum()), int((rows & flipped.any(-1)).sum()), bool((tie | ~flipped).all())))
        worst[name] = (float((diff / base).max()), float((diff / (base + flip[:, cols])).max()), int((diff > base).sum()))
    print("[%s] appended rows: worst |got - bf16(ref)| / allowance without the LayerNorm-flip term k %.3f v %.3f (elements over: %d, %d), "
          "with it k %.3f v %.3f; LayerNorm elements near a rounding boundary: %.2f %%"
          % (tag, worst["k"][0], worst["v"][0], worst["k"][2], worst["v"][2], worst["k"][1], worst["v"][1], 100.0 * float(tie.double().mean())))
    assert worst["k"][1] <= 1.0 and worst["v"][1] <= 1.0, (tag, worst)


def check_self_bookkeeping(tag, p, Kc, Vc, hist, Tk, K0, V0, hist0):
    R = p["R"]
    assert torch.equal(hist[:, Tk - 1], torch.arange(R, dtype=torch.int32, device=hist.device)), tag
    keep = torch.ones(hist.shape[1], dtype=torch.bool, device=hist.device)
    keep[Tk - 1] = False
    assert torch.equal(hist[:, keep], hist0[:, keep]), tag
    assert torch.equal(Kc[:, keep], K0[:, keep]) and torch.equal(Vc[:, keep], V0[:, keep]), tag


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("c", SELF_CASES, ids=self_id)
def test_self_block_with_history(c):
    p = self_inputs(c, DEV)
    ex, model = self_ref(p), self_ref(p, REF.rounding_model)
    out, ln_out, Kc, Vc, hist = run_self(p)
    tag = self_id(c)
    check_self_bookkeeping(tag, p, Kc, Vc, hist, c["Tk"], p["Kc"], p["Vc"], p["hist"])
    check_ln(tag, ln_out, p, ex)
    check_new_rows(tag, Kc[:, c["Tk"] - 1], Vc[:, c["Tk"] - 1], p, ex, model, ln_out)
    check_heads(tag, "self", out, ex, c["H"])


@pytest.mark.parametrize("c", CROSS_CASES, ids=cross_id)
def test_cross_block(c):
    p = cross_inputs(c, DEV)
    ex = cross_ref(p)
    ckv0 = p["ckv"].clone()
    out, ln_out = run_cross(c, p)
    tag = cross_id(c)
    assert torch.equal(p["ckv"], ckv0)
    check_ln(tag, ln_out, p, ex)
    fam = "cross_kvlds" if cross_route(c["nb"], c["S"], c["grouped"]) == "attn_cross_kvlds" else "cross_vec"
    dead = p["R"] - c["nb"]                         # the last item has no key: zeros
    assert float(ex["out"][dead:].abs().max()) == 0.0 and float(out[dead:].float().abs().max()) == 0.0
    check_heads(tag, fam, out, ex, c["H"])


@pytest.mark.parametrize("c", [dict(B=7, nb=5, S=104, grouped=True, H=12, layers=1, layer=0), dict(B=3, nb=4, S=37, grouped=True, H=12, layers=1, layer=0),
                               dict(B=7, nb=5, S=105, grouped=True, H=12, layers=1, layer=0), dict(B=5, nb=3, S=50, grouped=False, H=12, layers=1, layer=0)],
                         ids=cross_id)
def test_cross_items_are_isolated(c):
    """change only item j's keys, values and mask: the rows of every other item are bit-identical (a KVLDS tile stages up to four items),
    the rows of item j are not"""
    p = cross_inputs(c, DEV)
    out0, _ = run_cross(c, p)
    j, nb, d = 1, c["nb"], c["H"] * HD
    g = _gen(77)
    ckv = p["ckv"].clone()
    ckv[j] = _bf(torch.randn(c["S"], 2 * d, generator=g)).to(DEV)
    mask = p["mask"].clone()
    mask[j] = 1
    mask[j, 1::3] = 0
    out1, _ = run_cross(c, p, Kc=ckv[:, :, :d], Vc=ckv[:, :, d:], mask=mask)
    mine = torch.zeros(p["R"], dtype=torch.bool, device=DEV)
    mine[j * nb:(j + 1) * nb] = True
    assert torch.equal(out0[~mine], out1[~mine])
    assert bool((out0[mine] != out1[mine]).view(nb, c["H"], HD).any(-1).all())     # every (row, head) of item j moved


@pytest.mark.parametrize("R,Tk", [(37, 22), (37, 12)])
def test_self_rows_ignore_unreferenced_cache(R, Tk):
    """change every cache entry (row, t) that no hist[r][t] names: the output is bit-identical"""
    c = dict(R=R, Tk=Tk, H=12)
    p = self_inputs(c, DEV)
    out0, _, K0, V0, _ = run_self(p)
    used = torch.zeros(R, p["Tmax"], dtype=torch.bool, device=DEV)
    t = torch.arange(Tk - 1, device=DEV)[None, :].expand(R, Tk - 1)
    used[p["hist"][:, :Tk - 1].long(), t] = True
    assert int((~used[:, :Tk - 1]).sum()) > R                   # there is something to change
    g = _gen(78)
    noise = _bf(torch.randn(R, p["Tmax"], D, generator=g) * 3.0).to(DEV)
    Kc = torch.where(used[:, :, None], p["Kc"], noise)
    Vc = torch.where(used[:, :, None], p["Vc"], -noise)
    out1, _, K1, V1, _ = run_self(p, Kc=Kc.clone(), Vc=Vc.clone())
    assert torch.equal(out0, out1)
    assert torch.equal(K0[:, Tk - 1], K1[:, Tk - 1]) and torch.equal(V0[:, Tk - 1], V1[:, Tk - 1])


def test_chained_steps_match_copy_reordered_caches():
    """4 decode steps of 3 items x 5 beams with a random within-item beam reorder between them (hist = hist[beam_idx], done here in torch):
    the fused self block and attn_decode_kernel, reading through the history index, against exact float64 over caches that were physically
    reordered (HF _reorder_cache) -- at every step"""
    R, nb, H, Tmax, steps = 15, 5, 12, 24, 4
    g = _gen(4242)
    proj = _proj_inputs(g, R, 3 * D, DEV)
    zero = lambda: torch.zeros(R, Tmax, D, dtype=torch.bfloat16, device=DEV)   # noqa: E731
    blk = dict(Kc=_poison(R, Tmax, D, 0).to(DEV), Vc=_poison(R, Tmax, D, 5).to(DEV), hist=_history(g, R, 1, Tmax).to(DEV))
    ad = dict(Kc=blk["Kc"].clone(), Vc=blk["Vc"].clone(), hist=blk["hist"].clone())
    ref_blk, ref_ad = dict(Kc=zero(), Vc=zero()), dict(Kc=zero(), Vc=zero())
    for step in range(steps):
        Tk = step + 1
        p = dict(proj, z=_bf(torch.randn(R, D, generator=g) * 1.3 + 0.2).to(DEV), R=R, Tk=Tk, H=H, Tmax=Tmax)
        ex = REF.exact(p["z"], H, W=p["W"], bias=p["bias"], q_scale=Q_SCALE, gamma=p["gamma"], beta=p["beta"], eps=EPS, Kc=ref_blk["Kc"],
                       Vc=ref_blk["Vc"], Tk=Tk, self_attn=True)
        model = REF.rounding_model(p["z"], H, W=p["W"], bias=p["bias"], q_scale=Q_SCALE, gamma=p["gamma"], beta=p["beta"], eps=EPS,
                                   Kc=ref_blk["Kc"], Vc=ref_blk["Vc"], Tk=Tk, self_attn=True)
        out, _, _, _, _ = run_self(dict(p, **blk), Kc=blk["Kc"], Vc=blk["Vc"], hist=blk["hist"])
        check_new_rows("chain step %d" % step, blk["Kc"][:, Tk - 1], blk["Vc"][:, Tk - 1], p, ex, model)
        check_heads("chain block step %d" % step, "self", out, ex, H)
        ref_blk["Kc"][:, Tk - 1], ref_blk["Vc"][:, Tk - 1] = model["k_new"].to(torch.bfloat16), model["v_new"].to(torch.bfloat16)
        # attn_decode_kernel: its q / k / v rows are inputs
        c = dict(R=R, H=H, Tk=Tk, style="self", new=True, hist=True)
        q = dict(qkv=_bf(torch.randn(R, 3 * D, generator=g) * 0.8).to(DEV), R=R, H=H, Tk=Tk, Tmax=Tmax)
        ex = REF.exact(q["qkv"][:, :D], H, Kc=ref_ad["Kc"], Vc=ref_ad["Vc"], Tk=Tk, k_new=q["qkv"][:, D:2 * D], v_new=q["qkv"][:, 2 * D:], self_attn=True)
        out, _, _, _ = run_attn_decode(c, q, Kc=ad["Kc"], Vc=ad["Vc"], hist=ad["hist"])
        check_heads("chain attn_decode step %d" % step, "attn_decode", out, ex, H)
        ref_ad["Kc"][:, Tk - 1], ref_ad["Vc"][:, Tk - 1] = q["qkv"][:, D:2 * D], q["qkv"][:, 2 * D:]
        assert torch.equal(ad["Kc"][:, Tk - 1], q["qkv"][:, D:2 * D]) and torch.equal(ad["Vc"][:, Tk - 1], q["qkv"][:, 2 * D:])
        # the beam reorder: every row continues a random beam of its own item
        beam_idx = ((torch.arange(R) // nb) * nb + torch.randint(0, nb, (R,), generator=g)).to(DEV)
        for st in (blk, ad):
            assert torch.equal(st["hist"][:, Tk - 1], torch.arange(R, dtype=torch.int32, device=DEV))
            st["hist"] = st["hist"][beam_idx].contiguous()
        for st in (ref_blk, ref_ad):
            st["Kc"], st["Vc"] = REF.reorder_by_copy(st["Kc"], st["Vc"], beam_idx)


@pytest.mark.parametrize("c", AD_CASES, ids=ad_id)
def test_attn_decode_kernel(c):
    p = ad_inputs(c, DEV)
    ex = ad_ref(c, p)
    tag = ad_id(c)
    out, Kc, Vc, hist = run_attn_decode(c, p)
    R, H, Tk, d = c["R"], c["H"], c["Tk"], c["H"] * HD
    if c["style"] == "self":
        keep = torch.ones(p["Tmax"], dtype=torch.bool, device=DEV)
        if c["new"]:   # appended bit for bit at Tk - 1, recorded in the history index; nothing else moved
            keep[Tk - 1] = False
            assert torch.equal(Kc[:, Tk - 1], p["qkv"][:, d:2 * d]) and torch.equal(Vc[:, Tk - 1], p["qkv"][:, 2 * d:]), tag
            if c["hist"]:
                assert torch.equal(hist[:, Tk - 1], torch.arange(R, dtype=torch.int32, device=DEV)), tag
        assert torch.equal(Kc[:, keep], p["Kc"][:, keep]) and torch.equal(Vc[:, keep], p["Vc"][:, keep]), tag
        if c["hist"]:
            assert torch.equal(hist[:, keep], p["hist"][:, keep]), tag
    else:
        dead = ex["out"].abs().sum(-1) == 0
        assert bool(dead.any()) and float(out[dead].float().abs().max()) == 0.0, tag      # the fully masked rows: zeros
    check_heads(tag, "attn_decode", out, ex, H)


if __name__ == "__main__":
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    for fam, e in model_head_errors().items():
        print('    "%s": %.2e,' % (fam, e))
