"""GPU: the FP8 (e4m3) decoder-weight kernels of csrc/decode.hip, operator by operator.

  * the device quantiser kmb_op_decode_pack_fp8 returns the bytes and row exponents of the reference quantiser tests/fp8_ref.py,
    torch.equal, with the exponent rule's hand-built rows spliced in and one padded row stride;
  * every FP8 instance of the fused decode blocks returns BIT FOR BIT what the bf16 instance returns on the dequantised weights:
    the same KmbDecodeBlock once with the codes (w_format 1) and once with kmb_op_decode_pack(dequantize(...)) -- out, ln_out and the
    cache rows the self-attention block appends, torch.equal.  No tolerance: every e4m3 value is a bf16 number and a power-of-two
    scale commutes with every rounding of the fp32 sum.
Shapes are the smallest that reach every instance (PROJ2 / PROJ4 / PROJ6 / PROJ_WIDE, self, cross per row, cross with staged keys)
with partial row tiles, with and without LayerNorm, GeLU and residual; a few weight rows are scaled by 2^+-10 so that the row
exponents differ inside a 16-row tile."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import fp8_ref as Q  # noqa: E402
from gpu_util import DEV, bf, stream  # noqa: E402
from kmbart import _lib  # noqa: E402
from kmbart._lib import DECODE_ROUTES, KmbDecodeBlock, check, ptr  # noqa: E402
from test_decode_fp8_cpu import hand_built_rows  # noqa: E402


def _weight(N, K, seed):
    """bf16 [N, K] on the CPU: randn * 0.04 with a few rows scaled by 2^+-10 (different exponents inside a tile)"""
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(N, K, generator=g) * 0.04
    for r, s in ((1, 1024.0), (2, 1.0 / 1024), (N - 3, 1024.0), (N // 2, 1.0 / 1024)):
        W[r] *= s
    return W.to(torch.bfloat16)


def _pack_fp8(Wdev, N, K):
    codes = torch.zeros(N * K, dtype=torch.uint8, device=DEV)
    exps = torch.full((N,), 99, dtype=torch.int8, device=DEV)
    check(_lib.load().kmb_op_decode_pack_fp8(ptr(Wdev), Wdev.stride(0), N, K, ptr(codes), ptr(exps), stream()))
    torch.cuda.synchronize()
    return codes, exps


@pytest.mark.parametrize("N,K,ld", [(16, 64, 64), (80, 768, 768), (2304, 768, 768), (768, 3072, 3072), (80, 768, 832)])
def test_device_quantiser_equals_the_reference(N, K, ld):
    W = _weight(N, K, N + K + ld)
    hb, _ = hand_built_rows(K)
    W[4: 4 + hb.shape[0]] = hb                                    # the exponent rule's edge cases, inside a tile of random rows
    want_codes, want_exps = Q.quantize(W)
    buf = torch.full((N, ld), 7.0, dtype=torch.bfloat16, device=DEV)   # (columns past K are never read: 7.0 would change amax)
    buf[:, :K] = W.to(DEV)
    codes, exps = _pack_fp8(buf, N, K)
    assert torch.equal(exps.cpu(), want_exps)
    assert torch.equal(codes.cpu(), Q.fragment_order(want_codes))


def _run_both(W, **kw):
    """The block described by kw (tensors on the device; `fresh` names the tensors it writes) on FP8 codes of W and, from the same
    inputs, in bf16 on the dequantised W.  Returns ({name: tensor} of the FP8 run, of the bf16 run, route name)."""
    lib = _lib.load()
    fresh = kw.pop("fresh")
    N, K = W.shape
    codes, exps = _pack_fp8(W.to(DEV).contiguous(), N, K)
    want_codes, want_exps = Q.quantize(W)
    assert torch.equal(codes.cpu(), Q.fragment_order(want_codes)) and torch.equal(exps.cpu(), want_exps)
    Wd = Q.dequantize(want_codes, want_exps).to(DEV).contiguous()
    packed = torch.empty_like(Wd)
    check(lib.kmb_op_decode_pack(ptr(Wd), Wd.stride(0), N, K, ptr(packed), stream()))
    results, route = [], None
    for f8 in (True, False):
        b = KmbDecodeBlock()
        out = {}
        for k, v in kw.items():
            if torch.is_tensor(v):
                if k in fresh:
                    v = v.clone()
                    out[k] = v
                v = ptr(v)
            setattr(b, "in_" if k == "inp" else k, v)
        b.W = ptr(codes if f8 else packed)
        if f8:
            b.w_format, b.w_exp = 1, ptr(exps)
        r = lib.kmb_debug_decode_route(C.byref(b))
        assert r >= 0 and (route is None or route == r), "the format must not change the route"
        route = r
        check(lib.kmb_op_decode_block(C.byref(b), stream()))
        torch.cuda.synchronize()
        results.append(out)
    return results[0], results[1], DECODE_ROUTES[route]


def _assert_equal(got, want, what):
    for k in want:
        assert bool(torch.isfinite(want[k].float()).all()), (what, k)
        assert torch.equal(got[k], want[k]), "%s: %s differs between FP8 and bf16 on the dequantised weights (%d elements)" % (
            what, k, int((got[k] != want[k]).sum()))


@pytest.mark.parametrize("R,K,N,ln,act,res,route", [(5, 768, 64, False, 0, False, "proj2"), (37, 1536, 128, False, 0, True, "proj4"),
                                                    (37, 2304, 768, False, 1, False, "proj6"), (21, 3072, 768, False, 0, True, "proj6"),
                                                    (40, 768, 1536, True, 1, False, "proj_wide"), (37, 768, 768, True, 0, True, "proj2")])
def test_projection_block_bit_for_bit(R, K, N, ln, act, res, route):
    torch.manual_seed(R + K + N)
    W = _weight(N, K, R + K + N)
    x = bf(torch.randn(R, K, device=DEV) * 1.5 + 0.3)
    kw = dict(kind=0, inp=x, ld_in=K, bias=torch.randn(N, device=DEV) * 0.1, R=R, K=K, N=N, act=act, eps=1e-5,
              out=torch.zeros(R, N, dtype=torch.bfloat16, device=DEV), ld_out=N, fresh={"out", "ln_out"})
    if ln:
        kw.update(gamma=torch.rand(K, device=DEV) + 0.5, beta=torch.randn(K, device=DEV) * 0.1,
                  ln_out=torch.zeros(R, K, dtype=torch.bfloat16, device=DEV))
    if res:
        kw.update(residual=bf(torch.randn(R, N, device=DEV)), ld_res=N)
    got, want, ran = _run_both(W, **kw)
    assert ran == route
    assert float(want["out"].float().abs().max()) > 0
    _assert_equal(got, want, "projection R=%d K=%d N=%d" % (R, K, N))


@pytest.mark.parametrize("R,Tk", [(5, 1), (37, 7)])
def test_self_attention_block_bit_for_bit(R, Tk):
    torch.manual_seed(R * 31 + Tk)
    H, d, Tmax = 12, 768, 8
    W = _weight(3 * d, d, R + Tk)
    kw = dict(kind=1, inp=bf(torch.randn(R, d, device=DEV)), ld_in=d, gamma=torch.rand(d, device=DEV) + 0.5,
              beta=torch.randn(d, device=DEV) * 0.1, eps=1e-5, ln_out=torch.zeros(R, d, dtype=torch.bfloat16, device=DEV),
              bias=torch.randn(3 * d, device=DEV) * 0.1, R=R, K=d, N=3 * d, out=torch.zeros(R, d, dtype=torch.bfloat16, device=DEV),
              ld_out=d, H=H, q_scale=0.125, Kc=bf(torch.randn(R, Tmax, d, device=DEV)), Vc=bf(torch.randn(R, Tmax, d, device=DEV)),
              Tmax=Tmax, ldc=d, Tk=Tk, fresh={"out", "ln_out", "Kc", "Vc"})
    got, want, ran = _run_both(W, **kw)
    assert ran == "attn_self"
    assert not torch.equal(want["Kc"][:, Tk - 1], kw["Kc"][:, Tk - 1])      # the new key row was appended
    _assert_equal(got, want, "self-attention R=%d Tk=%d" % (R, Tk))


@pytest.mark.parametrize("B,nb,S,grouped,route", [(3, 4, 37, True, "attn_cross_kvlds"), (5, 3, 50, True, "attn_cross"),
                                                  (3, 4, 37, False, "attn_cross")])
def test_cross_attention_block_bit_for_bit(B, nb, S, grouped, route):
    torch.manual_seed(B + S)
    H, d, R = 12, 768, B * nb
    W = _weight(d, d, B + nb + S)
    ckv = bf(torch.randn(B, S, 2 * d, device=DEV))
    mask = torch.ones(B, S, dtype=torch.int64, device=DEV)
    for b in range(B):
        mask[b, S - (b % 7):] = 0
    kw = dict(kind=2, inp=bf(torch.randn(R, d, device=DEV)), ld_in=d, gamma=torch.rand(d, device=DEV) + 0.5,
              beta=torch.randn(d, device=DEV) * 0.1, eps=1e-5, ln_out=torch.zeros(R, d, dtype=torch.bfloat16, device=DEV),
              bias=torch.randn(d, device=DEV) * 0.1, R=R, K=d, N=d, out=torch.zeros(R, d, dtype=torch.bfloat16, device=DEV), ld_out=d,
              H=H, q_scale=0.125, Kc=ckv, Vc=ckv.view(-1)[d:], Tmax=S, ldc=2 * d, Tk=S,
              kv_row=(torch.arange(R, device=DEV) // nb).to(torch.int32), key_mask=mask, mask_ld=S, kv_group=nb if grouped else 0,
              fresh={"out", "ln_out"})
    got, want, ran = _run_both(W, **kw)
    assert ran == route
    _assert_equal(got, want, "cross-attention B=%d beams=%d S=%d grouped=%s" % (B, nb, S, grouped))
