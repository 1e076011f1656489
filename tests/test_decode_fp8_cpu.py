"""CPU: the FP8 (e4m3) decoder-weight format -- the reference quantiser tests/fp8_ref.py against the
format's own definition, the fragment order against the lane formula, and the refusals of the C ABI that need no GPU."""
import ctypes as C
import os
import re

import pytest
import torch

import fp8_ref as Q
from kmbart import _lib
from kmbart._lib import KmbConfig, KmbDecodeBlock, check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bf(x):
    return torch.as_tensor(x, dtype=torch.float32).to(torch.bfloat16)


def _next_bf16(x):
    """the bf16 number one ulp above a positive bf16 scalar tensor"""
    return (x.view(torch.int16) + 1).view(torch.bfloat16)


def hand_built_rows(K):
    """(rows bf16 [n, K], expected exponents): the exponent rule's edge cases"""
    rows, want = [], []

    def row(vals, e):
        r = torch.zeros(K, dtype=torch.bfloat16)
        if vals:
            r[: len(vals)] = torch.stack([torch.as_tensor(v, dtype=torch.bfloat16).reshape(()) for v in vals])
        rows.append(r)
        want.append(e)

    for e in (-9, 0, 5):
        amax = _bf(448.0 * 2.0 ** e)
        assert float(amax) == 448.0 * 2.0 ** e
        row([amax, -amax / 4, amax / 64], e)                       # amax exactly 448 * 2^e
        row([_next_bf16(amax.reshape(1))[0], amax / 2], e + 1)      # one bf16 ulp above
    row([], 0)                                                      # all zero
    row([-0.0, 0.0], 0)                                             # negative zero only
    row([1.0] + [2.0 ** -j for j in range(1, 21)] + [-0.0], -8)     # 20 binades below amax = 1 = 256 * 2^-8
    return torch.stack(rows), torch.tensor(want, dtype=torch.int8)


def test_exponent_rule_on_hand_built_rows():
    W, want = hand_built_rows(64)
    codes, exps = Q.quantize(W)
    assert torch.equal(exps, want), (exps.tolist(), want.tolist())
    f = codes.view(torch.float8_e4m3fn).float()
    # the largest code of a row is at most 448 and, for a row that is not zero, at least 224 (its scaled amax lies above 224, else
    # e - 1 would do, and rounds no lower)
    top = f.abs().max(dim=1).values
    nz = W.float().abs().max(dim=1).values > 0
    assert bool((top <= 448).all()) and bool((top[nz] >= 224).all())
    # negative zero keeps its sign, zero rows are zero codes
    assert codes[7, 0].item() == 0x80 and codes[7, 1].item() == 0 and int(codes[6].max()) == 0
    # the row that spans 20 binades: 2^-j * 2^8 is exact down to the smallest subnormal code 2^-9 (j = 17), ties to even below
    span = f[8, :21]
    assert span[:18].tolist() == [2.0 ** (8 - j) for j in range(18)]
    assert span[18:].tolist() == [0.0, 0.0, 0.0]                   # 2^-10 is a tie between 0 and 2^-9: even is 0


def test_exponent_clamps_and_non_finite_weights():
    big = torch.finfo(torch.bfloat16).max
    W = torch.zeros(5, 64, dtype=torch.bfloat16)
    W[0, :3] = _bf([big, -big, 1.0])                                # clamped at E_MAX: saturates at +-448
    W[1, :3] = _bf([2.0 ** -130, 2.0 ** -126, 0.0])                 # clamped at E_MIN
    W[2, :4] = _bf([float("inf"), float("-inf"), 3.0, -0.5])        # infinities do not set the range, saturate
    W[3, :3] = _bf([0.0, 1.0, -1.0])
    W[3, 0] = torch.tensor([0x7FC0], dtype=torch.int16).view(torch.bfloat16)[0]             # a NaN without the sign bit
    W[3, 3] = torch.tensor([0xFFC0 - 0x10000], dtype=torch.int16).view(torch.bfloat16)[0]   # ... and one with it
    W[4, 0] = float("inf")                                          # nothing finite but zeros
    codes, exps = Q.quantize(W)
    assert exps.tolist() == [Q.E_MAX, Q.E_MIN, -7, -8, 0]
    assert codes[0, :3].tolist() == [0x7E, 0xFE, 0x00]
    assert codes[1, :3].tolist() == [0x00, 0x08, 0x00]              # 2^-126 * 2^120 = 2^-6, 2^-130 * 2^120 = 2^-10 -> 0
    assert codes[2, :4].tolist() == [0x7E, 0xFE, 0x7C, 0xE8]        # 3 * 2^7 = 384, -0.5 * 2^7 = -64
    assert codes[3, :4].tolist() == [0x7F, 0x78, 0xF8, 0xFF]        # NaN codes keep the sign
    assert codes[4, 0].item() == 0x7E
    back = Q.dequantize(codes, exps)
    assert bool(torch.isfinite(back[[0, 1, 2, 4]]).all()) and int(torch.isnan(back[3]).sum()) == 2


@pytest.mark.parametrize("N,K,scale", [(80, 768, 0.04), (32, 128, 3.0e4), (16, 64, 1e-12)])
def test_round_trip_is_idempotent_exact_and_within_half_an_ulp(N, K, scale):
    torch.manual_seed(N + K)
    W = (torch.randn(N, K) * scale).to(torch.bfloat16)
    W[1] = W[1] * 1024
    W[2] = W[2] / 1024
    codes, exps = Q.quantize(W)
    D = Q.dequantize(codes, exps)                                   # (asserts that every value is a bf16 number)
    c2, e2 = Q.quantize(D)
    assert torch.equal(Q.dequantize(c2, e2), D), "dequantize(quantize(.)) is not idempotent"
    # e4m3 has 3 mantissa bits: a NORMAL code (scaled magnitude >= 2^-6) is within half an ulp = relative 2^-4
    scaled = W.float().abs() * Q._pow2(-exps.to(torch.int32))[:, None]
    normal = scaled >= 2.0 ** -6
    assert int(normal.sum()) > N * K // 2
    rel = ((D.float() - W.float()).abs() / W.float().abs())[normal]
    assert float(rel.max()) <= 2.0 ** -4
    # below that the codes are subnormal: absolute half an ulp of 2^-9, scaled back
    absd = (D.float() - W.float()).abs() * Q._pow2(-exps.to(torch.int32))[:, None]
    assert float(absd[~normal].max() if bool((~normal).any()) else 0.0) <= 2.0 ** -10


def test_fragment_order_is_the_lane_formula():
    N, K = 32, 128
    codes = (torch.arange(N * K, dtype=torch.int64) * 7 % 251).to(torch.uint8).view(N, K)
    got = Q.fragment_order(codes)
    assert got.numel() == N * K
    for n in range(N // 16):
        for c in range(K // 64):
            base = (n * (K // 64) + c) * 1024
            for lane in range(64):
                row, col = n * 16 + (lane & 15), c * 64 + (lane >> 4) * 16
                assert torch.equal(got[base + lane * 16: base + lane * 16 + 16], codes[row, col: col + 16]), (n, c, lane)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    return _lib.load()


def test_new_symbols_are_declared_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "kmbart.h")).read()
    declared = set(re.findall(r"\b(kmb_[a-z0-9_]+)\s*\(", header))
    for name in ("kmb_gen_set_weight_format", "kmb_op_decode_pack_fp8"):
        assert name in declared and name in _lib.PROTOTYPES and hasattr(lib, name)
    assert "KMB_WFMT_BF16 0" in header and "KMB_WFMT_FP8_E4M3 1" in header
    names = [f[0] for f in KmbDecodeBlock._fields_]
    assert names[-2:] == ["w_format", "w_exp"] and names[-3] == "kv_group"      # appended: zeroed records mean bf16
    assert lib.kmb_abi_sizeof_decode_block() == C.sizeof(KmbDecodeBlock)


def _fake_block(**kw):
    """a kind-0 block over addresses that are never read (the checks under test run before any GPU call)"""
    fake = 1 << 20
    b = KmbDecodeBlock(kind=0, in_=fake, ld_in=768, W=fake, bias=fake, R=5, K=768, N=64, out=fake, ld_out=64)
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def test_block_refusals_need_no_gpu(lib):
    assert lib.kmb_debug_decode_route(C.byref(_fake_block())) == 1                               # bf16: proj2
    assert lib.kmb_debug_decode_route(C.byref(_fake_block(w_format=1, w_exp=1 << 20))) == 1      # the route ignores the format
    b = _fake_block(w_format=1)
    assert lib.kmb_debug_decode_route(C.byref(b)) == -1
    assert lib.kmb_op_decode_block(C.byref(b), None) != 0 and b"w_exp" in lib.kmb_last_error()
    b = _fake_block(w_format=2, w_exp=1 << 20)
    assert lib.kmb_debug_decode_route(C.byref(b)) == -1
    assert lib.kmb_op_decode_block(C.byref(b), None) != 0 and b"w_format" in lib.kmb_last_error()
    b = _fake_block(w_format=1, w_exp=(1 << 20) + 2)                                             # four exponents per lane: 4-byte aligned
    assert lib.kmb_op_decode_block(C.byref(b), None) != 0 and b"w_exp" in lib.kmb_last_error()


def test_handle_format_state_and_workspace_size(lib):
    from test_cabi_cpu import VCG_BASE
    h = C.c_void_p()
    check(lib.kmb_create(C.byref(KmbConfig(**VCG_BASE)), C.byref(h)))
    try:
        bf16 = lib.kmb_gen_workspace_bytes(h, 64, 100, 5, 20, 64 * 36)
        assert lib.kmb_gen_set_weight_format(h, 2) != 0 and b"format" in lib.kmb_last_error()
        assert lib.kmb_gen_set_weight_format(h, -1) != 0
        assert lib.kmb_gen_workspace_bytes(h, 64, 100, 5, 20, 64 * 36) == bf16                   # a refused format changes nothing
        check(lib.kmb_gen_set_weight_format(h, 1))
        fp8 = lib.kmb_gen_workspace_bytes(h, 64, 100, 5, 20, 64 * 36)
        # six layers x (9 d^2 + 2 d F) elements: two bytes each in bf16, one byte plus one exponent per row in FP8 (256-byte slots)
        d, F = 768, 3072
        elems = 6 * (6 * d * d + 2 * d * F)
        rows = 6 * (3 * d + 4 * d + F)
        assert bf16 - fp8 == elems - rows, (bf16, fp8)
        check(lib.kmb_gen_set_weight_format(h, 0))
        assert lib.kmb_gen_workspace_bytes(h, 64, 100, 5, 20, 64 * 36) == bf16
    finally:
        lib.kmb_destroy(h)
    # a configuration the fused blocks do not take has no FP8 mode: refused where it is asked for
    small = dict(VCG_BASE, d_model=128, encoder_attention_heads=2, decoder_attention_heads=2, encoder_ffn_dim=256, decoder_ffn_dim=256)
    check(lib.kmb_create(C.byref(KmbConfig(**small)), C.byref(h)))
    try:
        assert lib.kmb_gen_set_weight_format(h, 1) != 0 and b"fused" in lib.kmb_last_error()
        check(lib.kmb_gen_set_weight_format(h, 0))
    finally:
        lib.kmb_destroy(h)
