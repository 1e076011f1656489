"""CPU: what the decode-step attention tests (tests/test_decode_attn_gpu.py) stand on, and the host-side decisions around the kernels.

  * the float64 reference itself: attention through a history index built from a chain of beam reorders equals attention over caches that
    were reordered by copy (HF _reorder_cache);
  * the recorded rounding-model constants of test_decode_attn_gpu.py are what the model gives from the same seeds;
  * kmb_debug_decode_route: which kernel every decode block runs, on both sides of every threshold (no GPU call);
  * kmb_op_attn_decode and kmb_op_decode_block refuse bad arguments before any GPU call."""
import ctypes as C

import pytest
import torch

import decode_attn_ref as REF

HD = 64
# fake operands: aligned, non-null, never dereferenced
IN, W, BIAS, OUT, KC, VC, GAMMA, BETA, LN, KVROW, MASK, HIST, RES, Q, NEWK, NEWV = (0x10000000 * (i + 1) for i in range(16))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from kmbart import _lib
    return _lib.load()


# ------------------------------------------------------------------------------------------------ the reference against itself
def test_history_index_equals_reorder_by_copy():
    """4 chained steps, 3 items x 5 beams: `exact` through hist (permuted by beam_idx after every step, caches never moved) == `exact` on caches
    gathered by beam_idx, bit for bit -- the same numbers enter the same float64 operations"""
    R, nb, H, Tmax = 15, 5, 2, 6
    d = H * HD
    g = torch.Generator().manual_seed(7)
    bf = lambda x: x.to(torch.bfloat16)   # noqa: E731
    Wm, bias = bf(torch.randn(3 * d, d, generator=g) * 0.1), torch.randn(3 * d, generator=g) * 0.1
    gamma, beta = torch.rand(d, generator=g) + 0.5, torch.randn(d, generator=g) * 0.1
    Ki, Vi = torch.zeros(R, Tmax, d, dtype=torch.bfloat16), torch.zeros(R, Tmax, d, dtype=torch.bfloat16)   # indexed: rows stay put
    Kc, Vc = Ki.clone(), Vi.clone()                                                                            # copied: rows move
    hist = torch.full((R, Tmax), -1, dtype=torch.int32)
    moved = 0
    for step in range(4):
        Tk = step + 1
        z = bf(torch.randn(R, d, generator=g))
        kw = dict(W=Wm, bias=bias, q_scale=0.125, gamma=gamma, beta=beta, Tk=Tk, self_attn=True)
        a = REF.exact(z, H, Kc=Ki, Vc=Vi, hist=hist, **kw)
        b = REF.exact(z, H, Kc=Kc, Vc=Vc, **kw)
        assert torch.equal(a["out"], b["out"]) and torch.equal(a["k_new"], b["k_new"]), step
        m = REF.rounding_model(z, H, Kc=Ki, Vc=Vi, hist=hist, **kw)
        for cache_k, cache_v in ((Ki, Vi), (Kc, Vc)):     # the append: the row's own cache row, recorded in the index
            cache_k[:, Tk - 1], cache_v[:, Tk - 1] = bf(m["k_new"]), bf(m["v_new"])
        hist[:, Tk - 1] = torch.arange(R, dtype=torch.int32)
        beam_idx = (torch.arange(R) // nb) * nb + torch.randint(0, nb, (R,), generator=g)
        moved += int((beam_idx != torch.arange(R)).sum())
        hist = hist[beam_idx]
        Kc, Vc = REF.reorder_by_copy(Kc, Vc, beam_idx)
    assert moved > 2 * R                                  # the permutations were not the identity
    assert not torch.equal(Kc[:, :4], Ki[:, :4])


def test_fully_masked_rows_are_zero_and_masks_matter():
    g = torch.Generator().manual_seed(8)
    q, K, V = (torch.randn(s, generator=g).to(torch.bfloat16) for s in ((4, 2 * HD), (2, 9, 2 * HD), (2, 9, 2 * HD)))
    mask = torch.ones(2, 9, dtype=torch.int64)
    mask[1] = 0
    mask[0, 0] = 0
    kv_row = torch.tensor([0, 1, 1, 0], dtype=torch.int32)
    o = REF.exact(q, 2, Kc=K, Vc=V, Tk=9, kv_row=kv_row, key_mask=mask, self_attn=False)["out"]
    assert float(o[1:3].abs().max()) == 0.0 and float(o[0].abs().min()) > 0.0
    # against the textbook formula on the unmasked keys
    for h in range(2):
        qh, kh, vh = q[0, h * HD:(h + 1) * HD].double(), K[0, 1:, h * HD:(h + 1) * HD].double(), V[0, 1:, h * HD:(h + 1) * HD].double()
        want = torch.softmax(kh @ qh, 0) @ vh
        assert torch.allclose(o[0, h * HD:(h + 1) * HD], want, rtol=1e-12, atol=1e-14)


def test_recorded_model_constants_are_what_the_model_gives():
    """test_decode_attn_gpu.py's bounds are 2 x these: they must come from the rounding model, not from a kernel"""
    import test_decode_attn_gpu as T
    got = T.model_head_errors("cpu")
    print(got)
    assert set(got) == set(T.MODEL_HEAD_ERR)
    for fam, e in got.items():
        assert abs(e - T.MODEL_HEAD_ERR[fam]) <= 0.02 * T.MODEL_HEAD_ERR[fam], (fam, e, T.MODEL_HEAD_ERR[fam])
    assert T.MARGIN == 2.0 and all(T.HEAD_BOUND[k] == 2.0 * v for k, v in T.MODEL_HEAD_ERR.items())
    # the KVLDS variant's weights: two bf16 numbers carry 16 significant bits
    e = torch.rand(1000, dtype=torch.float64) + 1e-3
    hi = REF.bf16_round(e)
    assert float(((hi + REF.bf16_round(e - hi) - e).abs() / e).max()) < 2.0 ** -16


# ------------------------------------------------------------------------------------------------ routes
def block(kind, R=320, K=768, N=768, H=12, Tk=20, Tmax=None, kv_group=0, ln=True, **extra):
    from kmbart._lib import KmbDecodeBlock
    b = KmbDecodeBlock()
    b.kind, b.in_, b.ld_in, b.W, b.bias, b.R, b.K, b.N, b.out, b.ld_out = kind, IN, K, W, BIAS, R, K, N, OUT, N
    if ln and K == 768:
        b.gamma, b.beta, b.eps, b.ln_out = GAMMA, BETA, 1e-5, LN
    if kind:
        b.H, b.q_scale, b.Kc, b.Vc, b.Tk, b.Tmax, b.ldc = H, 0.125, KC, VC, Tk, Tmax or max(Tk, 24), H * HD
        b.N = (3 if kind == 1 else 1) * H * HD
        b.ld_out = H * HD
    if kind == 2:
        b.kv_row, b.key_mask, b.mask_ld, b.kv_group = KVROW, MASK, Tk, kv_group
    for k, v in extra.items():
        setattr(b, k, v)
    return b


ROUTES = [
    ("proj_wide", block(0, N=3072)), ("proj_wide", block(0, N=1536)), ("proj2", block(0, N=1408)), ("proj2", block(0, N=768)),
    ("proj2", block(0, N=1600)),                                   # >= 1536 but not a multiple of 128
    ("proj4", block(0, K=1536, N=128, ln=False)), ("proj6", block(0, K=2304, N=768, ln=False)), ("proj6", block(0, K=3072, N=768, ln=False)),
    ("attn_self", block(1, Tk=1)), ("attn_self", block(1, Tk=64, Tmax=70)), ("attn_self", block(1, R=1290, Tk=19)), ("attn_self", block(1, H=3)),
    ("attn_cross_kvlds", block(2, Tk=104, kv_group=5)), ("attn_cross", block(2, Tk=105, kv_group=5)),
    ("attn_cross_kvlds", block(2, Tk=100, kv_group=4)), ("attn_cross", block(2, Tk=100, kv_group=3)),
    ("attn_cross", block(2, Tk=120, kv_group=6)), ("attn_cross", block(2, Tk=130, kv_group=5)), ("attn_cross", block(2, Tk=100, kv_group=0)),
    ("attn_cross_kvlds", block(2, Tk=1, kv_group=4)), ("attn_cross_kvlds", block(2, Tk=33, kv_group=17)),
    ("attn_cross_kvlds", block(2, Tk=104, kv_group=5, H=3)), ("attn_cross", block(2, Tk=105, kv_group=5, H=3)),
]


@pytest.mark.parametrize("want,b", ROUTES, ids=["%s-%d" % (w, i) for i, (w, _) in enumerate(ROUTES)])
def test_decode_route(lib, want, b):
    from kmbart._lib import DECODE_ROUTES
    got = lib.kmb_debug_decode_route(C.byref(b))
    assert 0 <= got < len(DECODE_ROUTES) and DECODE_ROUTES[got] == want, (got, want)


def test_the_gpu_cases_name_the_kernel_they_run(lib):
    """test_decode_attn_gpu.py labels its cross cases with a route worked out from (beams, keys); the library agrees for every one, and
    both cross kernels are reached"""
    import test_decode_attn_gpu as T
    from kmbart._lib import DECODE_ROUTES
    seen = set()
    for c in T.CROSS_CASES:
        b = block(2, R=c["B"] * c["nb"], H=c["H"], Tk=c["S"], Tmax=c["S"], kv_group=c["nb"] if c["grouped"] else 0, ldc=c["layers"] * 2 * c["H"] * HD)
        got = DECODE_ROUTES[lib.kmb_debug_decode_route(C.byref(b))]
        assert got == T.cross_route(c["nb"], c["S"], c["grouped"]), c
        seen.add(got)
    assert seen == {"attn_cross", "attn_cross_kvlds"}


def test_decode_route_refuses_what_the_block_refuses(lib):
    assert lib.kmb_debug_decode_route(None) == -1
    self_grouped, self_q_only = block(1), block(1)
    self_grouped.kv_group, self_q_only.N = 5, 768
    for bad in (block(1, Tk=0), block(1, Tk=25, Tmax=24), block(2, Tk=20, kv_group=-1), self_grouped, self_q_only,
                block(2, Kc=KC + 2), block(2, ldc=770), block(1, Kc=0), block(2, H=0), block(3), block(0, K=700), block(1, R=0),
                block(2, Tk=2000, Tmax=2000)):
        assert lib.kmb_debug_decode_route(C.byref(bad)) == -1
        assert lib.kmb_op_decode_block(C.byref(bad), None) != 0          # refused before any GPU call
        assert lib.kmb_last_error().decode().startswith("decode block:")


# ------------------------------------------------------------------------------------------------ kmb_op_attn_decode's argument check
def attn_decode(new=False, **extra):
    from kmbart._lib import KmbAttnDecode
    a = KmbAttnDecode()
    a.Q, a.ldq, a.Kc, a.Vc, a.Tmax, a.ldc, a.R, a.H, a.Tk, a.O, a.ldo = Q, 2304, KC, VC, 24, 768, 15, 12, 7, OUT, 768
    if new:
        a.new_k, a.new_v, a.ld_new, a.Kw, a.Vw = NEWK, NEWV, 2304, KC, VC
    for k, v in extra.items():
        setattr(a, k, v)
    return a


BAD_ATTN_DECODE = {
    "Tk0": dict(Tk=0), "Tk_over_Tmax": dict(Tk=25), "Tk_over_lds": dict(Tk=4097, Tmax=5000),
    "no_Q": dict(Q=0), "no_Kc": dict(Kc=0), "no_Vc": dict(Vc=0), "no_O": dict(O=0),
    "new_k_alone": dict(new_k=NEWK), "no_new_v": dict(new=True, new_v=0), "no_Kw": dict(new=True, Kw=0), "no_Vw": dict(new=True, Vw=0),
    "Kw_alone": dict(Kw=KC),
    "Q_misaligned": dict(Q=Q + 8), "Kc_misaligned": dict(Kc=KC + 2), "Vc_misaligned": dict(Vc=VC + 4),
    "new_k_misaligned": dict(new=True, new_k=NEWK + 8), "new_v_misaligned": dict(new=True, new_v=NEWV + 2),
    "ldq": dict(ldq=2300), "ldc": dict(ldc=772), "ld_new": dict(new=True, ld_new=2306),
    "mask_ld": dict(key_mask=MASK, mask_ld=6),
}


@pytest.mark.parametrize("name", sorted(BAD_ATTN_DECODE))
def test_attn_decode_refuses(lib, name):
    a = attn_decode(**BAD_ATTN_DECODE[name])
    assert lib.kmb_op_attn_decode(C.byref(a), None) != 0                # returns before any GPU call: there is no GPU here
    assert lib.kmb_last_error().decode().startswith("attention decode:"), lib.kmb_last_error()


def test_attn_decode_nothing_to_do_is_not_an_error(lib):
    for kw in (dict(R=0), dict(H=0), dict(R=0, Tk=0, Q=0)):
        assert lib.kmb_op_attn_decode(C.byref(attn_decode(**kw)), None) == 0
    assert lib.kmb_op_attn_decode(None, None) != 0
