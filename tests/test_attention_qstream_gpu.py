"""GPU: the query-streaming attention kernels (csrc/attention.hip attn_fwd_qstream_kernel / attn_bwd_qstream_kernel): Tq > 64, Tk <= 64, not
causal -- G targets of T tokens attending to one input's keys as one problem of Tq = G T query rows.

1. Every case first asserts kmb_debug_attn_route == 3 in both directions: the new kernels ran, not the general ones.
2. Every (batch, head) item of O, dQ, dK, dV and every batch item's column sums against the fp64 reference of the same bf16
   inputs (tests/test_attention_train_gpu.py::attn_reference; with dropout tests/test_attention_dropout_gpu.py's, on the mask
   kmb_op_dropout_mask(seed, p, B * H * Tq, Tk) returns).  Bounds: MARGIN = 2 times what the rounding model of those files (P and dS rounded to
   bf16 before the products, outputs rounded to bf16) loses against fp64 on THESE cases, measured on the CPU from the cases' seeds by
   `python tests/test_attention_qstream_gpu.py`; WHOLE_BOUND holds as well.
3. Persistence: one call over all 840 items equals, bit for bit, calls over batch slices of fewer items than workgroups (no second item per
   workgroup, no cross-item prefetch), forward and backward.
4. Surroundings: outputs are allocated with sentinel rows / columns, all intact afterwards; nothing behind the last lse is written.
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

from kmbart import _lib  # noqa: E402
from kmbart._lib import check  # noqa: E402
from gpu_util import DEV, attn_bwd_fields, attn_struct, dropout_mask, stream  # noqa: E402
import test_attention_dropout_gpu as TD  # noqa: E402
from test_attention_train_gpu import (DQ_SCALE, HD, MARGIN, PAD_COLS, PAD_ROWS, WHOLE_BOUND, alloc_grads, attn_reference,  # noqa: E402,F401
                                      check_against_reference, colsum_errors, heads, item_errors, make_inputs, measure_model,
                                      run_backward, run_forward, untouched, worst, zero_sample)

FWD_GROUP, BWD_GROUP = 768, 512   # workgroups the two launchers start at the most
ROUTE_QSTREAM = 3

# ---- rounding-model measurements (`python tests/test_attention_qstream_gpu.py`, CPU, the seeds below) and the bounds = MARGIN x measured ----
# worst per-(batch, head)-item norm-wise error of the rounding model against exact fp64 over all items of all CASES; column sums per batch item
MODEL_ITEM_ERR = {"O": 2.53e-03, "dQ": 2.81e-03, "dK": 2.85e-03, "dV": 2.53e-03}   # (O: tests/test_attention_dropout_gpu.py::measure_model, all-keep mask)
MODEL_COLSUM_ERR = {"row": 2.88e-03, "part": 9.23e-04}
# ... of DROP_CASES at p = 0.1 and 0.5 (tests/test_attention_dropout_gpu.py::measure_model)
MODEL_ITEM_ERR_DROP = {"O": 2.77e-03, "dQ": 3.09e-03, "dK": 3.11e-03, "dV": 2.84e-03}
MODEL_COLSUM_ERR_DROP = {"row": 3.14e-03, "part": 1.07e-03}
ITEM_BOUND = {k: MARGIN * v for k, v in MODEL_ITEM_ERR.items()}
COLSUM_BOUND = {k: MARGIN * v for k, v in MODEL_COLSUM_ERR.items()}
ITEM_BOUND_DROP = {k: MARGIN * v for k, v in MODEL_ITEM_ERR_DROP.items()}
COLSUM_BOUND_DROP = {k: MARGIN * v for k, v in MODEL_COLSUM_ERR_DROP.items()}

CASES = [
    # 840 items: more than the workgroups started in either direction, so the item walk and the cross-item prefetch run; three query tiles, the
    # last one half full; key mask with padding, holes and one sample without keys
    dict(name="g5_cross", B=70, H=12, Tq=160, Tk=64, causal=False, layout="cross", seed=701, drop_seed=0x1234abcd),
    dict(name="ragged", B=70, H=12, Tq=69, Tk=50, causal=False, layout="cross", seed=702, drop_seed=31337),   # five rows in the last tile, clamping on both sides
    dict(name="one_and_a_half", B=2, H=2, Tq=96, Tk=64, causal=False, layout="separate", seed=703, mask=False),   # 4 items: fewer than workgroups
    dict(name="q384", B=1, H=2, Tq=384, Tk=8, causal=False, layout="cross", seed=704, pad_off=1),              # the backward's limit
]
DROP_CASES = CASES[:2]
PROBS = (0.1, 0.5)


def routes(case, Q, K, V):
    B, H, Tq, Tk = case["B"], case["H"], case["Tq"], case["Tk"]
    O = torch.empty((B * Tq, H * HD), dtype=torch.bfloat16, device=DEV)
    lse = torch.empty((B, H, Tq), dtype=torch.float32, device=DEV)
    grads, cs, _ = alloc_grads(case, pad=False, sentinel=0.0)
    a = attn_struct(Q, K, V, B, H, Tq, Tk, None, case["causal"], O, lse)
    attn_bwd_fields(a, O, grads[0], grads[1], grads[2], cs, DQ_SCALE)
    lib = _lib.load()
    return lib.kmb_debug_attn_route(C.byref(a), 0), lib.kmb_debug_attn_route(C.byref(a), 1)


def forward_padded(case, Q, K, V, key_mask, sentinel, b0=0, nb=None, out=None, drop=None):
    """kmb_op_attn_fwd over the batch items b0 .. b0 + nb - 1 into O / lse buffers with spare columns, rows and a spare lse tail"""
    B, H, Tq, Tk = case["B"], case["H"], case["Tq"], case["Tk"]
    nb = B - b0 if nb is None else nb
    if out is None:
        Ob = torch.full((B * Tq + PAD_ROWS, H * HD + PAD_COLS), sentinel, dtype=torch.bfloat16, device=DEV)
        lb = torch.full((B * H * Tq + PAD_ROWS,), sentinel, dtype=torch.float32, device=DEV)
    else:
        Ob, lb = out
    O, lse = Ob[:B * Tq, :H * HD], lb[:B * H * Tq].view(B, H, Tq)
    rq, rk, rb = slice(b0 * Tq, (b0 + nb) * Tq), slice(b0 * Tk, (b0 + nb) * Tk), slice(b0, b0 + nb)
    a = attn_struct(Q[rq], K[rk], V[rk], nb, H, Tq, Tk, None if key_mask is None else key_mask[rb], case["causal"], O[rq], lse[rb])
    TD.set_drop(a, drop)
    check(_lib.load().kmb_op_attn_fwd(C.byref(a), stream()))
    return O, lse, (Ob, lb)


def forward_untouched(case, bufs, sentinel):
    B, H, Tq = case["B"], case["H"], case["Tq"]
    Ob, lb = bufs
    return bool((Ob[B * Tq:] == sentinel).all()) and bool((Ob[:, H * HD:] == sentinel).all()) and bool((lb[B * H * Tq:] == sentinel).all())


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_qstream_against_fp64(case):
    inp = make_inputs(case, DEV)
    Q, K, V, dO, key_mask = inp
    assert routes(case, Q, K, V) == (ROUTE_QSTREAM, ROUTE_QSTREAM)
    O, lse, bufs = forward_padded(case, Q, K, V, key_mask, 5.0)
    g1, cs1, whole1 = alloc_grads(case, pad=True, sentinel=7.0)
    run_backward(case, Q, K, V, dO, key_mask, O, lse, g1, cs1)
    torch.cuda.synchronize()
    fails = []
    if not forward_untouched(case, bufs, 5.0):
        fails.append("spare rows / columns of O or the words behind lse were written")
    if not untouched(whole1, 7.0):
        fails.append("spare rows / columns of the gradients were written")
    ref = attn_reference(case, Q, K, V, dO, key_mask)
    B, H, Tq = case["B"], case["H"], case["Tq"]
    live = torch.isfinite(ref["lse"])
    lerr = float((lse.double()[live] - ref["lse"][live]).abs().max())
    err_o, where = worst(item_errors(heads(O, B, Tq, H), ref["O"]))   # EVERY (batch, head) item of the forward output
    print(f"[{case['name']}] O: worst item {err_o:.3e} at (b, h) = {where} (< {ITEM_BOUND['O']:.3e}); lse: max abs error {lerr:.3e}")
    if not torch.isfinite(O).all():
        fails.append("O is not finite")
    if not err_o < ITEM_BOUND["O"]:
        fails.append(f"O item {where} error {err_o:.3e} >= {ITEM_BOUND['O']:.3e}")
    if not bool((lse[~live] == float("-inf")).all()):
        fails.append("a query row without keys has a finite lse")
    if not lerr < 1e-4:   # fp32 log-sum-exp of scores of magnitude < 32: 2^-19 relative on the sum and __logf's absolute error
        fails.append(f"lse error {lerr:.3e}")
    check_against_reference(case, inp, O, lse, g1, cs1, ITEM_BOUND, COLSUM_BOUND, fails)
    assert not fails, "\n".join(fails)


def test_qstream_persistent_equals_one_item_per_workgroup():
    """Both kernels over all 840 items at once (workgroups walk a second item, whose K / V / first tile are prefetched at the first item's last
    tile) against the same kernels over batch slices of fewer items than workgroups: identical bits everywhere."""
    case = CASES[0]
    B, H = case["B"], case["H"]
    assert B * H > FWD_GROUP and B * H > BWD_GROUP
    Q, K, V, dO, key_mask = make_inputs(case, DEV)
    assert routes(case, Q, K, V) == (ROUTE_QSTREAM, ROUTE_QSTREAM)
    O1, lse1, _ = forward_padded(case, Q, K, V, key_mask, 5.0)
    g1, cs1, _ = alloc_grads(case, pad=True, sentinel=7.0)
    run_backward(case, Q, K, V, dO, key_mask, O1, lse1, g1, cs1)
    step = (min(FWD_GROUP, BWD_GROUP) - 1) // H
    assert step * H < min(FWD_GROUP, BWD_GROUP)
    out = None
    g2, cs2, _ = alloc_grads(case, pad=False, sentinel=3.0)
    for b0 in range(0, B, step):
        O2, lse2, out = forward_padded(case, Q, K, V, key_mask, 3.0, b0, min(step, B - b0), out)
    for b0 in range(0, B, step):
        run_backward(case, Q, K, V, dO, key_mask, O1, lse1, g2, cs2, b0, min(step, B - b0))
    torch.cuda.synchronize()
    fails = []
    for n, x, y in zip(("O", "lse", "dQ", "dK", "dV", "dq_colsum", "dk_colsum", "dv_colsum"), (O1, lse1) + g1 + cs1, (O2, lse2) + g2 + cs2):
        same = torch.equal(x.view(torch.int16), y.view(torch.int16)) if x.dtype == torch.bfloat16 else torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))
        if not same:
            fails.append(f"{n}: the persistent run differs from the one-item-per-workgroup run")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("p", PROBS)
@pytest.mark.parametrize("case", DROP_CASES, ids=lambda c: c["name"])
def test_qstream_dropout_against_fp64(case, p):
    B, H, Tq, Tk = case["B"], case["H"], case["Tq"], case["Tk"]
    thr = TD.thr16_of(p)
    drop = (thr, case["drop_seed"], TD.scale_of(thr))
    inp = make_inputs(case, DEV)
    Q, K, V, dO, key_mask = inp
    assert routes(case, Q, K, V) == (ROUTE_QSTREAM, ROUTE_QSTREAM)
    O, lse, bufs = forward_padded(case, Q, K, V, key_mask, 5.0, drop=drop)
    grads, cs = TD.run_backward(case, inp, O, lse, drop)
    O0, lse0, _ = forward_padded(case, Q, K, V, key_mask, 5.0)
    O2, lse2, _ = forward_padded(case, Q, K, V, key_mask, 5.0, drop=drop)
    grads2, cs2 = TD.run_backward(case, inp, O2, lse2, drop)
    torch.cuda.synchronize()
    fails = []
    if not forward_untouched(case, bufs, 5.0):
        fails.append("spare rows / columns of O or the words behind lse were written")
    if not TD.same_bits([lse.contiguous()], [lse0.contiguous()]):
        fails.append("lse of the dropped forward differs from the launch with drop_thr16 = 0")
    if not TD.same_bits([O.contiguous(), lse.contiguous()] + list(grads) + [c.contiguous() for c in cs],
                        [O2.contiguous(), lse2.contiguous()] + list(grads2) + [c.contiguous() for c in cs2]):
        fails.append("the same seed gave different bits")
    if torch.equal(O, O0):
        fails.append("the dropped O equals the undropped one")
    keep = dropout_mask(case["drop_seed"], thr / 65536.0, B * H * Tq, Tk).view(B, H, Tq, Tk)   # the mask on logical coordinates
    ref = TD.attn_reference(case, Q, K, V, dO, key_mask, keep, drop[2])
    got = dict(O=heads(O, B, Tq, H), dQ=heads(grads[0], B, Tq, H), dK=heads(grads[1], B, Tk, H), dV=heads(grads[2], B, Tk, H))
    want = dict(O=ref["O"], dQ=ref["exact"][0], dK=ref["exact"][1], dV=ref["exact"][2])
    for nme in ("O", "dQ", "dK", "dV"):
        a, ex = got[nme], want[nme]
        whole_err = float((a - ex).norm() / ex.norm())
        err, where = worst(item_errors(a, ex))
        print(f"[{case['name']} p={p}] {nme}: whole {whole_err:.3e} (< {WHOLE_BOUND}); worst item {err:.3e} at (b, h) = {where} (< {ITEM_BOUND_DROP[nme]:.3e})")
        if not torch.isfinite(a).all():
            fails.append(f"{nme} is not finite")
        if not whole_err < WHOLE_BOUND:
            fails.append(f"{nme} whole-tensor error {whole_err:.3e} >= {WHOLE_BOUND}")
        if not err < ITEM_BOUND_DROP[nme]:
            fails.append(f"{nme} item {where} error {err:.3e} >= {ITEM_BOUND_DROP[nme]:.3e}")
    row, part = colsum_errors(cs, ref["exact"])
    for nme, e in (("row", row), ("part", part)):
        i = int(torch.argmax(e))
        print(f"[{case['name']} p={p}] column sums ({nme}): worst batch item {float(e[i]):.3e} at b = {i} (< {COLSUM_BOUND_DROP[nme]:.3e})")
        if not float(e[i]) < COLSUM_BOUND_DROP[nme]:
            fails.append(f"column sums ({nme}) of batch item {i}: error {float(e[i]):.3e} >= {COLSUM_BOUND_DROP[nme]:.3e}")
    zb = zero_sample(case)
    assert zb is not None and not bool(key_mask[zb].any())
    if not (all(bool((g[zb] == 0).all()) for g in got.values()) and all(bool((c[zb] == 0).all()) for c in cs)):
        fails.append(f"sample {zb} has no keys: O, dQ, dK, dV and its column sums must be exactly zero")
    dead_keys = (key_mask == 0)[:, None, :, None]
    if bool(((got["dK"] != 0) & dead_keys).any()) or bool(((got["dV"] != 0) & dead_keys).any()):
        fails.append("dK / dV of a masked key is not exactly zero")
    assert not fails, "\n".join(fails)


if __name__ == "__main__":
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    tot = {}
    for case in CASES:
        m = measure_model(case)
        m["O"] = TD.measure_model(case, 0.0)["O"]   # the forward's rounding model (P rounded to bf16 before P V, O rounded to bf16) under an all-keep mask
        print(f"{case['name']:16s} " + "  ".join(f"{k} {v:.3e}" for k, v in m.items()))
        tot = {k: max(v, tot.get(k, 0.0)) for k, v in m.items()}
    print("MODEL_ITEM_ERR = {" + ", ".join(f'"{k}": {tot[k]:.2e}' for k in ("O", "dQ", "dK", "dV")) + "}")
    print("MODEL_COLSUM_ERR = {" + ", ".join(f'"{k}": {tot[k]:.2e}' for k in ("row", "part")) + "}")
    tot = {}
    for case in DROP_CASES:
        for p in PROBS:
            m = TD.measure_model(case, p)
            print(f"{case['name']:16s} p={p} " + "  ".join(f"{k} {v:.3e}" for k, v in m.items()))
            tot = {k: max(v, tot.get(k, 0.0)) for k, v in m.items()}
    print("MODEL_ITEM_ERR_DROP = {" + ", ".join(f'"{k}": {tot[k]:.2e}' for k in ("O", "dQ", "dK", "dV")) + "}")
    print("MODEL_COLSUM_ERR_DROP = {" + ", ".join(f'"{k}": {tot[k]:.2e}' for k in ("row", "part")) + "}")
