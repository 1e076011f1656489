"""GPU: dropout of the attention probabilities in the four training attention kernels (the DROP instantiations of csrc/attention.hip),
through kmb_op_attn_fwd / kmb_op_attn_bwd.

The mask is defined on logical coordinates -- keep(b, h, q, k) = element ((b * H + h) * Tq + q, k) of
kmb_op_dropout_mask(drop_seed, p, B * H * Tq, Tk) -- so the test exports it with that operator and runs plain fp64 attention with it:
P~ = keep ? P * scale : 0 goes into P V, the log-sum-exp stays the undropped softmax's, and the gradients are fp64 autograd's.

1. Every (batch, head) item of O, dQ, dK, dV and every batch item's three column sums against that reference.  The per-item bounds are
   twice what a ROUNDING MODEL of the kernels loses against exact fp64 (P~ and dS rounded to bf16 before the products, outputs rounded to
   bf16; the model's mask is drawn by torch with the same keep probability): `python tests/test_attention_dropout_gpu.py` measures them on
   the CPU from the seeds below.  The factor 2 (tests/test_attention_train_gpu.py's MARGIN) covers fp32 accumulation order and __expf.
2. lse of a dropped forward is bit-identical to the same launch with drop_thr16 = 0; rows without any key give O = 0 and zero gradients;
   nothing is NaN; drop_thr16 = 0 with any seed / scale gives the bits of a struct without the fields; the same seed gives the same
   bits, another seed another O; the exported mask keeps the expected fraction.
3. The argument check refuses drop_thr16 > 65535, a bad drop_scale and B * H * Tq beyond 32 bits.
"""
import ctypes as C
import math
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
from test_attention_train_gpu import (DQ_SCALE, HD, MARGIN, WHOLE_BOUND, alloc_grads, bf16_round, colsum_errors, colsums,  # noqa: E402
                                      heads, item_errors, make_inputs, worst, zero_sample)

# ---- rounding-model measurements (`python tests/test_attention_dropout_gpu.py`, CPU, the seeds below, p = 0.1 and 0.5) and the bounds = 2 x measured ----
# worst per-(batch, head)-item norm-wise error of the rounding model against exact fp64 over all items of all SMALL_CASES / GENERAL_CASES and both p
MODEL_ITEM_ERR_SMALL = {"O": 3.35e-03, "dQ": 3.86e-03, "dK": 3.49e-03, "dV": 3.19e-03}
MODEL_ITEM_ERR_GENERAL = {"O": 2.56e-03, "dQ": 2.55e-03, "dK": 2.50e-03, "dV": 2.55e-03}
# worst per-batch-item error of the model's column sums ("row" / "part": tests/test_attention_train_gpu.py::colsum_errors)
MODEL_COLSUM_ERR_SMALL = {"row": 3.85e-03, "part": 1.26e-03}
MODEL_COLSUM_ERR_GENERAL = {"row": 2.51e-03, "part": 4.11e-04}
ITEM_BOUND = {False: {k: MARGIN * v for k, v in MODEL_ITEM_ERR_SMALL.items()}, True: {k: MARGIN * v for k, v in MODEL_ITEM_ERR_GENERAL.items()}}
COLSUM_BOUND = {False: {k: MARGIN * v for k, v in MODEL_COLSUM_ERR_SMALL.items()}, True: {k: MARGIN * v for k, v in MODEL_COLSUM_ERR_GENERAL.items()}}

PROBS = (0.1, 0.5)
# the smallest shapes that reach every code path: >= 1024 items (the persistent forward runs and its workgroups take a second item; more than 768:
# the backward's do too), two heads per tile (PACK), one head per tile at T <= 32 (odd H), row clamping (ragged), and the general kernels
SMALL_CASES = [
    dict(name="enc_self", B=90, H=12, Tq=64, Tk=64, causal=False, layout="fused", seed=401, drop_seed=0x1234abcd),
    dict(name="dec_self_pack", B=180, H=12, Tq=32, Tk=32, causal=True, layout="fused", seed=402, drop_seed=0x0badf00d),
    dict(name="dec_self_pack_ragged", B=180, H=12, Tq=23, Tk=23, causal=True, layout="fused", seed=403, drop_seed=77),
    dict(name="odd_heads", B=342, H=3, Tq=32, Tk=32, causal=True, layout="fused", seed=404, drop_seed=0xffffffff),
    dict(name="cross", B=90, H=12, Tq=32, Tk=64, causal=False, layout="cross", seed=405, drop_seed=0x80000001),
    dict(name="cross_ragged", B=90, H=12, Tq=20, Tk=50, causal=False, layout="cross", seed=406, drop_seed=31337),
]
GENERAL_CASES = [
    dict(name="self_130", B=2, H=3, Tq=130, Tk=130, causal=True, layout="fused", seed=501, pad_step=37, drop_seed=0xdeadbeef),
    dict(name="cross_40_100", B=2, H=2, Tq=40, Tk=100, causal=False, layout="cross", seed=502, pad_step=37, drop_seed=99),
    dict(name="q384", B=1, H=2, Tq=384, Tk=70, causal=False, layout="cross", seed=503, pad_off=9, drop_seed=0x7fffffff),
]
ALL_CASES = SMALL_CASES + GENERAL_CASES


def is_general(case):
    return case["Tq"] > 64 or case["Tk"] > 64


def thr16_of(p):
    return min(int(round(p * 65536)), 65535)


def scale_of(thr16):
    return float(torch.tensor(1.0 / (1.0 - thr16 / 65536.0), dtype=torch.float32))   # the float the kernels are given


# ------------------------------------------------------------------------------------------------ fp64 reference and rounding model
def attn_reference(case, Q, K, V, dO, key_mask, keep, scale):
    """tests/test_attention_train_gpu.py::attn_reference with a `keep` mask [B, H, Tq, Tk] on the probabilities that go into P V.
    exact: O and (dQ * dq_scale, dK, dV) by fp64 autograd; model_acc / model: the rounding model's accumulators and bf16 outputs."""
    B, H, Tq, Tk = case["B"], case["H"], case["Tq"], case["Tk"]
    q, k, v = (heads(x, B, T, H).clone().requires_grad_(True) for x, T in ((Q, Tq), (K, Tk), (V, Tk)))
    do = heads(dO, B, Tq, H)
    allowed = torch.ones((B, 1, Tq, Tk), dtype=torch.bool, device=do.device)
    if case["causal"]:
        allowed = allowed & torch.tril(torch.ones((Tq, Tk), dtype=torch.bool, device=do.device))
    if key_mask is not None:
        allowed = allowed & (key_mask != 0)[:, None, None, :]
    s = (q @ k.transpose(-1, -2)).masked_fill(~allowed, float("-inf"))
    m = s.detach().amax(dim=-1, keepdim=True)
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    e = torch.exp(s - m)
    l = e.sum(dim=-1, keepdim=True)
    live = l > 0
    l1 = torch.where(live, l, torch.ones_like(l))
    P = torch.where(live, e / l1, torch.zeros_like(e))
    lse = torch.where(live, m + torch.log(l1), torch.full_like(l, float("-inf"))).squeeze(-1).detach()
    kf = keep.to(torch.float64) * scale
    O = (P * kf) @ v
    (O * do).sum().backward()
    exact = (q.grad * DQ_SCALE, k.grad, v.grad)
    with torch.no_grad():
        qd, kd, vd, Pn = q.detach(), k.detach(), v.detach(), P.detach()
        Pd = Pn * kf
        dPd = (do @ vd.transpose(-1, -2)) * kf
        dS = Pn * (dPd - (Pn * dPd).sum(dim=-1, keepdim=True))
        Pr, dSr = bf16_round(Pd), bf16_round(dS)
        model_acc = ((dSr @ kd) * DQ_SCALE, dSr.transpose(-1, -2) @ qd, Pr.transpose(-1, -2) @ do)
        model = tuple(bf16_round(x) for x in model_acc)
        O_model = bf16_round(Pr @ vd)
    return dict(exact=exact, model_acc=model_acc, model=model, O=O.detach(), O_model=O_model, lse=lse, live=live.squeeze(-1))


def measure_model(case, p, dev="cpu"):
    """What the rounding model loses against exact fp64 on this case's inputs under a torch-drawn mask of keep probability 1 - thr16 / 65536."""
    Q, K, V, dO, key_mask = make_inputs(case, dev)
    B, H, Tq, Tk = case["B"], case["H"], case["Tq"], case["Tk"]
    thr = thr16_of(p)
    g = torch.Generator(device="cpu").manual_seed(case["seed"] * 1000 + thr)
    keep = (torch.rand((B, H, Tq, Tk), generator=g) >= thr / 65536.0).to(dev)
    ref = attn_reference(case, Q, K, V, dO, key_mask, keep, scale_of(thr))
    out = {n: worst(item_errors(mo, ex))[0] for n, mo, ex in zip(("dQ", "dK", "dV"), ref["model"], ref["exact"])}
    out["O"] = worst(item_errors(ref["O_model"], ref["O"]))[0]
    row, part = colsum_errors([colsums(x) for x in ref["model_acc"]], ref["exact"])
    out["row"], out["part"] = float(row.max()), float(part.max())
    return out


# ------------------------------------------------------------------------------------------------ kernel runs
def set_drop(a, drop):
    if drop is not None:
        a.drop_thr16, a.drop_seed, a.drop_scale = drop
    return a


def run_forward(case, inp, drop):
    Q, K, V, _, key_mask = inp
    B, H, Tq, Tk = case["B"], case["H"], case["Tq"], case["Tk"]
    O = torch.full((B * Tq, H * HD), 5.0, dtype=torch.bfloat16, device=DEV)
    lse = torch.full((B, H, Tq), 5.0, dtype=torch.float32, device=DEV)
    a = set_drop(attn_struct(Q, K, V, B, H, Tq, Tk, key_mask, case["causal"], O, lse), drop)
    check(_lib.load().kmb_op_attn_fwd(C.byref(a), stream()))
    return O, lse


def run_backward(case, inp, O, lse, drop):
    Q, K, V, dO, key_mask = inp
    B, H, Tq, Tk = case["B"], case["H"], case["Tq"], case["Tk"]
    grads, cs, _ = alloc_grads(case, pad=False, sentinel=7.0)
    a = set_drop(attn_struct(Q, K, V, B, H, Tq, Tk, key_mask, case["causal"], O, lse), drop)
    attn_bwd_fields(a, dO, grads[0], grads[1], grads[2], cs, DQ_SCALE)
    check(_lib.load().kmb_op_attn_bwd(C.byref(a), stream()))
    return grads, cs


def same_bits(xs, ys):
    return all(torch.equal(x.view(torch.int16) if x.dtype == torch.bfloat16 else x.view(torch.int32), y.view(torch.int16) if y.dtype == torch.bfloat16 else y.view(torch.int32))
               for x, y in zip(xs, ys))


@pytest.mark.parametrize("p", PROBS)
@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c["name"])
def test_attention_dropout_against_fp64(case, p):
    B, H, Tq, Tk = case["B"], case["H"], case["Tq"], case["Tk"]
    gen = is_general(case)
    if not gen:
        pack = Tq <= 32 and Tk <= 32 and H % 2 == 0
        assert B * H >= 1024 and (B * H // 2 if pack else B * H) > 768, "the case must reach the persistent kernels with a second item per workgroup"
    thr = thr16_of(p)
    drop = (thr, case["drop_seed"], scale_of(thr))
    inp = make_inputs(case, DEV)
    Q, K, V, dO, key_mask = inp
    fails = []

    O, lse = run_forward(case, inp, drop)
    grads, cs = run_backward(case, inp, O, lse, drop)
    O0, lse0 = run_forward(case, inp, None)
    O2, lse2 = run_forward(case, inp, drop)
    grads2, cs2 = run_backward(case, inp, O2, lse2, drop)
    O3, _ = run_forward(case, inp, (thr, case["drop_seed"] ^ 0x5a5a5a5a, drop[2]))
    torch.cuda.synchronize()

    # ---- lse: the undropped softmax's, bit for bit; determinism; seed dependence
    if not same_bits([lse], [lse0]):
        fails.append("lse of the dropped forward differs from the launch with drop_thr16 = 0")
    if torch.isnan(lse).any():
        fails.append("lse has a NaN")
    if not same_bits([O, lse] + list(grads) + list(cs), [O2, lse2] + list(grads2) + list(cs2)):
        fails.append("the same seed gave different bits")
    if torch.equal(O, O3):
        fails.append("another seed gave the same O")
    if torch.equal(O, O0):
        fails.append("the dropped O equals the undropped one")

    # ---- the mask, exported on logical coordinates
    keep = dropout_mask(case["drop_seed"], thr / 65536.0, B * H * Tq, Tk).view(B, H, Tq, Tk)
    n, kp = keep.numel(), 1.0 - thr / 65536.0
    frac = float(keep.double().mean())
    print(f"[{case['name']} p={p}] kept {frac:.5f} of {n} (expected {kp:.5f} +- {5 * math.sqrt(kp * (1 - kp) / n):.5f})")
    if not abs(frac - kp) <= 5 * math.sqrt(kp * (1 - kp) / n):
        fails.append(f"kept fraction {frac:.5f} is more than five standard deviations from {kp:.5f}")

    ref = attn_reference(case, Q, K, V, dO, key_mask, keep, drop[2])
    item_bound, colsum_bound = ITEM_BOUND[gen], COLSUM_BOUND[gen]
    got = dict(O=heads(O, B, Tq, H), dQ=heads(grads[0], B, Tq, H), dK=heads(grads[1], B, Tk, H), dV=heads(grads[2], B, Tk, H))
    want = dict(O=ref["O"], dQ=ref["exact"][0], dK=ref["exact"][1], dV=ref["exact"][2])
    for nme in ("O", "dQ", "dK", "dV"):
        a, ex = got[nme], want[nme]
        whole_err = float((a - ex).norm() / ex.norm()) if float(ex.norm()) > 0 else float(a.norm())
        err, where = worst(item_errors(a, ex))   # EVERY (batch, head) item
        print(f"[{case['name']} p={p}] {nme}: whole {whole_err:.3e} (< {WHOLE_BOUND}); worst item {err:.3e} at (b, h) = {where} (< {item_bound[nme]:.3e})")
        if not torch.isfinite(a).all():
            fails.append(f"{nme} is not finite")
        if not whole_err < WHOLE_BOUND:
            fails.append(f"{nme} whole-tensor error {whole_err:.3e} >= {WHOLE_BOUND}")
        if not err < item_bound[nme]:
            fails.append(f"{nme} item {where} error {err:.3e} >= {item_bound[nme]:.3e}")
    row, part = colsum_errors(cs, ref["exact"])
    for nme, e in (("row", row), ("part", part)):
        i = int(torch.argmax(e))
        print(f"[{case['name']} p={p}] column sums ({nme}): worst batch item {float(e[i]):.3e} at b = {i} (< {colsum_bound[nme]:.3e})")
        if not float(e[i]) < colsum_bound[nme]:
            fails.append(f"column sums ({nme}) of batch item {i}: error {float(e[i]):.3e} >= {colsum_bound[nme]:.3e}")
    if not all(bool(torch.isfinite(c).all()) for c in cs):
        fails.append("column sums are not finite")

    # ---- rows without any key (the all-zero sample; a causal row whose only key is masked): O = 0, no gradient, lse = -inf
    dead_rows = ~ref["live"]   # [B, H, Tq]
    assert bool(dead_rows.any()) or zero_sample(case) is None, "the case must have a query row without keys"
    if bool((got["O"][dead_rows] != 0).any()) or bool((got["dQ"][dead_rows] != 0).any()):
        fails.append("a query row without keys has a non-zero O or dQ")
    if not bool((lse[dead_rows] == float("-inf")).all()):
        fails.append("a query row without keys has a finite lse")
    dead_keys = (key_mask == 0)[:, None, :, None]
    if bool(((got["dK"] != 0) & dead_keys).any()) or bool(((got["dV"] != 0) & dead_keys).any()):
        fails.append("dK / dV of a masked key is not exactly zero")
    zb = zero_sample(case)
    if zb is not None:
        assert not bool(key_mask[zb].any())
        ok = all(bool((g[zb] == 0).all()) for g in got.values()) and all(bool((c[zb] == 0).all()) for c in cs)
        if not ok:
            fails.append(f"sample {zb} has no keys: O, dQ, dK, dV and its column sums must be exactly zero")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c["name"])
def test_thr16_zero_is_a_noop(case):
    """drop_thr16 = 0 picks the kernels without dropout whatever drop_seed / drop_scale hold: the bits of a struct without the fields."""
    inp = make_inputs(case, DEV)
    O, lse = run_forward(case, inp, None)
    grads, cs = run_backward(case, inp, O, lse, None)
    O1, lse1 = run_forward(case, inp, (0, 0xdeadbeef, float("nan")))
    grads1, cs1 = run_backward(case, inp, O1, lse1, (0, 12345, -3.0))
    torch.cuda.synchronize()
    assert same_bits([O, lse] + list(grads) + list(cs), [O1, lse1] + list(grads1) + list(cs1))


# ------------------------------------------------------------------------------------------------ argument contract: refusals only
TINY = dict(name="tiny", B=2, H=2, Tq=16, Tk=16, causal=False, layout="cross", seed=601)


def refused(change, backward):
    lib = _lib.load()
    case = TINY
    B, H, Tq, Tk = case["B"], case["H"], case["Tq"], case["Tk"]
    Q, K, V, dO, key_mask = make_inputs(case, DEV)
    O = torch.full((B * Tq, H * HD), 7.0, dtype=torch.bfloat16, device=DEV)
    lse = torch.zeros((B, H, Tq), dtype=torch.float32, device=DEV)
    grads, cs, whole = alloc_grads(case, pad=False, sentinel=7.0)
    a = attn_struct(Q, K, V, B, H, Tq, Tk, key_mask, case["causal"], O, lse)
    attn_bwd_fields(a, dO, grads[0], grads[1], grads[2], cs, DQ_SCALE)
    change(a)
    rc = (lib.kmb_op_attn_bwd if backward else lib.kmb_op_attn_fwd)(C.byref(a), stream())
    torch.cuda.synchronize()
    assert rc != 0, "the call was accepted"
    assert bool((O == 7.0).all()) and all(bool((x == 7.0).all()) for x, _, _ in whole), "a refused call wrote to its outputs"
    return lib.kmb_last_error().decode("utf-8", "replace")


@pytest.mark.parametrize("backward", [False, True], ids=["fwd", "bwd"])
def test_attention_dropout_argument_check(backward):
    def thr_70000(a):
        a.drop_thr16, a.drop_seed, a.drop_scale = 70000, 1, 2.0
    assert "drop_thr16" in refused(thr_70000, backward)
    for bad_scale in (0.0, -1.0, float("inf"), float("nan")):
        def scale(a, s=bad_scale):
            a.drop_thr16, a.drop_seed, a.drop_scale = 6554, 1, s
        assert "drop_scale" in refused(scale, backward), bad_scale

    def rows_past_32_bits(a):   # sizes only: the refusal precedes any launch
        a.B = (1 << 32) // (TINY["H"] * TINY["Tq"])   # B * H * Tq = 2^32: one past the last 32-bit row index (every stride / column-sum check still holds)
    assert "32 bits" in refused(rows_past_32_bits, backward)


if __name__ == "__main__":
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    for title, cases in (("SMALL", SMALL_CASES), ("GENERAL", GENERAL_CASES)):
        tot = {}
        for case in cases:
            for p in PROBS:
                m = measure_model(case, p)
                print(f"{case['name']:22s} p={p} " + "  ".join(f"{k} {v:.3e}" for k, v in m.items()))
                tot = {k: max(v, tot.get(k, 0.0)) for k, v in m.items()}
        print(f"MODEL_ITEM_ERR_{title} = {{" + ", ".join(f'"{k}": {tot[k]:.2e}' for k in ("O", "dQ", "dK", "dV")) + "}")
        print(f"MODEL_COLSUM_ERR_{title} = {{" + ", ".join(f'"{k}": {tot[k]:.2e}' for k in ("row", "part")) + "}")
