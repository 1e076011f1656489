"""GPU: attention backward the way the training step runs it -- more (batch, head) items than workgroups, the interleaved
dQ|dK|dV output layout, key masks with padding, holes and one fully masked sample, and the bias-gradient column sums.

1. attn_bwd_small_kernel (Tq, Tk <= 64) is persistent: min(items, 768) workgroups walk item += gridDim.x with the next item's
   operands prefetched into registers and the previous item's column sums written one barrier late.  One call over all items
   must equal, bit for bit, calls over batch slices of < 768 items (one item per workgroup: no prefetch, no LDS reuse).
2. Every (batch, head) item against a plain fp64 torch attention backward of the same bf16 inputs.  The per-item bounds are
   twice what a ROUNDING MODEL of the kernel loses against the exact fp64 result (same computation, P and dS rounded to bf16
   before the three products, outputs rounded to bf16): `python tests/test_attention_train_gpu.py` measures them on the CPU
   from the same seeds.  The factor 2 covers fp32 accumulation order and __expf.
3. The general kernel (Tq or Tk > 64): the same checks, its own constants.
4. The argument check refuses what the single-tile kernel cannot take (partial column sums, unaligned dK / dV) and Tq > 384.
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
from gpu_util import DEV, attn_bwd_fields, attn_struct, rel_err, stream  # noqa: E402

HD = 64
DQ_SCALE = 0.125
GROUP = 768          # workgroups attn_bwd_small_kernel's launcher starts at the most
PAD_COLS, PAD_ROWS = 8, 64

# ---- rounding-model measurements (`python tests/test_attention_train_gpu.py`, CPU, the seeds below) and the bounds = 2 x measured ----
# worst per-(batch, head)-item norm-wise error of the rounding model against exact fp64, over all items of all SMALL_CASES / GENERAL_CASES
MODEL_ITEM_ERR_SMALL = {"dQ": 3.53e-03, "dK": 3.27e-03, "dV": 2.79e-03}
MODEL_ITEM_ERR_GENERAL = {"dQ": 2.39e-03, "dK": 2.36e-03, "dV": 2.49e-03}
# worst per-batch-item norm-wise error of the model's column sums (its unrounded accumulators, as the kernels sum them) against the exact ones:
# "row" = the batch item's whole dq|dk|dv row against its norm; "part" = each of the three against the norm of the column sums of |gradient|
# (the exact dK column sums are zero -- softmax does not see a key bias -- so only the second form says anything about them)
MODEL_COLSUM_ERR_SMALL = {"row": 3.35e-03, "part": 1.22e-03}
MODEL_COLSUM_ERR_GENERAL = {"row": 2.37e-03, "part": 3.62e-04}
MARGIN = 2.0
ITEM_BOUND_SMALL = {k: MARGIN * v for k, v in MODEL_ITEM_ERR_SMALL.items()}
ITEM_BOUND_GENERAL = {k: MARGIN * v for k, v in MODEL_ITEM_ERR_GENERAL.items()}
COLSUM_BOUND_SMALL = {k: MARGIN * v for k, v in MODEL_COLSUM_ERR_SMALL.items()}
COLSUM_BOUND_GENERAL = {k: MARGIN * v for k, v in MODEL_COLSUM_ERR_GENERAL.items()}
WHOLE_BOUND = 2e-2   # whole-tensor norm-wise bound of test_ops_gpu.py::test_attention_fwd_bwd

# layout: "fused" = q|k|v rows of width 3d in, dQ|dK|dV rows of width 3d out (self-attention); "cross" = Q / dQ of width d, K|V / dK|dV of
# width 2d; "separate" = every tensor on its own
SMALL_CASES = [
    dict(name="enc_self", B=70, H=12, Tq=64, Tk=64, causal=False, layout="fused", seed=101),            # 840 items: 72 workgroups do 2
    dict(name="enc_self_nomask", B=70, H=12, Tq=64, Tk=64, causal=False, layout="fused", seed=101, mask=False),
    dict(name="enc_self_3rounds", B=131, H=12, Tq=64, Tk=64, causal=False, layout="fused", seed=102),   # 1572: 3 / 2 items per workgroup
    dict(name="dec_self_pack", B=131, H=12, Tq=32, Tk=32, causal=True, layout="fused", seed=103),       # two heads per tile, 786 items
    dict(name="dec_self_pack_ragged", B=262, H=12, Tq=23, Tk=23, causal=True, layout="fused", seed=104),  # ... row clamping, 1572 items
    dict(name="cross", B=70, H=12, Tq=32, Tk=64, causal=False, layout="cross", seed=105),               # rows 32 .. 63 of Q / dO never fetched
    dict(name="cross_ragged", B=70, H=12, Tq=20, Tk=50, causal=False, layout="cross", seed=106),        # clamp on both sides
    dict(name="odd_heads", B=300, H=3, Tq=32, Tk=32, causal=True, layout="fused", seed=107),            # one head per tile at T <= 32
    dict(name="q40_k30", B=70, H=12, Tq=40, Tk=30, causal=False, layout="separate", seed=108),          # K / V upper rows not fetched, Q fetched
]
GENERAL_CASES = [
    dict(name="self_130", B=2, H=3, Tq=130, Tk=130, causal=True, layout="fused", seed=201, pad_step=37),
    dict(name="cross_40_100", B=2, H=2, Tq=40, Tk=100, causal=False, layout="cross", seed=202, pad_step=37),
    dict(name="q384", B=1, H=2, Tq=384, Tk=70, causal=False, layout="cross", seed=203, pad_off=9),      # the largest Tq the LDS accumulator takes
    dict(name="q384_allzero", B=1, H=2, Tq=384, Tk=70, causal=False, layout="cross", seed=203, zero_b=0),
]


# ------------------------------------------------------------------------------------------------ inputs
def zero_sample(case):
    """The sample whose key mask is all zero: late in the batch, so that the persistent kernel meets it as a prefetched item."""
    if "zero_b" in case:
        return case["zero_b"]
    B = case["B"]
    return B - 3 if B >= 4 else (B - 1 if B >= 2 else None)


def make_key_mask(case):
    """Right padding of a different length per sample (at least five keys kept), holes inside the kept keys of some samples -- key 0 among
    them, which leaves causal query row 0 without any key -- and one sample without any key."""
    B, Tk = case["B"], case["Tk"]
    m = torch.ones((B, Tk), dtype=torch.int64)
    for b in range(B):
        kept = Tk - (b * case.get("pad_step", 1) + case.get("pad_off", 0)) % (Tk - 4)
        m[b, kept:] = 0
        if b % 7 in (0, 3):
            m[b, 1 + b % 3] = 0
            if kept > Tk // 2 + 1:
                m[b, Tk // 2] = 0
        if b % 11 == 5:
            m[b, 0] = 0
    zb = zero_sample(case)
    if zb is not None:
        m[zb] = 0
    return m


def make_inputs(case, dev):
    """bf16 Q / K / V / dO (2-D views in the case's layout) and the key mask, drawn on the CPU from the case's seed."""
    B, H, Tq, Tk = case["B"], case["H"], case["Tq"], case["Tk"]
    d = H * HD
    g = torch.Generator(device="cpu").manual_seed(case["seed"])

    def rnd(rows, cols, scale):
        return (torch.randn(rows, cols, generator=g) * scale).to(torch.bfloat16).to(dev)

    if case["layout"] == "fused":
        qkv = rnd(B * Tq, 3 * d, 0.7)
        Q, K, V = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
    elif case["layout"] == "cross":
        Q, kv = rnd(B * Tq, d, 0.7), rnd(B * Tk, 2 * d, 0.7)
        K, V = kv[:, :d], kv[:, d:]
    else:
        Q, K, V = rnd(B * Tq, d, 0.7), rnd(B * Tk, d, 0.7), rnd(B * Tk, d, 0.7)
    dO = rnd(B * Tq, d, 1.0)
    key_mask = make_key_mask(case).to(dev) if case.get("mask", True) else None
    return Q, K, V, dO, key_mask


# ------------------------------------------------------------------------------------------------ fp64 reference and rounding model
def heads(x, B, T, H):
    """[B*T, H*64] rows (any row stride) -> [B, H, T, 64] fp64"""
    return x.double().reshape(B, T, H, HD).transpose(1, 2)


def bf16_round(x):
    return x.float().to(torch.bfloat16).double()


def colsums(x):
    """[B, H, T, 64] -> [B, H*64]: the bias-gradient partial of every batch item"""
    return x.sum(dim=2).reshape(x.shape[0], -1)


def attn_reference(case, Q, K, V, dO, key_mask):
    """HF 3.0.2 SelfAttention forward / backward (q pre-scaled, -inf at masked keys and above the diagonal) in fp64 from the bf16 inputs;
    a query row without any key has P = 0 (O = 0, lse = -inf, no gradient), as csrc/attention.hip defines it.
    Returns exact (dQ * dq_scale, dK, dV), the rounding model's fp64 accumulators and its bf16-rounded outputs, each [B, H, T, 64], O and lse."""
    B, H, Tq, Tk = case["B"], case["H"], case["Tq"], case["Tk"]
    q, k, v, do = heads(Q, B, Tq, H), heads(K, B, Tk, H), heads(V, B, Tk, H), heads(dO, B, Tq, H)
    keep = torch.ones((B, 1, Tq, Tk), dtype=torch.bool, device=q.device)
    if case["causal"]:
        keep = keep & torch.tril(torch.ones((Tq, Tk), dtype=torch.bool, device=q.device))
    if key_mask is not None:
        keep = keep & (key_mask != 0)[:, None, None, :]
    s = (q @ k.transpose(-1, -2)).masked_fill(~keep, float("-inf"))
    m = s.amax(dim=-1, keepdim=True)
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    e = torch.exp(s - m)
    l = e.sum(dim=-1, keepdim=True)
    live = l > 0
    l1 = torch.where(live, l, torch.ones_like(l))
    P = torch.where(live, e / l1, torch.zeros_like(e))
    lse = torch.where(live, m + torch.log(l1), torch.full_like(l, float("-inf"))).squeeze(-1)
    O = P @ v
    dP = do @ v.transpose(-1, -2)
    dS = P * (dP - (P * dP).sum(dim=-1, keepdim=True))

    def grads(Pm, dSm):
        return (dSm @ k) * DQ_SCALE, dSm.transpose(-1, -2) @ q, Pm.transpose(-1, -2) @ do

    exact = grads(P, dS)
    model_acc = grads(bf16_round(P), bf16_round(dS))
    model = tuple(bf16_round(x) for x in model_acc)
    return dict(exact=exact, model_acc=model_acc, model=model, O=O, lse=lse)


def item_errors(a, b):
    """norm-wise error of a against b per (batch, head) item: [B, H]; an item whose b is zero must be zero in a"""
    num = (a - b).pow(2).sum(dim=(-1, -2)).sqrt()
    den = b.pow(2).sum(dim=(-1, -2)).sqrt()
    bad = torch.where(num > 0, torch.full_like(num, float("inf")), torch.zeros_like(num))
    return torch.where(den > 0, num / torch.where(den > 0, den, torch.ones_like(den)), bad)


def worst(err):
    """(value, (b, h)) of the worst item"""
    i = int(torch.argmax(err))
    return float(err.flatten()[i]), (i // err.shape[1], i % err.shape[1])


def colsum_errors(cs, exact):
    """cs: three [B, d] column-sum matrices (dq, dk, dv); exact: the exact gradients [B, H, T, 64].
    Returns per batch item the error of the whole row against the exact row's norm, and the worst of the three parts' errors against
    the norm of the column sums of |gradient| (1 where that is zero: the error itself must then be zero)."""
    ex = [colsums(x) for x in exact]
    num2 = sum((c.double() - x).pow(2).sum(dim=-1) for c, x in zip(cs, ex))
    den2 = sum(x.pow(2).sum(dim=-1) for x in ex)
    one = torch.ones_like(den2)
    row = torch.where(den2 > 0, (num2 / torch.where(den2 > 0, den2, one)).sqrt(), torch.where(num2 > 0, one * float("inf"), 0 * one))
    part = torch.zeros_like(den2)
    for c, x, gabs in zip(cs, ex, exact):
        n = (c.double() - x).pow(2).sum(dim=-1).sqrt()
        dn = colsums(gabs.abs()).pow(2).sum(dim=-1).sqrt()
        part = torch.maximum(part, torch.where(dn > 0, n / torch.where(dn > 0, dn, one), torch.where(n > 0, one * float("inf"), 0 * one)))
    return row, part


def measure_model(case, dev="cpu"):
    """What the rounding model loses against exact fp64 on this case's inputs: the figures behind the MODEL_* constants."""
    Q, K, V, dO, key_mask = make_inputs(case, dev)
    ref = attn_reference(case, Q, K, V, dO, key_mask)
    out = {n: worst(item_errors(mo, ex))[0] for n, mo, ex in zip(("dQ", "dK", "dV"), ref["model"], ref["exact"])}
    row, part = colsum_errors([colsums(x) for x in ref["model_acc"]], ref["exact"])
    out["row"], out["part"] = float(row.max()), float(part.max())
    return out


# ------------------------------------------------------------------------------------------------ kernel runs
def alloc_grads(case, pad, sentinel):
    """Gradient and column-sum buffers filled with `sentinel`; pad: 8 spare columns per row and 64 spare rows (gradients) / one spare row
    (column sums).  Returns (dQ, dK, dV) views of the valid rows, the (dq, dk, dv) column-sum views, and the list of whole buffers with the
    number of rows and columns of each that may be written."""
    B, H, Tq, Tk = case["B"], case["H"], case["Tq"], case["Tk"]
    d = H * HD
    pc, pr = (PAD_COLS, PAD_ROWS) if pad else (0, 0)

    def buf(rows, cols, extra_rows, dtype):
        return torch.full((rows + extra_rows, cols + pc), sentinel, dtype=dtype, device=DEV)

    if case["layout"] == "fused":   # the training step's dqkv buffer: dK = dqkv + d, dV = dqkv + 2d
        g = buf(B * Tq, 3 * d, pr, torch.bfloat16)
        views = (g[:B * Tq, :d], g[:B * Tk, d:2 * d], g[:B * Tk, 2 * d:3 * d])
        whole = [(g, B * Tq, 3 * d)]
    elif case["layout"] == "cross":
        gq, gkv = buf(B * Tq, d, pr, torch.bfloat16), buf(B * Tk, 2 * d, pr, torch.bfloat16)
        views = (gq[:B * Tq, :d], gkv[:B * Tk, :d], gkv[:B * Tk, d:2 * d])
        whole = [(gq, B * Tq, d), (gkv, B * Tk, 2 * d)]
    else:
        gs = [buf(B * T, d, pr, torch.bfloat16) for T in (Tq, Tk, Tk)]
        views = tuple(x[:B * T, :d] for x, T in zip(gs, (Tq, Tk, Tk)))
        whole = [(x, B * T, d) for x, T in zip(gs, (Tq, Tk, Tk))]
    cs = buf(B, 3 * d, 1 if pad else 0, torch.float32)   # the training step's partials: parts, parts + d, parts + 2d
    whole.append((cs, B, 3 * d))
    return views, (cs[:B, :d], cs[:B, d:2 * d], cs[:B, 2 * d:3 * d]), whole


def run_forward(case, Q, K, V, key_mask):
    B, H, Tq, Tk = case["B"], case["H"], case["Tq"], case["Tk"]
    O = torch.full((B * Tq, H * HD), 5.0, dtype=torch.bfloat16, device=DEV)
    lse = torch.full((B, H, Tq), 5.0, dtype=torch.float32, device=DEV)
    a = attn_struct(Q, K, V, B, H, Tq, Tk, key_mask, case["causal"], O, lse)
    check(_lib.load().kmb_op_attn_fwd(C.byref(a), stream()))
    return O, lse


def run_backward(case, Q, K, V, dO, key_mask, O, lse, grads, cs, b0=0, nb=None):
    """kmb_op_attn_bwd over the batch items b0 .. b0 + nb - 1, on slices of every tensor"""
    H, Tq, Tk = case["H"], case["Tq"], case["Tk"]
    nb = case["B"] - b0 if nb is None else nb
    rq, rk, rb = slice(b0 * Tq, (b0 + nb) * Tq), slice(b0 * Tk, (b0 + nb) * Tk), slice(b0, b0 + nb)
    a = attn_struct(Q[rq], K[rk], V[rk], nb, H, Tq, Tk, None if key_mask is None else key_mask[rb], case["causal"], O[rq], lse[rb])
    attn_bwd_fields(a, dO[rq], grads[0][rq], grads[1][rk], grads[2][rk], tuple(c[rb] for c in cs), DQ_SCALE)
    check(_lib.load().kmb_op_attn_bwd(C.byref(a), stream()))


def untouched(whole, sentinel):
    """every element outside the first `rows` x `cols` of each buffer still holds the sentinel"""
    return all(bool((x[rows:] == sentinel).all()) and bool((x[:, cols:] == sentinel).all()) for x, rows, cols in whole)


def check_against_reference(case, inp, O, lse, grads, cs, item_bound, colsum_bound, fails):
    """Section 2 of the module docstring; appends one line per missed check to `fails` and prints every figure."""
    Q, K, V, dO, key_mask = inp
    B, H, Tq, Tk = case["B"], case["H"], case["Tq"], case["Tk"]
    ref = attn_reference(case, Q, K, V, dO, key_mask)
    got = (heads(grads[0], B, Tq, H), heads(grads[1], B, Tk, H), heads(grads[2], B, Tk, H))
    for n, a, ex in zip(("dQ", "dK", "dV"), got, ref["exact"]):
        whole_err = float((a - ex).norm() / ex.norm()) if float(ex.norm()) > 0 else float(a.norm())
        err, where = worst(item_errors(a, ex))
        print(f"[{case['name']}] {n}: whole {whole_err:.3e} (< {WHOLE_BOUND}); worst item {err:.3e} at (b, h) = {where} (< {item_bound[n]:.3e})")
        if not torch.isfinite(a).all():
            fails.append(f"{n} is not finite")
        if not whole_err < WHOLE_BOUND:
            fails.append(f"{n} whole-tensor error {whole_err:.3e} >= {WHOLE_BOUND}")
        if not err < item_bound[n]:
            fails.append(f"{n} item {where} error {err:.3e} >= {item_bound[n]:.3e}")
    row, part = colsum_errors(cs, ref["exact"])
    for n, e in (("row", row), ("part", part)):
        i = int(torch.argmax(e))
        print(f"[{case['name']}] column sums ({n}): worst batch item {float(e[i]):.3e} at b = {i} (< {colsum_bound[n]:.3e})")
        if not float(e[i]) < colsum_bound[n]:
            fails.append(f"column sums ({n}) of batch item {i}: error {float(e[i]):.3e} >= {colsum_bound[n]:.3e}")
    if not all(bool(torch.isfinite(c).all()) for c in cs):
        fails.append("column sums are not finite")
    if rel_err(O, ref["O"].transpose(1, 2).reshape(B * Tq, H * HD)) >= 1e-2:   # (the forward only feeds the backward here: test_ops_gpu.py's bound)
        fails.append("forward output")
    if key_mask is not None:
        # fully masked key columns: exactly zero dK / dV
        dead = (key_mask == 0)[:, None, :, None]
        if bool(((got[1] != 0) & dead).any()) or bool(((got[2] != 0) & dead).any()):
            fails.append("dK / dV of a masked key is not exactly zero")
        zb = zero_sample(case)
        if zb is not None:   # the sample without keys: defined as all zeros, where torch's softmax would give NaN
            assert not bool(key_mask[zb].any())
            ok = bool((O[zb * Tq:(zb + 1) * Tq] == 0).all()) and bool((lse[zb] == float("-inf")).all())
            ok = ok and all(bool((g[zb] == 0).all()) for g in got) and all(bool((c[zb] == 0).all()) for c in cs)
            if not ok:
                fails.append(f"sample {zb} has no keys: O, dQ, dK, dV and its column sums must be exactly zero and lse -inf")


@pytest.mark.parametrize("case", SMALL_CASES, ids=lambda c: c["name"])
def test_attn_bwd_persistent_equals_one_item_per_workgroup(case):
    """attn_bwd_small_kernel over all items at once (workgroups take 2 - 3 items each) against the same kernel over batch slices of fewer than
    768 items (one item per workgroup): the per-item arithmetic is the same, so dQ, dK, dV and the three column-sum matrices must be
    IDENTICAL; then every item of the first run against the fp64 reference, and nothing outside the outputs is written."""
    B, H = case["B"], case["H"]
    assert case["Tq"] <= 64 and case["Tk"] <= 64
    pack = case["Tq"] <= 32 and case["Tk"] <= 32 and H % 2 == 0
    assert (B * H // 2 if pack else B * H) > GROUP, "the case must give some workgroup a second item"
    inp = make_inputs(case, DEV)
    Q, K, V, dO, key_mask = inp
    O, lse = run_forward(case, Q, K, V, key_mask)
    g1, cs1, whole1 = alloc_grads(case, pad=True, sentinel=7.0)
    run_backward(case, Q, K, V, dO, key_mask, O, lse, g1, cs1)
    g2, cs2, whole2 = alloc_grads(case, pad=False, sentinel=3.0)   # the training strides: 3d / 2d / d
    step = (GROUP - 1) // H
    assert step * H < GROUP
    for b0 in range(0, B, step):
        run_backward(case, Q, K, V, dO, key_mask, O, lse, g2, cs2, b0, min(step, B - b0))
    torch.cuda.synchronize()
    fails = []
    for n, x, y in zip(("dQ", "dK", "dV", "dq_colsum", "dk_colsum", "dv_colsum"), g1 + cs1, g2 + cs2):
        if not torch.equal(x, y):
            rows = torch.nonzero((x != y).any(dim=-1)).flatten()
            fails.append(f"{n}: persistent run differs from the one-item-per-workgroup run in {rows.numel()} rows, first {int(rows[0])}")
    if not untouched(whole1, 7.0):
        fails.append("spare rows / columns of the outputs were written")
    check_against_reference(case, inp, O, lse, g1, cs1, ITEM_BOUND_SMALL, COLSUM_BOUND_SMALL, fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("case", GENERAL_CASES, ids=lambda c: c["name"])
def test_attn_bwd_general_kernel_colsums_and_training_layout(case):
    """attn_bwd_kernel (Tq or Tk > 64): column sums, the interleaved output layouts and masks with holes against the fp64 reference.
    The "column sums (row)" bound is what made the kernel take delta = sum_k P * dP in fp32 (a pass of its own over the key tiles) instead
    of rowsum(dO * O) from the saved bf16 output: with the latter, self_130 and q384 measured 5.58e-03 and 5.65e-03 against 4.74e-03."""
    assert case["Tq"] > 64 or case["Tk"] > 64
    inp = make_inputs(case, DEV)
    Q, K, V, dO, key_mask = inp
    O, lse = run_forward(case, Q, K, V, key_mask)
    g1, cs1, whole1 = alloc_grads(case, pad=True, sentinel=7.0)
    run_backward(case, Q, K, V, dO, key_mask, O, lse, g1, cs1)
    torch.cuda.synchronize()
    fails = []
    if not untouched(whole1, 7.0):
        fails.append("spare rows / columns of the outputs were written")
    check_against_reference(case, inp, O, lse, g1, cs1, ITEM_BOUND_GENERAL, COLSUM_BOUND_GENERAL, fails)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ argument contract: refusals only
def refused(case, change):
    """A valid backward call at `case` with `change(a, grads, cs)` applied: returns the error text; every output must keep its sentinel."""
    lib = _lib.load()
    B, H, Tq, Tk = case["B"], case["H"], case["Tq"], case["Tk"]
    Q, K, V, dO, key_mask = make_inputs(case, DEV)
    O = torch.zeros((B * Tq, H * HD), dtype=torch.bfloat16, device=DEV)
    lse = torch.zeros((B, H, Tq), dtype=torch.float32, device=DEV)
    grads, cs, whole = alloc_grads(case, pad=False, sentinel=7.0)
    a = attn_struct(Q, K, V, B, H, Tq, Tk, key_mask, case["causal"], O, lse)
    attn_bwd_fields(a, dO, grads[0], grads[1], grads[2], cs, DQ_SCALE)
    change(a, grads, cs)
    rc = lib.kmb_op_attn_bwd(C.byref(a), stream())
    torch.cuda.synchronize()
    assert rc != 0, "the call was accepted"
    assert all(bool((x == 7.0).all()) for x, _, _ in whole), "a refused call wrote to its outputs"
    return lib.kmb_last_error().decode("utf-8", "replace")


TINY = dict(name="tiny", B=2, H=2, Tq=16, Tk=16, causal=False, layout="cross", seed=301)


@pytest.mark.parametrize("missing", ["dq_colsum", "dk_colsum", "dv_colsum", "dq_colsum dv_colsum", "dk_colsum dv_colsum"])
def test_attn_bwd_refuses_partial_column_sums(missing):
    """The single-tile kernel gates all three column sums on dk_colsum: a partial set is refused before any launch."""
    def change(a, grads, cs):
        for f in missing.split():
            setattr(a, f, None)
    assert "all three or none" in refused(TINY, change)


def test_attn_bwd_refuses_short_colsum_stride():
    def change(a, grads, cs):
        a.ld_colsum = TINY["H"] * HD - 8
    assert "ld_colsum" in refused(TINY, change)


@pytest.mark.parametrize("which", ["dK", "dV"])
def test_attn_bwd_refuses_unaligned_dk_dv(which):
    """dK / dV leave in 16-byte stores: a pointer 8 bytes off is refused (the row strides stay multiples of 8 elements)."""
    def change(a, grads, cs):
        g = grads[1] if which == "dK" else grads[2]
        setattr(a, which, C.c_void_p(g.data_ptr() + 8))
    assert "16-byte aligned" in refused(TINY, change)


def test_attn_bwd_refuses_tq_385():
    """Tq = 384 is the largest the general kernel's dQ accumulator takes (GENERAL_CASES runs it); 385 is refused before any launch."""
    case = dict(name="q385", B=1, H=1, Tq=385, Tk=8, causal=False, layout="cross", seed=302)
    assert "Tq > 384" in refused(case, lambda a, grads, cs: None)


if __name__ == "__main__":
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    for title, cases in (("SMALL", SMALL_CASES), ("GENERAL", GENERAL_CASES)):
        tot = {}
        for case in cases:
            m = measure_model(case)
            print(f"{case['name']:22s} " + "  ".join(f"{k} {v:.3e}" for k, v in m.items()))
            tot = {k: max(v, tot.get(k, 0.0)) for k, v in m.items()}
        print(f"MODEL_ITEM_ERR_{title} = {{" + ", ".join(f'"{k}": {tot[k]:.2e}' for k in ("dQ", "dK", "dV")) + "}")
        print(f"MODEL_COLSUM_ERR_{title} = {{" + ", ".join(f'"{k}": {tot[k]:.2e}' for k in ("row", "part")) + "}")
