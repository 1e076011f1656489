"""GPU: the three kernels of the clipped / guarded optimizer step on raw pointers (kmb_op_grad_sumsq, kmb_op_clip_finish,
kmb_op_adamw_dev) against numpy float64 and tests/clip_ref.py.

Element counts are the smallest at which each code path turns: 1, 3, 7, 8 (the tail alone, fewer elements than one vector, one and two
vectors), 1023 and 1024 + 5 (a partial workgroup, a second one), 1023 * 1024 + 1 + 3 (the first count whose workgroup count is the cap of
1024, plus a tail), 1024 * 1024 + 4 + 3 (one vector more than 1024 workgroups' FIRST load covers: a thread's second of its four loads per
turn) and 4 * 1024 * 1024 + 4 + 3 (a turn of 1024 workgroups covers four vectors per thread, 4 * 1024 * 1024 elements: one vector more
makes the grid-stride loop take its second turn, with three of that turn's four loads out of range)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import clip_ref  # noqa: E402
from kmbart import _lib  # noqa: E402
from kmbart._lib import KmbAdamW, KmbStepState, check, ptr  # noqa: E402
from gpu_util import DEV, stream  # noqa: E402

CAP_N = 1023 * 1024 + 1           # ceil(n / 1024) == 1024 for the first time
TURN_N = 4 * 1024 * 1024           # what 1024 workgroups cover in one turn of the grid-stride loop
COUNTS = [1, 3, 7, 8, 1023, 1024 + 5, CAP_N + 3, 1024 * 1024 + 4 + 3, TURN_N + 4 + 3]
LR, WD = 1e-3, 0.01


def lib():
    return _lib.load()


def rnd(n, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(n, generator=g) * scale).to(DEV)


def hp(grad_scale=1.0, wd=WD):
    return KmbAdamW(lr=LR, beta1=0.9, beta2=0.999, eps=1e-6, weight_decay=wd, step=0, correct_bias=1, grad_scale=grad_scale)


def new_state(steps=0, skipped=0):
    """a KmbStepState on the device as six 4-byte words (steps / skipped preset)"""
    st = torch.zeros(6, dtype=torch.int32, device=DEV)
    st[4], st[5] = steps, skipped
    return st


def read_state(st):
    torch.cuda.synchronize()
    r = KmbStepState.from_buffer_copy(st.cpu().numpy().tobytes())
    return r


def sumsq(g, partials, slot0=0, grad_scale=1.0):
    check(lib().kmb_op_grad_sumsq(ptr(g), g.numel(), grad_scale, ptr(partials), slot0, stream()))
    return lib().kmb_op_grad_sumsq_slots(g.numel())


def finish(partials, nslots, st, max_norm=0.0, skip=False, grad_scale=1.0):
    h = hp(grad_scale)
    check(lib().kmb_op_clip_finish(ptr(partials), nslots, max_norm, 1 if skip else 0, C.byref(h), ptr(st), stream()))


def test_slot_counts():
    want = {1: 1, 3: 1, 7: 1, 8: 1, 1023: 1, 1029: 2, CAP_N + 3: 1024, 1024 * 1024 + 7: 1024, TURN_N + 7: 1024}
    for n in COUNTS:
        assert lib().kmb_op_grad_sumsq_slots(n) == want[n], n


@pytest.mark.parametrize("n", COUNTS)
def test_norm_matches_numpy_float64(n):
    """Double accumulation over n <= 2^22 + 7 terms is bounded by n * 2^-53 ~ 4.7e-10 relative: 1e-9.  The record's norm is an fp32: it must be
    the float64 norm rounded once (compared after the same rounding, one ulp of slack for the double sum's last bit)."""
    g = rnd(n, seed=100 + n % 97, scale=0.3)
    ns = lib().kmb_op_grad_sumsq_slots(n)
    partials = torch.full((ns + 2,), -1.0, dtype=torch.float64, device=DEV)   # (a guard slot behind the used ones)
    assert sumsq(g, partials) == ns
    st = new_state()
    finish(partials, ns, st)
    r = read_state(st)
    ref_total = float(np.dot(g.cpu().numpy().astype(np.float64), g.cpu().numpy().astype(np.float64)))
    got_total = float(partials[:ns].sum().cpu())
    print("n %d slots %d total %.17g ref %.17g rel %.2e" % (n, ns, got_total, ref_total, abs(got_total - ref_total) / ref_total))
    assert abs(got_total - ref_total) <= 1e-9 * ref_total
    assert float(partials[ns].cpu()) == -1.0, "a workgroup wrote past its slots"
    ref_norm = np.float32(np.sqrt(ref_total))
    assert abs(np.float32(r.norm) - ref_norm) <= np.spacing(ref_norm)
    assert r.coef == 1.0 and r.applied == 1 and r.steps == 1 and r.skipped == 0


def test_grad_scale_is_part_of_the_norm():
    g = rnd(1029, seed=7)
    partials = torch.zeros(4, dtype=torch.float64, device=DEV)
    ns = sumsq(g, partials, grad_scale=0.25)
    ref = 0.0625 * float(np.dot(g.cpu().numpy().astype(np.float64), g.cpu().numpy().astype(np.float64)))
    assert abs(float(partials[:ns].sum().cpu()) - ref) <= 1e-9 * ref


def test_two_ranges_in_disjoint_slot_blocks_one_finish():
    a, b = rnd(1029, seed=1), rnd(CAP_N + 3, seed=2)
    na, nb = (lib().kmb_op_grad_sumsq_slots(x.numel()) for x in (a, b))
    partials = torch.full((na + nb + 1,), -1.0, dtype=torch.float64, device=DEV)
    assert sumsq(b, partials, slot0=na) == nb     # (launch order does not matter: each range owns its block)
    assert sumsq(a, partials, slot0=0) == na
    st = new_state()
    finish(partials, na + nb, st, max_norm=1.0)
    r = read_state(st)
    both = np.concatenate([a.cpu().numpy(), b.cpu().numpy()]).astype(np.float64)
    ref = np.sqrt(np.dot(both, both))
    assert float(partials[na + nb].cpu()) == -1.0
    # slot blocks hold each range's own sums
    ra = float(np.dot(both[:1029], both[:1029]))
    assert abs(float(partials[:na].sum().cpu()) - ra) <= 1e-9 * ra
    assert abs(np.float32(r.norm) - np.float32(ref)) <= np.spacing(np.float32(ref))
    want = clip_ref.clip_coef(ref, 1.0)
    assert abs(r.coef - want) <= 2e-7 * want and r.coef < 1.0


def test_huge_finite_gradient_does_not_overflow():
    """3e19 squares to 9e38 > FLT_MAX: the sum is formed in double, the norm is finite and equals the reference."""
    g = torch.zeros(1029, device=DEV)
    g[1027] = 3e19   # (a tail element)
    g[5] = 3e19      # (a vector element)
    partials = torch.zeros(2, dtype=torch.float64, device=DEV)
    ns = sumsq(g, partials)
    st = new_state()
    finish(partials, ns, st, max_norm=1.0, skip=True)
    r = read_state(st)
    ref = clip_ref.global_norm([g.cpu().numpy()])
    assert np.isfinite(r.norm) and abs(np.float32(r.norm) - np.float32(ref)) <= np.spacing(np.float32(ref))
    assert r.applied == 1 and r.skipped == 0
    assert abs(r.coef - clip_ref.clip_coef(ref, 1.0)) <= 2e-7 * clip_ref.clip_coef(ref, 1.0)


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
@pytest.mark.parametrize("where", ["first", "last_vector", "tail"])
def test_nonfinite_gradient_skips_the_step(bad, where):
    n = 1024 + 7                                   # 257 whole vectors, then a tail of 3
    pos = {"first": 0, "last_vector": (n // 4) * 4 - 1, "tail": n - 2}[where]
    g = rnd(n, seed=31, scale=0.1)
    g[pos] = bad
    p, m, v = rnd(n, seed=32), rnd(n, seed=33, scale=0.01), rnd(n, seed=34, scale=0.01).abs()
    pb = p.to(torch.bfloat16)
    keep = [t.clone() for t in (p, m, v, pb)]
    partials = torch.zeros(4, dtype=torch.float64, device=DEV)
    ns = sumsq(g, partials)
    st = new_state(steps=5, skipped=2)
    finish(partials, ns, st, max_norm=1.0, skip=True)
    h = hp()
    check(lib().kmb_op_adamw_dev(ptr(p), ptr(g), ptr(m), ptr(v), ptr(pb), n, C.byref(h), ptr(st), stream()))
    r = read_state(st)
    assert r.applied == 0 and r.skipped == 3 and r.steps == 5
    for got, want in zip((p, m, v, pb), keep):
        assert torch.equal(got.view(torch.uint8), want.view(torch.uint8))


def test_nonfinite_gradient_without_skip_follows_the_arithmetic():
    """skip_nonfinite off: the step is applied as torch's clip_grad_norm_ + AdamW would apply it -- an infinite norm gives coefficient 0,
    the Inf element's scaled gradient is Inf * 0 = NaN and poisons that element only; the other elements see a zero gradient."""
    n = 1029
    g = rnd(n, seed=41, scale=0.1)
    g[3] = float("inf")
    p0 = rnd(n, seed=42)
    p, m, v = p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    partials = torch.zeros(4, dtype=torch.float64, device=DEV)
    ns = sumsq(g, partials)
    st = new_state()
    finish(partials, ns, st, max_norm=1.0, skip=False)
    h = hp(wd=0.0)
    check(lib().kmb_op_adamw_dev(ptr(p), ptr(g), ptr(m), ptr(v), None, n, C.byref(h), ptr(st), stream()))
    r = read_state(st)
    assert r.applied == 1 and r.steps == 1 and r.skipped == 0 and np.isinf(r.norm) and r.coef == 0.0
    assert bool(torch.isnan(p[3])) and bool(torch.isnan(m[3]))
    others = torch.ones(n, dtype=torch.bool, device=DEV)
    others[3] = False
    assert torch.equal(p[others], p0[others]) and bool((m[others] == 0).all()) and bool((v[others] == 0).all())


@pytest.mark.parametrize("n", [7, 1024 + 5, 100003])
def test_clipped_update_matches_clip_ref(n):
    """Three clipped steps (weight decay on, bf16 mirror) against the float64 restatement at the tolerance tests/test_ops_gpu.py's AdamW test
    uses for the same fp32 arithmetic (atol 2e-7, rtol 1e-6); the mirror is the bf16 rounding of the fp32 parameters."""
    p0 = rnd(n, seed=70)
    p, m, v = p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    pb = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
    rp, rm, rv = p0.cpu().numpy().astype(np.float64), np.zeros(n), np.zeros(n)
    ref = clip_ref.RefState()
    ns = lib().kmb_op_grad_sumsq_slots(n)
    partials = torch.zeros(ns, dtype=torch.float64, device=DEV)
    st = new_state()
    max_norm = 0.25 * 0.1 * np.sqrt(n)           # about a quarter of the expected norm: every step clips
    for step in range(1, 4):
        g = rnd(n, seed=70 + step, scale=0.1)
        sumsq(g, partials, grad_scale=0.5)
        finish(partials, ns, st, max_norm=max_norm, grad_scale=0.5)
        h = hp(grad_scale=0.5)
        check(lib().kmb_op_adamw_dev(ptr(p), ptr(g), ptr(m), ptr(v), ptr(pb), n, C.byref(h), ptr(st), stream()))
        clip_ref.decide(ref, [g.cpu().numpy()], LR, max_norm=max_norm, grad_scale=0.5)
        clip_ref.adamw_update(rp, g.cpu().numpy(), rm, rv, ref, LR, weight_decay=WD, grad_scale=0.5)
        r = read_state(st)
        assert r.steps == step and r.applied == 1 and r.coef < 1.0
        assert abs(r.coef - ref.coef) <= 2e-7 * ref.coef
        assert abs(r.step_size - ref.step_size) <= 2e-7 * ref.step_size
    assert np.allclose(p.cpu().numpy(), rp, atol=2e-7, rtol=1e-6)
    assert np.allclose(m.cpu().numpy(), rm, atol=2e-7, rtol=1e-6)
    assert np.allclose(v.cpu().numpy(), rv, atol=2e-7, rtol=1e-6)
    assert torch.equal(pb, p.to(torch.bfloat16))


@pytest.mark.parametrize("n", [1024 * 1024 + 7, TURN_N + 4 + 3])
def test_two_runs_give_the_same_bits(n):
    g = rnd(n, seed=90, scale=0.1)
    p0 = rnd(n, seed=91)
    ns = lib().kmb_op_grad_sumsq_slots(n)
    out = []
    for _ in range(2):
        p, m, v = p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        partials = torch.zeros(ns, dtype=torch.float64, device=DEV)
        st = new_state()
        sumsq(g, partials)
        finish(partials, ns, st, max_norm=1.0)
        h = hp()
        check(lib().kmb_op_adamw_dev(ptr(p), ptr(g), ptr(m), ptr(v), None, n, C.byref(h), ptr(st), stream()))
        torch.cuda.synchronize()
        out.append((partials.clone(), st.clone(), p, m, v))
    for a, b in zip(*out):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
