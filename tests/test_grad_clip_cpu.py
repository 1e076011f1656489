"""CPU: the clipped / guarded optimizer step's float64 restatement (tests/clip_ref.py) against torch's own clipping and the oracle's
HF AdamW, the new C-ABI symbols and the record's size, and the optimizer's host-side decisions that need no GPU."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import clip_ref  # noqa: E402
from kmbart import _lib  # noqa: E402
from kmbart.optim import AdamW  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("kmb_op_grad_sumsq", "kmb_op_grad_sumsq_slots", "kmb_op_clip_finish", "kmb_op_adamw_dev",
               "kmb_step_state_bytes", "kmb_bind_step_state", "kmb_grad_sumsq", "kmb_clip_finish", "kmb_adamw_step_dev",
               "kmb_step_state_read", "kmb_step_state_set_steps")


def _grads(seed, scale):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(shape, generator=g) * scale for shape in ((7, 5), (33,), (4, 4, 3))]


@pytest.mark.parametrize("max_norm,scale", [(1.0, 3.0), (0.1, 1.0), (100.0, 0.5), (0.5, 1e-4)])
def test_coefficient_equals_torch_clip_grad_norm(max_norm, scale):
    """clip_grad_norm_ works in fp32: its norm and the gradients it leaves agree with the float64 restatement to fp32 rounding
    (2^-24 per operation, a norm over 80 elements and one multiply: 1e-6 relative is ten times that)."""
    grads = _grads(3, scale)
    params = [torch.nn.Parameter(torch.zeros_like(g)) for g in grads]
    for p, g in zip(params, grads):
        p.grad = g.clone()
    total = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
    norm = clip_ref.global_norm([g.numpy() for g in grads])
    coef = clip_ref.clip_coef(norm, max_norm)
    assert abs(total - norm) <= 1e-6 * norm
    assert coef == 1.0 if norm + 1e-6 <= max_norm else coef < 1.0
    for p, g in zip(params, grads):
        np.testing.assert_allclose(p.grad.numpy(), g.numpy().astype(np.float64) * coef, rtol=1e-6, atol=0)


def test_coefficient_edge_cases():
    assert clip_ref.clip_coef(5.0, None) == 1.0 and clip_ref.clip_coef(5.0, 0.0) == 1.0
    assert clip_ref.clip_coef(float("inf"), 1.0) == 0.0
    c = clip_ref.clip_coef(float("nan"), 1.0)
    assert c != c
    assert clip_ref.global_norm([np.array([3e19], dtype=np.float32)]) == float(np.float32(3e19))   # no fp32 overflow of the square


def test_update_equals_oracle_adamw_on_clipped_gradients():
    """Three steps, the second one non-finite and skipped: the restatement equals clip_grad_norm_ + the oracle's HF AdamW run on the
    two good steps only (the skipped step must not advance the bias correction).  The oracle computes in fp32: 1e-6 relative + 2e-7
    absolute, the tolerance tests/test_ops_gpu.py uses for this arithmetic."""
    from oracle.kmbart_oracle import HFAdamW
    n, lr, wd, max_norm = 1001, 1e-3, 0.01, 0.5
    g0 = torch.Generator().manual_seed(11)
    p0 = torch.randn(n, generator=g0)
    ref_p = torch.nn.Parameter(p0.clone())
    opt = HFAdamW([ref_p], lr=lr, eps=1e-6, weight_decay=wd)
    p = p0.numpy().astype(np.float64)
    m, v = np.zeros(n), np.zeros(n)
    st = clip_ref.RefState()
    for step in range(3):
        g = torch.randn(n, generator=g0) * 0.1
        if step == 1:
            g[17] = float("inf")
        before = (p.copy(), m.copy(), v.copy())
        clip_ref.decide(st, [g.numpy()], lr, max_norm=max_norm, skip_nonfinite=True)
        clip_ref.adamw_update(p, g.numpy(), m, v, st, lr, weight_decay=wd)
        if step == 1:
            assert st.applied == 0 and st.skipped == 1 and st.steps == 1
            assert all(np.array_equal(a, b) for a, b in zip(before, (p, m, v)))
            continue
        ref_p.grad = g.clone()
        torch.nn.utils.clip_grad_norm_([ref_p], max_norm)
        opt.step()
    assert st.steps == 2 and st.skipped == 1 and opt.state[ref_p]["step"] == 2
    assert np.allclose(p, ref_p.detach().numpy(), atol=2e-7, rtol=1e-6)


def test_new_symbols_are_declared_listed_and_exported():
    import __graft_entry__
    __graft_entry__.build()
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "kmbart.h")).read()
    declared = set(re.findall(r"\b(kmb_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared, "%s is not declared in include/kmbart.h" % name
        assert name in _lib.PROTOTYPES, "%s is not in _lib.PROTOTYPES" % name
        assert hasattr(lib, name), "libkmbart_hip.so does not export %s" % name


def test_step_state_record_size_and_slot_count():
    assert C.sizeof(_lib.KmbStepState) == 24
    assert [n for n, _ in _lib.KmbStepState._fields_] == ["norm", "coef", "step_size", "applied", "steps", "skipped"]
    header = open(os.path.join(ROOT, "include", "kmbart.h")).read()
    assert re.search(r"typedef struct KmbStepState \{ float norm, coef, step_size; int32_t applied, steps, skipped; \} KmbStepState;", header)
    import __graft_entry__
    __graft_entry__.build()
    lib = _lib.load()
    # the grid (= the slots) is a function of n alone: min(ceil(n / 1024), 1024)
    for n, want in ((0, 0), (1, 1), (1024, 1), (1025, 2), (1023 * 1024, 1023), (1023 * 1024 + 1, 1024), (1 << 30, 1024)):
        assert lib.kmb_op_grad_sumsq_slots(n) == want, n


def _fake_engine_params(n=3):
    class Eng:
        index = {("p%d" % i): (64 * i, 1, 64) for i in range(n)}
        step_count = 0

    eng = Eng()
    params = []
    for i in range(n):
        p = torch.nn.Parameter(torch.zeros(64))
        p._kmb_engine, p._kmb_range, p._kmb_name = eng, (64 * i, 64), "p%d" % i
        params.append(p)
    return eng, params


def test_constructor_validation():
    _, params = _fake_engine_params()
    for bad in (-1.0, 0.0, float("nan")):
        with pytest.raises(ValueError, match="max_grad_norm"):
            AdamW(params, lr=1e-3, max_grad_norm=bad)
    assert not AdamW(params, lr=1e-3).guarded
    assert AdamW(params, lr=1e-3, max_grad_norm=0.5).guarded
    assert AdamW(params, lr=1e-3, skip_nonfinite=True).guarded


def test_begin_fused_step_declines_when_an_option_is_set(monkeypatch):
    """The data-parallel wrapper's per-piece fused tail would move parameters before the global norm exists: it is taken only with
    both options off, and declining must not advance the host step count."""
    monkeypatch.delenv("KMB_ADAMW_OVERLAP", raising=False)
    for kw, want in (({}, True), ({"max_grad_norm": 1.0}, False), ({"skip_nonfinite": True}, False)):
        eng, params = _fake_engine_params()
        opt = AdamW(params, lr=1e-3, **kw)
        opt.allow_overlap(True)
        assert opt.begin_fused_step(eng) is want
        assert eng.step_count == (1 if want else 0)
