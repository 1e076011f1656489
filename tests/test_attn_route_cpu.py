"""CPU: which kernel an attention forward / backward runs (kmb_debug_attn_route, csrc/attention.hip kmb_attn_route).

The query is answered by the function kmb_attn_fwd_launch / kmb_attn_bwd_launch themselves ask, makes no GPU call and never dereferences
the operands, so this walks both sides of every threshold in milliseconds.  Routes: 0 general, 1 single-tile, 2 single-tile with two heads
per tile, 3 query-streaming (Tq > 64, Tk <= 64, not causal); negative: the operator refuses the problem.

KMB_ATTN_QSTREAM=0 sends the query-streaming class back to the general kernels in the DIAGNOSTIC build only (csrc/diag.h: the product library
compiles every KMB_DIAG_ENV knob out), so the product library, which this test loads, must ignore the variable: that is what is tested here.
"""
import ctypes as C
import os
import subprocess
import sys

import pytest

from kmbart import _lib
from kmbart._lib import KmbAttn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HD = 64
BASE = 0x10000   # any 16-byte aligned non-null address: never dereferenced


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    return _lib.load()


def problem(Tq, Tk, causal, H=12, B=128):
    """A training-layout cross / self problem of B * H >= 1024 items (the single-tile forward starts at 1024 items) with every backward field."""
    a = KmbAttn()
    d = H * HD
    for f in ("Q", "K", "V", "O", "lse", "dO", "dQ", "dK", "dV"):
        setattr(a, f, C.c_void_p(BASE))
    a.ldq = a.ldk = a.ldv = a.ldo = a.lddo = a.lddq = a.lddk = a.lddv = d
    a.B, a.H, a.Tq, a.Tk, a.causal = B, H, Tq, Tk, int(causal)
    a.dq_scale = 0.125
    return a


# (Tq, Tk, causal, H, forward route, backward route)
TABLE = [
    (64, 64, False, 12, 1, 1),
    (32, 32, True, 12, 2, 2),
    (32, 32, True, 3, 1, 1),
    (130, 130, True, 12, 0, 0),
    (40, 100, False, 12, 0, 0),
    (384, 70, False, 12, 0, 0),
    (96, 64, True, 12, 0, 0),
    (65, 64, False, 12, 3, 3),
    (96, 64, False, 12, 3, 3),
    (160, 50, False, 12, 3, 3),
    (384, 8, False, 12, 3, 3),
    (385, 8, False, 12, 3, -1),   # the backward's Tq limit is kmb_attn_check's, whichever kernel would run
]


@pytest.mark.parametrize("Tq,Tk,causal,H,fwd,bwd", TABLE)
def test_route_table(lib, Tq, Tk, causal, H, fwd, bwd):
    B = 128 if H >= 8 else 512
    a = problem(Tq, Tk, causal, H, B)
    got_f, got_b = lib.kmb_debug_attn_route(C.byref(a), 0), lib.kmb_debug_attn_route(C.byref(a), 1)
    assert got_f == fwd, (Tq, Tk, causal, H, "forward", got_f)
    if bwd < 0:
        assert got_b < 0
    else:
        assert got_b == bwd, (Tq, Tk, causal, H, "backward", got_b)


def test_query_streaming_runs_at_every_item_count(lib):
    """One item is enough (the single-tile forward needs 1024: below that it is the general kernel, the backward has no such limit)."""
    a = problem(160, 64, False, H=1, B=1)
    assert lib.kmb_debug_attn_route(C.byref(a), 0) == 3 and lib.kmb_debug_attn_route(C.byref(a), 1) == 3
    a = problem(64, 64, False, H=1, B=1)
    assert lib.kmb_debug_attn_route(C.byref(a), 0) == 0 and lib.kmb_debug_attn_route(C.byref(a), 1) == 1


def test_tensors_of_4gb_take_the_general_kernel(lib):
    """32-bit byte offsets: B * max(Tq, Tk) * ld * 2 must stay below 2^32 for both persistent classes."""
    B = (1 << 32) // (160 * 768 * 2) + 1
    a = problem(160, 64, False, 12, B)
    assert lib.kmb_debug_attn_route(C.byref(a), 0) == 0 and lib.kmb_debug_attn_route(C.byref(a), 1) == 0
    a = problem(160, 64, False, 12, B - 1)
    assert lib.kmb_debug_attn_route(C.byref(a), 0) == 3 and lib.kmb_debug_attn_route(C.byref(a), 1) == 3
    # the backward also looks at the gradient strides (dqkv rows of width 3 d)
    a = problem(160, 64, False, 12, B - 1)
    a.lddq = 3 * 768
    assert lib.kmb_debug_attn_route(C.byref(a), 0) == 3 and lib.kmb_debug_attn_route(C.byref(a), 1) == 0


def test_refused_problems_have_no_route(lib):
    assert lib.kmb_debug_attn_route(None, 0) < 0
    a = problem(160, 64, False)
    a.ldq = 772
    assert lib.kmb_debug_attn_route(C.byref(a), 0) < 0          # row stride not a multiple of 8
    a = problem(160, 64, False)
    a.dV = None
    assert lib.kmb_debug_attn_route(C.byref(a), 0) == 3 and lib.kmb_debug_attn_route(C.byref(a), 1) < 0   # missing backward tensor


def test_product_build_ignores_the_ab_knob():
    """KMB_ATTN_QSTREAM=0 is a KMB_DIAG_ENV knob: the product library has no code that reads it (a fresh process, the variable set before load)."""
    code = ("import ctypes as C, sys\n"
            "sys.path[:0] = [%r, %r]\n"
            "import test_attn_route_cpu as T\n"
            "from kmbart import _lib\n"
            "lib = _lib.load()\n"
            "a = T.problem(160, 64, False)\n"
            "print(lib.kmb_debug_attn_route(C.byref(a), 0), lib.kmb_debug_attn_route(C.byref(a), 1))\n"
            % (os.path.join(ROOT, "km-bart_amd"), os.path.join(ROOT, "tests")))
    env = dict(os.environ, KMB_ATTN_QSTREAM="0")
    env.pop("KMB_LIB_PATH", None)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == ["3", "3"], r.stdout
