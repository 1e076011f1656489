"""CPU: the host side of activation dropout -- a run-time setting of the handle (kmb_set_activation_dropout), like attention
dropout; the query entry before any forward; and the route of the new epilogue class (act 1 + dropout) through the launch
table: the eight-wave variant 6 and the two-workgroup variant 9 admit it instead of falling back to variant 11, and the same
launch without dropout routes exactly as it did before the class existed."""
import ctypes as C
import math

import pytest

from kmbart import _lib
from kmbart._lib import KmbConfig, check
from test_attention_dropout_cpu import VCG_BASE
from test_gemm_route_cpu import FORCED, PRE, problem


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    return _lib.load()


@pytest.fixture()
def handle(lib):
    h = C.c_void_p()
    check(lib.kmb_create(C.byref(KmbConfig(**VCG_BASE)), C.byref(h)))
    yield h
    lib.kmb_destroy(h)


def test_the_two_symbols_exist(lib):
    assert lib.kmb_set_activation_dropout is not None
    assert lib.kmb_activation_dropout_site is not None


def test_setter_takes_probabilities_in_the_half_open_unit_interval(lib, handle):
    for ok in (0.0, 0.1, 0.999):
        assert lib.kmb_set_activation_dropout(handle, ok) == 0, ok
    for bad in (-0.1, 1.0, math.nan):
        assert lib.kmb_set_activation_dropout(handle, bad) != 0, bad
        assert b"kmb_set_activation_dropout" in lib.kmb_last_error(), bad
    assert lib.kmb_set_activation_dropout(None, 0.1) != 0


def test_site_query_before_any_forward_returns_zeros(lib, handle):
    check(lib.kmb_set_activation_dropout(handle, 0.1))
    for kind in (0, 1):
        for layer in range(6):
            thr, seed = C.c_uint32(7), C.c_uint32(7)
            check(lib.kmb_activation_dropout_site(handle, kind, layer, C.byref(thr), C.byref(seed)))
            assert (thr.value, seed.value) == (0, 0), (kind, layer)
    thr, seed = C.c_uint32(7), C.c_uint32(7)
    for kind, layer in ((2, 0), (-1, 0), (0, 6), (1, -1), (1, 6)):
        assert lib.kmb_activation_dropout_site(handle, kind, layer, C.byref(thr), C.byref(seed)) != 0, (kind, layer)
        assert b"kmb_activation_dropout_site" in lib.kmb_last_error()
    assert lib.kmb_activation_dropout_site(handle, 0, 0, None, C.byref(seed)) != 0


def _route(lib, p, forced):
    out = (C.c_int32 * 128)()
    n = lib.kmb_debug_gemm_route(C.byref(p), forced, out, len(out))
    assert n >= 4 and (n - 1) % 3 == 0, (forced, n)
    return list(out[:n])


def _fc1(drop):
    extra = dict(drop_thr16=6554, drop_scale=1.0 / (1.0 - 6554 / 65536.0)) if drop else {}
    return problem(2048, 4096, 384, act=1, preact=PRE, ld_preact=4096, **extra)


# The routes of _fc1(False) for KMB_GEMM_VARIANT = 0 .. 16 (0: the tuner's candidate list), recorded with this probe from the library of
# the commit before the class existed: [0, configuration, kernel variant, tile_order] or [1, (configuration, variant, tile_order) ...].
ROUTES_WITHOUT_DROPOUT = [
    [1, 7, 7, 2, 23, 7, 3, 8, 8, 2, 24, 8, 3, 11, 11, 3, 27, 11, 3, 12, 12, 3, 28, 12, 3, 13, 13, 3, 29, 13, 3, 14, 14, 3, 30, 14, 3,
     15, 15, 3, 31, 15, 3, 9, 9, 2, 6, 6, 2],
    [0, 1, 1, 2], [0, 7, 7, 2], [0, 7, 7, 2], [0, 7, 7, 2], [0, 7, 7, 2], [0, 6, 6, 2], [0, 7, 7, 2], [0, 8, 8, 2], [0, 9, 9, 2],
    [0, 11, 11, 2], [0, 11, 11, 2], [0, 12, 12, 2], [0, 13, 13, 2], [0, 14, 14, 2], [0, 15, 15, 2], [0, 7, 7, 2]]


def test_gelu_dropout_runs_on_the_lean_variants(lib):
    p = _fc1(True)
    assert _route(lib, p, 6)[2] == 6     # (both fell back to variant 11 while the class was a "rare combination")
    assert _route(lib, p, 9)[2] == 9
    # the four-wave persistent kernels and the 128 x 128 kernels take it as they take the launch without dropout; the 256 x 256
    # kernel and the eight-wave persistent kernels do not carry the class (it cost them scratch): forced, they fall back to 7
    for forced in (1, 5, 7, 11, 12):
        assert _route(lib, p, forced) == ROUTES_WITHOUT_DROPOUT[forced], forced
    for forced in (8, 14, 15, 13):   # (13: 4096 columns are no whole number of its 192-column tiles)
        assert _route(lib, p, forced)[2] == 7, forced
    tuned = _route(lib, p, 0)
    assert tuned[0] == 1 and set(tuned[1::3]) == {7, 23, 11, 27, 12, 28, 9, 6}   # the candidate list without 8, 13, 14, 15
    wide = problem(2048, 3072, 384, act=1, preact=PRE, ld_preact=3072, drop_thr16=6554, drop_scale=1.1)   # 16 whole tiles of 192 columns
    assert _route(lib, wide, 13)[2] == 13
    # a four-wave persistent kernel takes only launches of whole tiles with the lean epilogue's options: an edge row sends it on
    edge = problem(2048 + 8, 4096, 384, act=1, preact=PRE, ld_preact=4096, drop_thr16=6554, drop_scale=1.1)
    for forced in (11, 12, 13, 6, 9):
        assert _route(lib, edge, forced)[2] == 7, forced
    assert _route(lib, problem(2048 + 8, 4096, 384, act=1, preact=PRE, ld_preact=4096), 11)[2] == 11   # without dropout it stays


def test_the_launch_without_dropout_routes_as_before(lib):
    got = [_route(lib, _fc1(False), forced) for forced in FORCED]
    assert got == ROUTES_WITHOUT_DROPOUT
