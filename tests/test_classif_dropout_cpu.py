"""CPU: the host side of classification-head dropout -- the third run-time setting of the handle (kmb_set_classif_dropout), like attention
and activation dropout; the query entry before any forward; and the route of the two data-gradient launches head_run now requests
(act 4 + aux + dropout over the padded class dimension, act 0 + dropout without residual): the launch table sends them where it sends the
same launch without dropout, to kernels whose general epilogue carries the mask (no GEMM source changed for this feature)."""
import ctypes as C
import math

import pytest

from kmbart import _lib
from kmbart._lib import KmbConfig, check
from test_attention_dropout_cpu import VCG_BASE
from test_gemm_route_cpu import AUX, problem

THR16 = 6554
DROP = dict(drop_thr16=THR16, drop_seed=12345, drop_scale=1.0 / (1.0 - THR16 / 65536.0))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    return _lib.load()


@pytest.fixture()
def handle(lib):
    h = C.c_void_p()
    check(lib.kmb_create(C.byref(KmbConfig(num_labels=1601, num_attributes=401, num_relations=21, **VCG_BASE)), C.byref(h)))
    yield h
    lib.kmb_destroy(h)


def test_the_symbols_exist(lib):
    assert lib.kmb_set_classif_dropout is not None
    assert lib.kmb_classif_dropout_site is not None
    assert lib.kmb_op_gather_rows_drop_bf16 is not None


def test_setter_takes_probabilities_in_the_half_open_unit_interval(lib, handle):
    for ok in (0.0, 0.1, 0.999):
        assert lib.kmb_set_classif_dropout(handle, ok) == 0, ok
    for bad in (-0.1, 1.0, math.nan):
        assert lib.kmb_set_classif_dropout(handle, bad) != 0, bad
        assert b"kmb_set_classif_dropout" in lib.kmb_last_error(), bad
    assert lib.kmb_set_classif_dropout(None, 0.1) != 0
    assert b"kmb_set_classif_dropout" in lib.kmb_last_error()


def test_kmb_config_keeps_its_layout(lib):
    """the setting is not part of the creation struct: 17 int32 + 4 float + 3 int32 as before"""
    assert C.sizeof(KmbConfig) == 24 * 4
    assert "classif_dropout" not in [f[0] for f in KmbConfig._fields_]


def test_site_query_before_any_forward_returns_zeros(lib, handle):
    check(lib.kmb_set_classif_dropout(handle, 0.1))
    for head in (0, 1, 2):
        for which in (0, 1):
            thr, seed = C.c_uint32(7), C.c_uint32(7)
            check(lib.kmb_classif_dropout_site(handle, head, which, C.byref(thr), C.byref(seed)))
            assert (thr.value, seed.value) == (0, 0), (head, which)
    thr, seed = C.c_uint32(7), C.c_uint32(7)
    for head, which in ((3, 0), (-1, 0), (0, 2), (1, -1), (3, 2)):
        assert lib.kmb_classif_dropout_site(handle, head, which, C.byref(thr), C.byref(seed)) != 0, (head, which)
        assert b"kmb_classif_dropout_site" in lib.kmb_last_error()
    assert lib.kmb_classif_dropout_site(handle, 0, 0, None, C.byref(seed)) != 0
    assert lib.kmb_classif_dropout_site(handle, 0, 0, C.byref(thr), None) != 0
    assert lib.kmb_classif_dropout_site(None, 0, 0, C.byref(thr), C.byref(seed)) != 0
    assert b"kmb_classif_dropout_site" in lib.kmb_last_error()


def test_a_model_without_heads_takes_the_setting_and_reports_zeros(lib):
    h = C.c_void_p()
    check(lib.kmb_create(C.byref(KmbConfig(**VCG_BASE)), C.byref(h)))
    try:
        check(lib.kmb_set_classif_dropout(h, 0.1))
        thr, seed = C.c_uint32(7), C.c_uint32(7)
        check(lib.kmb_classif_dropout_site(h, 2, 1, C.byref(thr), C.byref(seed)))
        assert (thr.value, seed.value) == (0, 0)
    finally:
        lib.kmb_destroy(h)


def _route(lib, p, forced=0):
    out = (C.c_int32 * 128)()
    n = lib.kmb_debug_gemm_route(C.byref(p), forced, out, len(out))
    assert n >= 4 and (n - 1) % 3 == 0, (forced, n)
    return list(out[:n])


# kernels whose epilogue is gemm_epilogue_body's run-time path for these launches (its dropout block follows the activation and precedes the
# residual): the 128 x 128 kernels 1, 5, 7 and the 256 x 256 kernel 8
GENERAL_EPILOGUE = {1, 5, 7, 8}


def test_tanh_backward_with_dropout_has_a_route(lib):
    """out_proj's data gradient: dlogits [203, 1608] W_o [1608, 768] times 1 - aux^2, then the hidden site's mask; K = 1608 is no multiple
    of 64, which the register-staged kernel (variant 1) takes"""
    for K in (1608, 136):
        plain = problem(203, 768, K, "dgrad", act=4, bias=False, aux=AUX, ld_aux=768)
        drop = problem(203, 768, K, "dgrad", act=4, bias=False, aux=AUX, ld_aux=768, **DROP)
        r = _route(lib, drop)
        assert r == _route(lib, plain), K
        assert r[0] == 0 and r[2] == 1, (K, r)


@pytest.mark.parametrize("N", [768, 1536])
def test_dense_data_gradient_with_dropout_has_a_route(lib, N):
    """dense's data gradient: d_pre [203, 768] W_d [768, N] with the input site's mask and no residual (N = 1536: the relation head)"""
    plain = problem(203, N, 768, "dgrad", bias=False)
    drop = problem(203, N, 768, "dgrad", bias=False, **DROP)
    r = _route(lib, drop)
    assert r == _route(lib, plain)                       # the tuner's key does not hold the mask: both launches share one choice
    assert set(r[2::3]) <= GENERAL_EPILOGUE, r           # ... among kernels that all carry it
    for forced in range(1, 17):                          # and whatever KMB_GEMM_VARIANT asks for ends on one of them
        f = _route(lib, drop, forced)
        assert f[0] == 0 and f[2] in GENERAL_EPILOGUE, (forced, f)
