"""CPU: the host side of attention dropout -- a run-time setting of the handle (kmb_set_attention_dropout), not a field of the
creation struct, which keeps refusing it; the query entry before any forward; and the KmbAttn layout of the ctypes binding
against the library's own (three fields were appended for the DROP kernel instantiations)."""
import ctypes as C
import math

import pytest

from kmbart import _lib
from kmbart._lib import KmbConfig, check

VCG_BASE = dict(vocab_size=50320, d_model=768, encoder_layers=6, decoder_layers=6, encoder_attention_heads=12,
                decoder_attention_heads=12, encoder_ffn_dim=3072, decoder_ffn_dim=3072, max_position_embeddings=1024,
                extra_pos_embeddings=2, image_feature_size=2052, pad_token_id=1, bos_token_id=0, eos_token_id=2,
                img_feat_id=50273, cls_token_id=50276, scale_embedding=0, dropout=0.1, attention_dropout=0.0,
                activation_dropout=0.0, layer_norm_eps=1e-5)


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


def test_setter_takes_probabilities_in_the_half_open_unit_interval(lib, handle):
    assert lib.kmb_set_attention_dropout(handle, 0.1) == 0
    assert lib.kmb_set_attention_dropout(handle, 0.0) == 0
    assert lib.kmb_set_attention_dropout(handle, 0.999) == 0
    for bad in (-0.1, 1.0, 1.5, math.nan, math.inf):
        assert lib.kmb_set_attention_dropout(handle, bad) != 0, bad
        assert b"kmb_set_attention_dropout" in lib.kmb_last_error(), bad


def test_site_query_before_any_forward_returns_zeros(lib, handle):
    check(lib.kmb_set_attention_dropout(handle, 0.1))
    for kind, layers in ((0, 6), (1, 6), (2, 6)):
        for layer in range(layers):
            thr, seed = C.c_uint32(7), C.c_uint32(7)
            check(lib.kmb_attention_dropout_site(handle, kind, layer, C.byref(thr), C.byref(seed)))
            assert (thr.value, seed.value) == (0, 0), (kind, layer)
    thr, seed = C.c_uint32(7), C.c_uint32(7)
    for kind, layer in ((3, 0), (-1, 0), (0, 6), (1, -1), (2, 6)):
        assert lib.kmb_attention_dropout_site(handle, kind, layer, C.byref(thr), C.byref(seed)) != 0, (kind, layer)
        assert b"kmb_attention_dropout_site" in lib.kmb_last_error()
    assert lib.kmb_attention_dropout_site(handle, 0, 0, None, C.byref(seed)) != 0


def test_creation_struct_still_refuses_attention_and_activation_dropout(lib):
    h = C.c_void_p()
    for bad in (dict(attention_dropout=0.1), dict(activation_dropout=0.1)):
        assert lib.kmb_create(C.byref(KmbConfig(**dict(VCG_BASE, **bad))), C.byref(h)) != 0, bad
        assert b"attention_dropout / activation_dropout != 0 are not implemented" in lib.kmb_last_error()


def test_kmbattn_layout_matches_the_library(lib):
    """sizeof as the library was compiled, and the appended fields at the end in the header's order."""
    A = _lib.KmbAttn
    assert C.sizeof(A) == lib.kmb_abi_sizeof_attn()
    names = [f[0] for f in A._fields_]
    assert names[-3:] == ["drop_thr16", "drop_seed", "drop_scale"]
    assert A.drop_thr16.offset == A.ld_colsum.offset + 4          # straight behind the last old field
    assert (A.drop_seed.offset, A.drop_scale.offset) == (A.drop_thr16.offset + 4, A.drop_thr16.offset + 8)
    a = A()
    assert (a.drop_thr16, a.drop_seed, a.drop_scale) == (0, 0, 0.0)   # a zero-constructed struct runs without dropout
