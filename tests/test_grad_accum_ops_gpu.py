"""GPU: the gradient-accumulation fold on raw pointers (kmb_op_grad_fold): dst = (add ? dst : 0) + src.

One correctly rounded fp32 add per element, so every comparison is bit for bit against torch's fp32 `dst + src` (or `src`).
Element counts: 1, 7, 8 (the scalar edges alone, fewer than / exactly two vectors), 4099 (vectors plus a tail), 3 * 2^20 + 1 (every
workgroup of one turn busy) and 2048 * 4096 + 4 + 3 (one vector more than the capped grid of 2048 workgroups covers in a turn of four
vectors per thread: the grid-stride loop's second turn, three of its four loads out of range).  Both pointers sit at 0 or 1 float
from a 16-byte boundary, independently: the aligned vector body, the scalar head, and the element-wise source reads when the two
phases differ."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from kmbart import _lib  # noqa: E402
from kmbart._lib import check, ptr  # noqa: E402
from gpu_util import DEV, stream  # noqa: E402

COUNTS = [1, 7, 8, 4099, 3 * 2 ** 20 + 1, 2048 * 4096 + 4 + 3]
GUARD = 8           # floats on either side of the range that must stay as they were
SENTINEL = -12345.5


def fold(dst, src, n, add):
    check(_lib.load().kmb_op_grad_fold(ptr(dst), ptr(src), n, 1 if add else 0, stream()))


def buffers(n, dst_off, src_off, seed):
    """(whole dst buffer, dst range view, src range view): the ranges start dst_off / src_off floats behind a 16-byte boundary and
    have GUARD sentinel floats in front and behind"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    dbuf = torch.full((n + 2 * GUARD + 4,), SENTINEL, dtype=torch.float32, device=DEV)
    sbuf = torch.full((n + 2 * GUARD + 4,), SENTINEL, dtype=torch.float32, device=DEV)
    assert dbuf.data_ptr() % 16 == 0 and sbuf.data_ptr() % 16 == 0
    d = dbuf[GUARD + dst_off: GUARD + dst_off + n]
    s = sbuf[GUARD + src_off: GUARD + src_off + n]
    assert d.data_ptr() % 16 == 4 * dst_off and s.data_ptr() % 16 == 4 * src_off
    d.copy_(torch.randn(n, generator=g).to(DEV))
    s.copy_((torch.randn(n, generator=g) * 3.0).to(DEV))
    return dbuf, d, s


def bits(t):
    return t.contiguous().view(torch.int32)


def guards_untouched(dbuf, dst_off, n):
    lo, hi = GUARD + dst_off, GUARD + dst_off + n
    return bool((dbuf[:lo] == SENTINEL).all()) and bool((dbuf[hi:] == SENTINEL).all())


@pytest.mark.parametrize("src_off", [0, 1])
@pytest.mark.parametrize("dst_off", [0, 1])
@pytest.mark.parametrize("n", COUNTS)
def test_fold_is_one_rounded_add_and_stays_inside_its_range(n, dst_off, src_off):
    for add in (True, False):
        dbuf, d, s = buffers(n, dst_off, src_off, seed=n % 1000 + 10 * dst_off + src_off)
        want = (d + s) if add else s.clone()
        src_before = s.clone()
        fold(d, s, n, add)
        torch.cuda.synchronize()
        assert torch.equal(bits(d), bits(want)), (n, dst_off, src_off, add, int((bits(d) != bits(want)).sum()))
        assert guards_untouched(dbuf, dst_off, n), (n, dst_off, src_off, add)
        assert torch.equal(bits(s), bits(src_before))


@pytest.mark.parametrize("dst_off,src_off", [(0, 0), (1, 0), (1, 1)])
@pytest.mark.parametrize("n", [7, 4099])
def test_overwrite_never_reads_the_destination(n, dst_off, src_off):
    """dst full of NaN (a skipped step, a poisoned arena): the overwrite form gives exactly src"""
    dbuf, d, s = buffers(n, dst_off, src_off, seed=3)
    d.fill_(float("nan"))
    fold(d, s, n, add=False)
    torch.cuda.synchronize()
    assert torch.equal(bits(d), bits(s))
    assert guards_untouched(dbuf, dst_off, n)


@pytest.mark.parametrize("add", [True, False])
@pytest.mark.parametrize("dst_off,src_off", [(0, 0), (0, 1)])
def test_nan_and_inf_in_the_source_arrive(add, dst_off, src_off):
    """skip_nonfinite sees a non-finite micro-batch only if the fold hands it on: one NaN and one Inf in the vector body, one Inf in
    the scalar tail"""
    n = 4099
    _, d, s = buffers(n, dst_off, src_off, seed=4)
    s[17] = float("nan")
    s[2050] = float("inf")
    s[n - 1] = float("-inf")
    want = (d + s) if add else s.clone()
    fold(d, s, n, add)
    torch.cuda.synchronize()
    assert bool(torch.isnan(d[17])) and float(d[2050]) == float("inf") and float(d[n - 1]) == float("-inf")
    finite = torch.isfinite(want)
    assert int((~finite).sum()) == 3 and torch.equal(bits(d)[finite], bits(want)[finite])


def test_bad_arguments_are_refused():
    lib = _lib.load()
    x = torch.zeros(64, dtype=torch.float32, device=DEV)
    y = torch.zeros(64, dtype=torch.float32, device=DEV)
    assert lib.kmb_op_grad_fold(ptr(x), ptr(y), 0, 1, stream()) != 0
    assert lib.kmb_op_grad_fold(None, ptr(y), 8, 1, stream()) != 0
    assert lib.kmb_op_grad_fold(ptr(x), ptr(x[4:]), 8, 1, stream()) != 0 and b"overlap" in lib.kmb_last_error()
    assert lib.kmb_op_grad_fold(ptr(x), ptr(x[8:]), 8, 1, stream()) == 0
    torch.cuda.synchronize()
