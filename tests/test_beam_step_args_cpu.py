"""CPU: the launch-side argument logic of the fused beam steps (csrc/beam_step.hip: the shape check the three launchers share and
each launcher's own conditions), through the C ABI.  Every call here is one the library answers before any launch -- a refusal, or
B == 0 -- so no device is needed; the pointers are real, 16-byte aligned host addresses that nothing dereferences."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    from kmbart import _lib
    __graft_entry__.build()
    return _lib.load()


_HOST = (C.c_char * 4096)()
_BASE = (C.addressof(_HOST) + 15) & ~15


def _p(i, off=0):
    """Host address number i (256 bytes apart), 16-byte aligned before `off`."""
    return C.c_void_p(_BASE + 256 * i + off)


def _err(lib):
    return lib.kmb_last_error().decode()


def _beam_step(lib, **over):
    a = dict(logits=_p(0), ld=64, V=64, B=2, num_beams=2, add=_p(1), force_token=-1, ban_token=-1, k=4, out=_p(2), eos_token=2,
             next_scores=_p(3), next_tokens=_p(4), next_beam_idx=_p(5), scratch=_p(6),
             scratch_floats=lib.kmb_logsoftmax_topk_scratch(4), scratch_short=0)
    a.update(over)
    a["scratch_floats"] -= a["scratch_short"]
    return lib.kmb_beam_step(a["logits"], a["ld"], a["V"], a["B"], a["num_beams"], a["add"], a["force_token"], a["ban_token"], a["k"],
                             a["out"], a["eos_token"], a["next_scores"], a["next_tokens"], a["next_beam_idx"], a["scratch"],
                             a["scratch_floats"], None)


def _beam_step_stats(lib, **over):
    a = dict(logits=_p(0), ld=512, V=512, B=2, num_beams=2, add=_p(1), force_token=-1, ban_token=-1, k=4, out=_p(2), eos_token=2,
             next_scores=_p(3), next_tokens=_p(4), next_beam_idx=_p(5), stats=_p(6), stats_blocks=2)
    a.update(over)
    return lib.kmb_beam_step_stats(a["logits"], a["ld"], a["V"], a["B"], a["num_beams"], a["add"], a["force_token"], a["ban_token"],
                                   a["k"], a["out"], a["eos_token"], a["next_scores"], a["next_tokens"], a["next_beam_idx"], a["stats"],
                                   a["stats_blocks"], None)


BEAM_STEP_REFUSED = [
    dict(k=0), dict(k=17), dict(num_beams=0), dict(num_beams=17), dict(ld=66), dict(logits=_p(0, 4)),
    dict(scratch_short=1),        # one float less than kmb_logsoftmax_topk_scratch(B * num_beams)
    dict(ld=53252),               # one float4 chunk per part more than the part kernel holds (4 parts x 13 x 256 chunks)
    dict(B=32768),                # 65536 rows: past the launch grid's second dimension
]


@pytest.mark.parametrize("over", BEAM_STEP_REFUSED, ids=lambda o: "-".join("%s" % k for k in o))
def test_beam_step_refuses_the_shape(lib, over):
    assert _beam_step(lib, **over) != 0
    assert _err(lib).startswith("kmb_beam_step: unsupported shape"), _err(lib)


def test_beam_step_missing_arguments_and_empty_batch(lib):
    assert _beam_step(lib, next_tokens=None) != 0
    assert _err(lib).startswith("kmb_beam_step: missing output"), _err(lib)
    assert _beam_step(lib, logits=None) != 0
    assert _err(lib).startswith("kmb_beam_step: missing tensor"), _err(lib)
    assert _beam_step(lib, B=0) == 0


BEAM_STEP_STATS_REFUSED = [
    dict(stats_blocks=0), dict(stats_blocks=3), dict(V=510), dict(ld=508), dict(B=107, num_beams=3),   # 321 rows
    dict(k=17), dict(num_beams=17), dict(logits=_p(0, 4)), dict(V=65540, ld=65540, stats_blocks=257),
]


@pytest.mark.parametrize("over", BEAM_STEP_STATS_REFUSED, ids=lambda o: "-".join("%s" % k for k in o))
def test_beam_step_stats_refuses_the_shape(lib, over):
    assert _beam_step_stats(lib, **over) != 0
    assert _err(lib).startswith("kmb_beam_step_stats: unsupported shape"), _err(lib)


def test_beam_step_stats_empty_batch(lib):
    assert _beam_step_stats(lib, B=0) == 0


def test_scratch_sizes(lib):
    for rows in (0, -3):
        assert lib.kmb_logsoftmax_topk_scratch(rows) == 0
        assert lib.kmb_beam_step_processed_scratch(rows, 12, 2) == 0
    assert lib.kmb_logsoftmax_topk_scratch(1) > 0
    assert lib.kmb_logsoftmax_topk_scratch(7) == 7 * lib.kmb_logsoftmax_topk_scratch(1)
