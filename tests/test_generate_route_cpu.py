"""CPU: generate()'s choice of decode loop and its forced-token rule, against the conditions the loops were chosen by before they
were split into methods (src/model/model.py: _decode_route, _forced_tokens)."""
import itertools

from src.model.model import _decode_route, _forced_tokens


def _route_as_written(num_beams, do_sample, processors_on, fp32, device_sampling, has_sampler, V):
    """The routing as generate() spelled it inline: the device-sampling test, then num_beams == 1, then the pipelined / host beam
    loops."""
    if num_beams == 1 and do_sample and not processors_on and not fp32 and device_sampling:
        return "device_sampling"
    if num_beams == 1:
        return "one_beam"
    device_beam_sampling = (do_sample and not processors_on and not fp32 and not has_sampler and device_sampling
                            and 2 * num_beams <= 16 and V <= 65536)
    host_loop = (do_sample and not device_beam_sampling) or processors_on or fp32
    return "host_beams" if host_loop else "pipelined_beams"


def test_route_equals_the_inline_conditions_over_the_grid():
    grid = itertools.product((1, 2, 5, 8, 9, 16), (False, True), (False, True), (False, True), (True, False, 0, None, 1),
                             (False, True), (1000, 50265, 65536, 65537))
    n = 0
    for args in grid:
        assert _decode_route(*args) == _route_as_written(*args), args
        n += 1
    assert n == 6 * 2 * 2 * 2 * 5 * 2 * 4


def test_route_table():
    V = 50265
    # one beam: the device loop unless post-processors, fp32 or a falsy _device_sampling; _sampler plays no part
    assert _decode_route(1, True, False, False, True, True, V) == "device_sampling"
    assert _decode_route(1, True, False, False, 0, False, V) == "one_beam"
    assert _decode_route(1, True, True, False, True, False, V) == "one_beam"
    assert _decode_route(1, False, False, False, True, False, V) == "one_beam"
    # beams: greedy pipelined; device beam sampling within 2 * num_beams <= 16 and V <= 65536, without a custom sampler
    assert _decode_route(5, False, False, False, None, True, 70000) == "pipelined_beams"
    assert _decode_route(5, True, False, False, True, False, V) == "pipelined_beams"
    assert _decode_route(8, True, False, False, True, False, 65536) == "pipelined_beams"
    assert _decode_route(9, True, False, False, True, False, V) == "host_beams"
    assert _decode_route(5, True, False, False, True, False, 65537) == "host_beams"
    assert _decode_route(5, True, False, False, True, True, V) == "host_beams"
    assert _decode_route(5, True, False, False, False, False, V) == "host_beams"
    # fp32 mode and the score post-processors: always a host loop
    assert _decode_route(5, False, True, False, True, False, V) == "host_beams"
    assert _decode_route(5, False, False, True, True, False, V) == "host_beams"


def test_forced_tokens():
    bos, eos = 0, 2
    assert _forced_tokens(1, 20, bos, eos) == [bos]
    assert _forced_tokens(19, 20, bos, eos) == [eos]
    assert _forced_tokens(19, 20, bos, None) == []
    assert all(_forced_tokens(t, 20, bos, eos) == [] for t in range(2, 19))
    # max_length 2: the first step is also the last -- BOS, then EOS, in the reference's order
    assert _forced_tokens(1, 2, bos, eos) == [bos, eos]
    assert _forced_tokens(1, 2, bos, None) == [bos]
