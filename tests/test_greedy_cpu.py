"""No GPU: the greedy entries of the built library and their declarations, and how generate() routes one-beam decoding."""
import ctypes as C
import itertools
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_greedy_entries_are_exported_and_declared():
    from kmbart import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "kmbart.h")).read()
    for name in ("kmb_greedy_step", "kmb_gen_greedy_step"):
        assert getattr(lib, name) is not None
        assert name in _lib.PROTOTYPES
        assert re.search(r"^int %s\(" % name, header, re.M), name
    # one argtype per declared parameter
    for name in ("kmb_greedy_step", "kmb_gen_greedy_step"):
        decl = re.search(r"^int %s\((.*?)\);" % name, header, re.M | re.S).group(1)
        assert len(decl.split(",")) == len(_lib.PROTOTYPES[name][1]), name


def test_one_beam_routing_truth_table():
    from src.model.model import _decode_route, _one_beam_on_device
    for do_sample, processors_on, fp32 in itertools.product((False, True), repeat=3):
        for flag in (True, False, 0, None):
            want = (not do_sample) and (not processors_on) and (not fp32) and flag is True
            got = _one_beam_on_device(do_sample, processors_on, fp32, flag)
            assert got is want, (do_sample, processors_on, fp32, flag)
    assert _one_beam_on_device(False, False, False, 1) is True      # any truthy value
    # the route names are unchanged: greedy without beams is still "one_beam", with or without processors / fp32
    for processors_on, fp32, dev in itertools.product((False, True), (False, True), (True, False, None)):
        assert _decode_route(1, False, processors_on, fp32, dev, False, 50265) == "one_beam"
    assert _decode_route(1, True, False, False, True, False, 50265) == "device_sampling"
