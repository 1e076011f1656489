"""CPU: the host side of beam search with score processors on the device (model._device_beam_processors) -- the two C-ABI
symbols, the routing predicate with each of its exclusions, the unchanged routing functions, the step reference
(tests/beam_process_ref.py) against the host beam loop's arithmetic, and the CLI flag."""
import itertools
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_process_ref  # noqa: E402
from src.model.model import (_beam_processors_on_device, _decode_route, _one_beam_on_device, _pack_bad_words,  # noqa: E402
                             _postprocess_next_token_scores, _processors_on_device)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOS, EOS, START = 0, 2, 2


def test_symbols_are_declared_and_exported():
    import __graft_entry__
    from kmbart import _lib
    __graft_entry__.build()
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "kmbart.h")).read()
    declared = set(re.findall(r"\b(kmb_[a-z0-9_]+)\s*\(", header))
    for name in ("kmb_beam_step_processed", "kmb_gen_beam_step_processed", "kmb_beam_step_processed_scratch"):
        assert name in declared and name in _lib.PROTOTYPES and hasattr(lib, name), name
    # the size query: the part records of kmb_logsoftmax_topk_scratch plus 2 t + n_bad list words per row
    assert lib.kmb_beam_step_processed_scratch(320, 12, 2) == lib.kmb_logsoftmax_topk_scratch(320) + 320 * (2 * 12 + 2)
    assert lib.kmb_beam_step_processed_scratch(0, 12, 2) == 0
    # bad arguments fail with a message before anything touches a device
    assert lib.kmb_beam_step_processed(None, 8, 8, 1, 2, None, -1, -1, 4, None, -1, None, None, None, None, 0, None, None, 4, 1, 1.0,
                                       0, None, None, 0, None) != 0
    assert lib.kmb_last_error().decode().startswith("kmb_beam_step_processed: ")


def _on(**over):
    kw = dict(num_beams=5, do_sample=False, processors_on=True, fp32=False, device_beam_processors=True, max_length=20,
              table=([], [0]), V=50320, ld=50432, no_repeat_ngram_size=3, bad_words_ids=None, bos_token_id=BOS, eos_token_id=EOS,
              decoder_start_token_id=7)
    kw.update(over)
    return _beam_processors_on_device(**kw)


def test_beam_processors_on_device_truth_table():
    assert _on() is True
    assert _on(no_repeat_ngram_size=0) is True and _on(no_repeat_ngram_size=2) is True
    assert _on(max_length=1024) is True and _on(max_length=1025) is False
    assert _on(num_beams=2) is True and _on(num_beams=8) is True
    for falsy in (False, 0, None):
        assert _on(device_beam_processors=falsy) is False
    for truthy in (True, 1, "yes"):
        assert _on(device_beam_processors=truthy) is True
    # each exclusion on its own
    for over in (dict(processors_on=False), dict(num_beams=1), dict(do_sample=True), dict(fp32=True), dict(table=None),
                 dict(num_beams=9), dict(V=65537), dict(ld=50430),                       # the fused step's shape limits
                 dict(no_repeat_ngram_size=1),                                           # bans the start token: BOS may be it
                 dict(bad_words_ids=[[5], [9, BOS]]), dict(bad_words_ids=[[EOS]]),       # a bad word ending in a forced token
                 dict(decoder_start_token_id=EOS)):                                      # an n-gram can close on EOS
        assert _on(**over) is False, over
    # what only looks like one of them
    assert _on(bad_words_ids=[[BOS, 5], [EOS, 9]]) is True                                # forced tokens in a head
    assert _on(bad_words_ids=[[EOS]], eos_token_id=None) is True and _on(decoder_start_token_id=EOS, eos_token_id=None) is True
    assert _on(decoder_start_token_id=BOS) is True
    # every combination of the plain switches: True exactly under the conjunction
    for nb, ds, po, fp, sw, ml, tb, n in itertools.product((1, 3, 9), (False, True), (False, True), (False, True), (False, True),
                                                           (12, 2000), (None, ([1], [0, 1])), (0, 1, 3)):
        want = po and sw and nb == 3 and not ds and not fp and ml <= 1024 and tb is not None and n != 1
        assert _on(num_beams=nb, do_sample=ds, processors_on=po, fp32=fp, device_beam_processors=sw, max_length=ml, table=tb,
                   no_repeat_ngram_size=n) is bool(want)


def test_the_routing_functions_are_unchanged():
    """_decode_route on the grid and the table of tests/test_generate_route_cpu.py, _processors_on_device and
    _one_beam_on_device on the inputs of tests/test_logits_process_cpu.py; generate() hands them processors_on and not (either
    device path)."""
    import test_generate_route_cpu as T
    T.test_route_equals_the_inline_conditions_over_the_grid()
    T.test_route_table()
    assert _processors_on_device(1, False, True, False, True, True, True, 20, ([], [0])) is True
    assert _processors_on_device(3, False, True, False, True, True, True, 20, ([], [0])) is False     # beams: the other switch
    assert _one_beam_on_device(False, False, False, True) is True and _one_beam_on_device(False, True, False, True) is False
    assert _one_beam_on_device(True, False, False, True) is False and _one_beam_on_device(False, False, True, True) is False
    from src.model import MultiModalBartForConditionalGeneration
    assert not hasattr(MultiModalBartForConditionalGeneration, "_device_beam_processors")
    on = _on()
    assert _decode_route(5, False, True and not on, False, True, False, 50320) == "pipelined_beams"
    off = _on(device_beam_processors=False)
    assert _decode_route(5, False, True and not off, False, True, False, 50320) == "host_beams"


def _host_step(logits, rows, add, B, nb, V, k, t, min_length, eos, p, n, bad):
    """The greedy-beam branch of _host_beam_loop: torch.log_softmax + _postprocess_next_token_scores + torch.topk."""
    sc = torch.log_softmax(torch.from_numpy(logits[:, :V]).float(), dim=-1)
    _postprocess_next_token_scores(sc, rows, t, min_length, eos, p, n, bad)
    sc = sc + torch.from_numpy(add)[:, None]
    ns, nt = torch.topk(sc.view(B, nb * V), k, dim=1, largest=True, sorted=True)
    return sc.numpy(), ns.numpy(), nt.numpy()


@pytest.mark.parametrize("name,p,n,bad", [("penalty", 1.3, 0, None), ("ngram", 1.0, 2, None), ("bad_words", 1.0, 0, "draw"),
                                          ("combined", 1.3, 3, "draw")])
def test_step_reference_equals_the_host_loop(name, p, n, bad):
    B, nb, V, ld, t, k = 3, 3, 97, 100, 7, 6
    rng = np.random.default_rng(5)
    logits = (rng.standard_normal((B * nb, ld)) * 4).astype(np.float32)
    top = np.argsort(-logits[:, :V], axis=1)[:, :4]
    rows = [[int(top[r, j % 4]) for j in range(t)] for r in range(B * nb)]      # the histories cycle through the rows' best tokens
    add = (-rng.random(B * nb) * 3).astype(np.float32)
    if bad == "draw":
        bad = [[int(top[0, 0])], [rows[1][-1], int(top[1, 1])]]                  # one bare token, one whose head row 1 ends with
    ref = beam_process_ref.step(logits, rows, add, B, nb, V, k, p, n, bad, ban_token=EOS, eos=EOS)
    sc, ns, nt = _host_step(logits, rows, add, B, nb, V, k, t, t + 1, EOS, p, n, bad)
    # float64 against fp32 log_softmax: a few ulp of values of magnitude <= 64, scaled by the penalty
    tol = 64 * 2.0 ** -23 * p
    assert np.array_equal(np.isinf(ref["s"]), np.isinf(sc))
    fin = np.isfinite(sc)
    assert np.abs(ref["s"][fin] - sc[fin]).max() <= tol
    assert np.abs(ref["val"][:, :k] - ns).max() <= tol
    gap = (ref["val"][:, :-1] - ref["val"][:, 1:]).min(axis=1)
    assert (gap > 2 * tol).all(), gap                                          # the order is decided: the ids must be equal
    assert np.array_equal(ref["idx"][:, :k], nt)
    edited = np.isinf(ref["s"]).sum() - B * nb                                  # beyond the EOS ban
    assert (edited > 0) == (n > 0 or bad is not None)
    if p != 1.0:   # the winners are penalised tokens: the edit decides the order
        assert any(int(i) % V in rows[b * nb + int(i) // V] for b in range(B) for i in ref["idx"][b, :k])
    # the bookkeeping's next beams
    for i, (tok, src) in enumerate(zip(ref["next_tokens"], ref["next_beam_idx"])):
        assert tok != EOS and ref["ids_out"][i] == rows[src] + [int(tok)]


def test_forced_step_of_the_reference():
    B, nb, V, k = 2, 2, 31, 4
    rng = np.random.default_rng(6)
    logits = (rng.standard_normal((B * nb, V)) * 4).astype(np.float32)
    rows = [[START, BOS, 5]] * (B * nb)
    add = np.array([0.0, -1.5, -0.25, -0.5], dtype=np.float32)
    ref = beam_process_ref.step(logits, rows, add, B, nb, V, k, 1.3, 2, None, force_token=9, eos=EOS)
    assert ref["next_tokens"].tolist() == [9] * 4 and ref["next_scores"].tolist() == [0.0, -1.5, -0.25, -0.5]
    assert ref["next_beam_idx"].tolist() == [0, 1, 2, 3]


def test_vcg_generate_flag():
    import vcg_generate
    base = ["--output_file", "o.json", "--checkpoint", "ck", "--synthetic", "1"]
    assert vcg_generate.parse_args(base).device_beam_processors is False
    a = vcg_generate.parse_args(base + ["--num_beams", "5", "--no_repeat_ngram_size", "3", "--device_beam_processors"])
    assert a.device_beam_processors is True and a.device_processors is False
    assert _pack_bad_words(None, 50) == ([], [0])
