"""CPU: the host side of the score processors on the device (model._device_processors) -- the routing predicate, the bad-word
packer, the kernel's rule (tests/process_ref.py) against _postprocess_next_token_scores on seeded cases, and the CLI plumbing."""
import itertools
import os
import random
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import process_ref  # noqa: E402
from src.data.synthetic import make_batch  # noqa: E402
from src.model.model import (_decode_route, _one_beam_on_device, _pack_bad_words, _postprocess_next_token_scores,  # noqa: E402
                             _processors_on_device)

INF = float("inf")


def _on(**over):
    kw = dict(num_beams=1, do_sample=False, processors_on=True, fp32=False, device_processors=True, device_greedy=True,
              device_sampling=True, max_length=20, table=([], [0]))
    kw.update(over)
    return _processors_on_device(**kw)


def test_processors_on_device_truth_table():
    assert _on() is True and _on(do_sample=True) is True
    assert _on(max_length=1024) is True and _on(max_length=1025) is False
    for over in (dict(processors_on=False), dict(num_beams=2), dict(num_beams=5, do_sample=True), dict(fp32=True), dict(table=None)):
        assert _on(**over) is False, over
    for falsy in (False, 0, None):
        assert _on(device_processors=falsy) is False
        assert _on(device_greedy=falsy) is False and _on(do_sample=True, device_sampling=falsy) is False
        # the switch of the OTHER one-beam loop does not matter
        assert _on(device_sampling=falsy) is True and _on(do_sample=True, device_greedy=falsy) is True
    for truthy in (True, 1, "yes"):
        assert _on(device_processors=truthy) is True
    # every combination: True exactly under the conjunction
    for nb, ds, po, fp, dp, dg, dsm, ml, tb in itertools.product((1, 3), (False, True), (False, True), (False, True), (False, True),
                                                                 (False, True), (False, True), (12, 2000), (None, ([1], [0, 1]))):
        want = po and dp and nb == 1 and not fp and (dsm if ds else dg) and ml <= 1024 and tb is not None
        assert _processors_on_device(nb, ds, po, fp, dp, dg, dsm, ml, tb) is bool(want)


def test_generate_reads_the_switch_as_absent_by_default_and_routes_are_unchanged():
    """What generate() hands the unchanged routing functions: processors_on and not on_device."""
    from src.model import MultiModalBartForConditionalGeneration
    assert not hasattr(MultiModalBartForConditionalGeneration, "_device_processors")
    for ds in (False, True):
        on = _on(do_sample=ds)
        assert _decode_route(1, ds, True and not on, False, True, False, 100) == ("device_sampling" if ds else "one_beam")
        assert _one_beam_on_device(ds, True and not on, False, True) is (not ds)
        off = _on(do_sample=ds, device_processors=False)
        assert _decode_route(1, ds, True and not off, False, True, False, 100) == "one_beam"
        assert _one_beam_on_device(ds, True and not off, False, True) is False


def test_packer_three_outcomes():
    assert _pack_bad_words(None, 50) == ([], [0])
    assert _pack_bad_words([[40], [29, 49], [0, 1, 2]], 50) == ([40, 29, 49, 0, 1, 2], [0, 1, 3, 6])
    with pytest.raises(AssertionError, match="cannot have an empty list"):
        _pack_bad_words([[3], []], 50)
    assert _pack_bad_words([[50]], 50) is None and _pack_bad_words([[3, -1]], 50) is None and _pack_bad_words([[50, 3]], 50) is None
    assert _pack_bad_words([[1]] * 4096, 50) is not None and _pack_bad_words([[1]] * 4097, 50) is None
    assert _pack_bad_words([[1] * 1024], 50) is not None and _pack_bad_words([[1] * 1025], 50) is None


def _host_banned(rows, t, n, bad, V):
    sc = torch.zeros(len(rows), V)
    _postprocess_next_token_scores(sc, rows, t, 0, None, 1.0, n, bad)
    return [set(torch.nonzero(sc[r] == -INF).flatten().tolist()) for r in range(len(rows))]


def _cases():
    rnd = random.Random(7)
    tables = [None, [[3]], [[2, 4], [5]], [[1, 2, 3], [4, 4], [6], [0, 1, 2, 3, 4, 5]]]
    for i in range(300):
        R, V, t = rnd.randint(1, 5), rnd.randint(7, 33), rnd.randint(1, 12)
        n = rnd.randint(0, 4)
        small = rnd.random() < 0.5                      # a small alphabet makes repeats, n-gram hits and tail matches common
        rows = [[rnd.randrange(4 if small else V) for _ in range(t)] for _ in range(R)]
        yield R, V, t, n, tables[i % 4], (1.0, 1.3, 2.0, 200.0)[(i // 4) % 4], rows
    # the edges by name: n == 1, t + 1 == n, n > t + 1, a head longer than t, a head longer than R
    yield 2, 9, 3, 1, None, 1.3, [[1, 2, 1], [4, 4, 4]]
    yield 1, 9, 3, 4, None, 1.0, [[1, 2, 3]]
    yield 1, 9, 3, 3, None, 1.0, [[2, 2, 2]]
    yield 1, 9, 2, 4, None, 2.0, [[1, 1]]
    yield 3, 9, 2, 0, [[1, 2, 3, 4]], 1.0, [[2, 3], [1, 2], [2, 3]]
    yield 1, 9, 3, 0, [[2, 3, 4]], 1.0, [[1, 2, 3]]            # head (2 tokens) matches the tail but is longer than R = 1
    yield 2, 9, 3, 0, [[2, 3, 4]], 1.0, [[1, 2, 3], [2, 3, 2]]  # ... banned in row 0 at R = 2


def test_rule_matches_postprocess_next_token_scores():
    g = torch.Generator().manual_seed(11)
    hits = dict(ngram=0, bad_head=0, long_head=0, pen=0)
    for R, V, t, n, bad, p, rows in _cases():
        want = _host_banned(rows, t, n, bad, V)
        got = [process_ref.banned(process_ref.kept(row, V), R, n, bad, V) for row in rows]
        assert got == want, (R, V, t, n, bad, rows)
        hits["ngram"] += n > 0 and any(want)
        hits["bad_head"] += bool(bad) and any(len(s) > 1 and s[-1] in w for s in bad for w in want)
        hits["long_head"] += bool(bad) and any(len(s) - 1 > R or len(s) - 1 > t for s in bad)
        # the whole edit on random logits with signed zeros and infinities
        x = torch.randn(R, V + 3, generator=g) * 3
        x[0, 0], x[0, 1], x[0, 2], x[0, 3] = 0.0, -0.0, INF, -INF
        ref = x.clone()
        _postprocess_next_token_scores(ref[:, :V], rows, t, 0, None, p, n, bad)
        mine = torch.from_numpy(process_ref.process(x.clone().numpy(), rows, V, p, n, bad))
        assert torch.equal(mine[:, V:], x[:, V:])
        assert torch.equal(mine == -INF, ref == -INF)
        a, b = mine.numpy(), ref.numpy()
        if p in (1.0, 2.0):
            assert np.array_equal(a.view(np.int32), b.view(np.int32)), (p, rows)
        else:
            one_ulp = (a == b) | (a == np.nextafter(b, np.float32(INF))) | (a == np.nextafter(b, np.float32(-INF)))
            assert one_ulp.all(), (p, rows)
        untouched = torch.ones(R, V + 3, dtype=torch.bool)
        for r, row in enumerate(rows):
            untouched[r, list(set(row) | want[r])] = False
        assert np.array_equal(a.view(np.int32)[untouched.numpy()], x.numpy().view(np.int32)[untouched.numpy()])
        hits["pen"] += p != 1.0 and not np.array_equal(a.view(np.int32), x.numpy().view(np.int32))
    assert all(v >= 3 for v in hits.values()), hits   # the cases reach what they are there for


def test_first_occurrence_and_out_of_range_tokens():
    assert process_ref.penalised([5, 5, 5, 5]) == [5]
    assert process_ref.penalised([3, 1, 3, 2, 1]) == [3, 1, 2]
    assert process_ref.kept([3, 50, -1, 4, 1 << 40], 50) == [3, 4]
    x = np.array([[4.0, -4.0, 1.0]], dtype=np.float32)
    process_ref.process(x, [[0, 1, 0, 1, 7]], 3, penalty=2.0)
    assert x.tolist() == [[2.0, -8.0, 1.0]]               # each once, the out-of-range token ignored


def _gen_text(args):
    from src.generation import generate_text
    seen = []

    class M:
        def eval(self):
            pass

        def generate(self, **kw):
            seen.append(kw)
            return torch.arange(4 * 3).view(4, 3)

    tok = types.SimpleNamespace(decode=lambda seq, skip_special_tokens=True: " ".join(str(int(x)) for x in seq))
    generate_text(M(), [make_batch(2, enc_len=16, dec_len=8, num_regions=3)], tok, args, "cpu")
    return seen[0]


def test_generate_text_forwards_the_processors_only_when_set():
    plain_keys = {"input_ids", "image_features", "attention_mask", "num_beams", "num_return_sequences", "do_sample", "top_p",
                  "top_k", "early_stopping"}
    assert set(_gen_text(types.SimpleNamespace(num_beams=1, num_gen=2))) == plain_keys
    assert set(_gen_text(types.SimpleNamespace(num_beams=1, num_gen=2, repetition_penalty=1.0, no_repeat_ngram_size=0,
                                               device_processors=True))) == plain_keys
    kw = _gen_text(types.SimpleNamespace(num_beams=1, num_gen=2, repetition_penalty=1.3, no_repeat_ngram_size=0))
    assert set(kw) == plain_keys | {"repetition_penalty"} and kw["repetition_penalty"] == 1.3
    kw = _gen_text(types.SimpleNamespace(num_beams=1, num_gen=2, repetition_penalty=1.2, no_repeat_ngram_size=3))
    assert set(kw) == plain_keys | {"repetition_penalty", "no_repeat_ngram_size"} and kw["no_repeat_ngram_size"] == 3


def test_vcg_generate_flags():
    import vcg_generate
    base = ["--output_file", "o.json", "--checkpoint", "ck", "--synthetic", "1"]
    a = vcg_generate.parse_args(base)
    assert a.repetition_penalty == 1.0 and a.no_repeat_ngram_size == 0 and a.device_processors is False
    a = vcg_generate.parse_args(base + ["--repetition_penalty", "1.2", "--no_repeat_ngram_size", "3", "--device_processors"])
    assert a.repetition_penalty == 1.2 and a.no_repeat_ngram_size == 3 and a.device_processors is True
