"""CPU: the host side of sampled-sequence log-probabilities -- the two C-ABI entries (kmb_sample_scored_step,
kmb_gen_sample_step) in the library, the header and the ctypes table, generate(return_logprobs=...), sample_sentence's
contract, the torch loop's per-step score, and generate_text's optional "scores"."""
import inspect
import math
import os
import re
import types

import pytest
import torch

from kmbart import _lib
from src.data.synthetic import make_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("kmb_sample_scored_step", "kmb_gen_sample_step")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    return _lib.load()


def test_new_symbols_in_library_header_and_prototypes(lib):
    header = open(os.path.join(ROOT, "include", "kmbart.h")).read()
    for name in NEW:
        assert hasattr(lib, name), "libkmbart_hip.so does not export %s" % name
        m = re.search(r"^int %s\(([^;]*)\);" % name, header, re.M)
        assert m, "include/kmbart.h does not declare %s" % name
        params = [p for p in m.group(1).replace("\n", " ").split(",") if p.strip()]
        restype, argtypes = _lib.PROTOTYPES[name]
        assert len(argtypes) == len(params), (name, len(argtypes), len(params))
    # the scored form is kmb_sample_step's arguments + (logprob_sum, logprob_out, ld_logprob) before the stream; the decode loop's
    # form drops V and R, gains the handle and embed_step
    base = _lib.PROTOTYPES["kmb_sample_step"][1]
    assert len(_lib.PROTOTYPES["kmb_sample_scored_step"][1]) == len(base) + 3
    assert _lib.PROTOTYPES["kmb_sample_scored_step"][1][:len(base) - 1] == base[:-1]
    assert len(_lib.PROTOTYPES["kmb_gen_sample_step"][1]) == len(base) + 3 - 2 + 2


def test_signatures():
    from src.model import MultiModalBartForConditionalGeneration
    from src.model.utils import sample_sentence
    p = inspect.signature(MultiModalBartForConditionalGeneration.generate).parameters
    assert p["return_logprobs"].default is False and p["return_scores"].default is False
    sig = inspect.signature(sample_sentence)
    assert [(n, q.default) for n, q in sig.parameters.items()] == [
        ("model", inspect.Parameter.empty), ("input_ids", inspect.Parameter.empty), ("image_features", inspect.Parameter.empty),
        ("attention_mask", inspect.Parameter.empty), ("tokenizer", inspect.Parameter.empty), ("top_k", 50), ("top_p", 1.0),
        ("max_length", 20)]


def test_sample_sentence_is_one_generate_call():
    from src.model import GenerationLogprobs
    from src.model.utils import sample_sentence
    seen = []
    ids = torch.arange(3 * 5).view(3, 5)
    sums = torch.tensor([-1.5, -2.25, -0.5])

    class M:
        def generate(self, **kw):
            seen.append(kw)
            return ids, GenerationLogprobs(torch.zeros(3, 4), sums)

    tok = types.SimpleNamespace(bos_token_id=0, pad_token_id=1, eos_token_id=2)
    inp, feats, am = torch.ones(3, 7, dtype=torch.long), [torch.zeros(2, 4)] * 3, torch.ones(3, 7, dtype=torch.long)
    out_ids, out_sum = sample_sentence(M(), inp, feats, am, tok, top_k=11, top_p=0.8, max_length=9)
    assert len(seen) == 1
    kw = seen[0]
    assert kw.pop("input_ids") is inp and kw.pop("image_features") is feats and kw.pop("attention_mask") is am
    assert kw == dict(do_sample=True, num_beams=1, return_logprobs=True, top_k=11, top_p=0.8, max_length=9, temperature=1.0,
                      min_length=0, num_return_sequences=1, repetition_penalty=1.0, no_repeat_ngram_size=0, bad_words_ids=None,
                      decoder_start_token_id=0, pad_token_id=1, eos_token_id=2)
    assert out_ids is ids and out_sum.shape == (3, 1) and torch.equal(out_sum, sums[:, None])
    # the defaults are the reference's
    sample_sentence(M(), inp, feats, am, tok)
    assert (seen[1]["top_k"], seen[1]["top_p"], seen[1]["max_length"]) == (50, 1.0, 20)


def test_torch_loop_step_score_is_the_renormalised_filtered_distribution():
    from src.model.model import _chosen_logprobs, _top_k_top_p_filtering
    x = torch.tensor([[0.0, 2.0, -1.0, 3.0, 0.5, -4.0],
                      [1.0, 1.0, -2.0, 0.0, 5.0, 4.0]])
    lg = _top_k_top_p_filtering(x.clone(), top_k=2, top_p=1.0)
    # row 0 keeps {3: 3.0, 1: 2.0}, row 1 keeps {4: 5.0, 5: 4.0}: two-token softmax with a gap of 1
    hi, lo = -math.log1p(math.exp(-1.0)), -1.0 - math.log1p(math.exp(-1.0))
    got = _chosen_logprobs(lg, torch.tensor([1, 4]))
    assert got.dtype == torch.float32
    assert abs(float(got[0]) - lo) <= 1e-6 and abs(float(got[1]) - hi) <= 1e-6
    got = _chosen_logprobs(lg, torch.tensor([3, 5]))
    assert abs(float(got[0]) - hi) <= 1e-6 and abs(float(got[1]) - lo) <= 1e-6
    # a finished row scores 0
    got = _chosen_logprobs(lg, torch.tensor([3, 5]), unfinished=torch.tensor([1, 0]))
    assert abs(float(got[0]) - hi) <= 1e-6 and float(got[1]) == 0.0


def _gen_text(args, returns_logprobs):
    from src.generation import generate_text
    from src.model import GenerationLogprobs
    seen = []

    class M:
        def eval(self):
            pass

        def generate(self, **kw):
            seen.append(kw)
            ids = torch.arange(4 * 3).view(4, 3)
            if returns_logprobs:
                return ids, GenerationLogprobs(torch.zeros(4, 2), torch.tensor([-0.5, -1.5, -2.5, -3.5]))
            return ids

    tok = types.SimpleNamespace(decode=lambda seq, skip_special_tokens=True: " ".join(str(int(x)) for x in seq))
    b = make_batch(2, enc_len=16, dec_len=8, num_regions=3)
    return generate_text(M(), [b], tok, args, "cpu"), seen


def test_generate_text_scores_only_when_asked():
    plain_keys = {"input_ids", "image_features", "attention_mask", "num_beams", "num_return_sequences", "do_sample", "top_p",
                  "top_k", "early_stopping"}
    out, seen = _gen_text(types.SimpleNamespace(num_beams=1, num_gen=2, do_sample=True, top_k=50, with_scores=True), True)
    assert set(seen[0]) == plain_keys | {"return_logprobs"} and seen[0]["return_logprobs"] is True
    assert [set(r) for r in out] == [{"index", "task_type", "generations", "scores"}] * 2
    assert out[0]["scores"] == [-0.5, -1.5] and out[1]["scores"] == [-2.5, -3.5]
    assert all(isinstance(x, float) for r in out for x in r["scores"])
    assert out[1]["generations"] == ["6 7 8", "9 10 11"]
    # without the flag, with it off, and with beams: today's call and today's records
    for args in (types.SimpleNamespace(num_beams=1, num_gen=2, do_sample=True),
                 types.SimpleNamespace(num_beams=1, num_gen=2, with_scores=False),
                 types.SimpleNamespace(num_beams=3, num_gen=2, with_scores=True)):
        out, seen = _gen_text(args, False)
        assert set(seen[0]) == plain_keys
        assert [set(r) for r in out] == [{"index", "task_type", "generations"}] * 2


def test_routes_are_unchanged():
    from src.model.model import _decode_route, _one_beam_on_device
    assert list(inspect.signature(_decode_route).parameters) == ["num_beams", "do_sample", "processors_on", "fp32",
                                                                  "device_sampling", "has_sampler", "V"]
    assert list(inspect.signature(_one_beam_on_device).parameters) == ["do_sample", "processors_on", "fp32", "device_greedy"]
    names = {_decode_route(nb, ds, pr, fp, dv, hs, 50265) for nb in (1, 5) for ds in (False, True) for pr in (False, True)
             for fp in (False, True) for dv in (False, True) for hs in (False, True)}
    assert names == {"device_sampling", "one_beam", "pipelined_beams", "host_beams"}
    assert _decode_route(1, True, False, False, True, False, 50265) == "device_sampling"
    assert _one_beam_on_device(False, False, False, True) and not _one_beam_on_device(True, False, False, True)
