"""GPU: generate() with its score processors applied on the device (model._device_processors = True, one beam): greedy ids
equal to the torch loop's and scores within 1e-4, the golden ids, no host processing on that path and the unchanged default,
seeded sampling against the torch loop (the bounds of tests/test_sample_scores_gpu.py), the folded embedding and the cleared
head statistics behind Engine.process_logits, and the searches that keep the host loops with the switch on."""
import ctypes as C
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ATOL = 1e-4            # tests/test_greedy_gpu.py, tests/test_sample_scores_gpu.py
BAD = [[40], [29, 52]]
COMBINED = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, bad_words_ids=BAD)


def _p(x):
    return None if x is None else C.c_void_p(x.data_ptr())


@pytest.fixture(scope="module")
def tiny():
    from oracle import goldenlib as G
    from src.model import MultiModalBartConfig, MultiModalBartForConditionalGeneration
    ocfg = G.tiny_config()
    keys = ("vocab_size", "d_model", "encoder_layers", "decoder_layers", "encoder_attention_heads",
            "decoder_attention_heads", "encoder_ffn_dim", "decoder_ffn_dim", "max_position_embeddings",
            "image_feature_size", "img_feat_id", "cls_token_id", "dropout", "attention_dropout", "activation_dropout")
    model = MultiModalBartForConditionalGeneration(MultiModalBartConfig.from_dict({k: getattr(ocfg, k) for k in keys}))
    model.load_state_dict(G.trained_state_dict(), strict=False)
    return model.to(DEV).eval()


@pytest.fixture()
def switched(tiny):
    tiny._device_processors = True
    yield tiny
    del tiny._device_processors


def _dev(b):
    return dict(input_ids=b["input_ids"].to(DEV), image_features=[f.to(DEV) for f in b["image_features"]],
                attention_mask=b["attention_mask"].to(DEV))


def _repeating_batch():
    """4 copy-task rows whose text repeats tokens and bigrams: the processors have something to act on."""
    from oracle.make_golden_reference_api import processors_batch
    return _dev(processors_batch())


def _batch(n, seed=9):
    from oracle.make_golden import copy_task_batch
    return _dev(copy_task_batch(seed, n))


def _count_calls(monkeypatch):
    """Counts Engine.process_logits and _postprocess_next_token_scores (both still run)."""
    import src.model.model as M
    from kmbart.engine import Engine
    calls = dict(device=0, host=0)
    real_dev, real_host = Engine.process_logits, M._postprocess_next_token_scores

    def dev(self, *a, **k):
        calls["device"] += 1
        return real_dev(self, *a, **k)

    def host(*a, **k):
        calls["host"] += 1
        return real_host(*a, **k)

    monkeypatch.setattr(Engine, "process_logits", dev)
    monkeypatch.setattr(M, "_postprocess_next_token_scores", host)
    return calls


@pytest.mark.parametrize("eos", ["eos", "no_eos"])
@pytest.mark.parametrize("over", [dict(repetition_penalty=1.3), dict(no_repeat_ngram_size=2), dict(bad_words_ids=BAD), COMBINED],
                         ids=["penalty", "ngram", "bad_words", "combined"])
def test_greedy_equals_the_torch_loop(switched, monkeypatch, over, eos):
    calls = _count_calls(monkeypatch)
    kw = dict(_repeating_batch(), num_beams=1, max_length=12, min_length=4, return_scores=True, **over)
    if eos == "no_eos":   # generate(eos_token_id=None) means the config's: only a config without one decodes without EOS
        monkeypatch.setattr(switched.config, "eos_token_id", None)
    a = switched.generate(**kw)
    assert calls["device"] >= 1 and calls["host"] == 0
    switched._device_greedy = False
    try:
        b = switched.generate(**kw)
    finally:
        del switched._device_greedy
    assert calls["host"] >= 1
    assert a[0].dtype == torch.long and torch.equal(a[0], b[0]), (a[0].tolist(), b[0].tolist())
    err = (a[1] - b[1]).abs().max().item()
    print("greedy %s %s: score difference %.3e" % (sorted(over), eos, err))
    assert a[1].dtype == torch.float32 and a[1].shape == (4,) and err <= ATOL, (a[1].tolist(), b[1].tolist())
    if eos == "eos":
        assert not bool((a[0][:, 1:4] == switched.config.eos_token_id).any())        # min_length still bans EOS
    else:
        assert a[0].shape == (4, 12)
    if "bad_words_ids" in over:   # the processors act on this search: the plain one starts row 0 with the banned token
        plain = switched.generate(**{k: v for k, v in kw.items() if k not in over})
        assert int(plain[0][0, 2]) == BAD[0][0] and not bool((a[0][:, 1:] == BAD[0][0]).any())


def test_golden_greedy_case(switched, gold_dir, monkeypatch):
    fx = json.load(open(os.path.join(gold_dir, "tiny_generate_processors.json")))
    case = [c for c in fx["cases"] if c["kwargs"].get("num_beams") == 1]
    assert len(case) == 1 and case[0]["kwargs"] == dict(num_beams=1, max_length=12, **COMBINED)
    calls = _count_calls(monkeypatch)
    ids = switched.generate(**case[0]["kwargs"], **_repeating_batch())
    assert ids.cpu().tolist() == case[0]["ids"]
    assert calls["device"] >= 1 and calls["host"] == 0


def test_no_host_processing_on_the_device_path_and_the_default_is_unchanged(tiny, monkeypatch):
    import src.model.model as M
    from kmbart.engine import Engine
    real = M._postprocess_next_token_scores
    reached, dev_calls = [], []

    def raising(*a, **k):
        raise AssertionError("the host function was reached")

    real_dev = Engine.process_logits
    monkeypatch.setattr(Engine, "process_logits", lambda self, *a, **k: dev_calls.append(1) or real_dev(self, *a, **k))
    kw = dict(_repeating_batch(), num_beams=1, max_length=12, **COMBINED)
    assert not hasattr(tiny, "_device_processors")
    monkeypatch.setattr(M, "_postprocess_next_token_scores", lambda *a, **k: reached.append(1) or real(*a, **k))
    want = tiny.generate(**kw)                                 # attribute absent: the torch loop, as before
    assert reached and not dev_calls
    torch.manual_seed(3)
    tiny.generate(**dict(kw, do_sample=True, top_k=8))
    assert not dev_calls
    monkeypatch.setattr(M, "_postprocess_next_token_scores", raising)
    with pytest.raises(AssertionError, match="host function was reached"):
        tiny.generate(**kw)
    for falsy in (False, 0, None):
        tiny._device_processors = falsy
        try:
            with pytest.raises(AssertionError, match="host function was reached"):
                tiny.generate(**kw)
        finally:
            del tiny._device_processors
    tiny._device_processors = True
    try:
        got = tiny.generate(**kw)                              # greedy
        n = len(dev_calls)
        assert n >= 1 and torch.equal(got, want)
        torch.manual_seed(3)
        tiny.generate(**dict(kw, do_sample=True, top_k=8))     # sampling
        assert len(dev_calls) > n
        n = len(dev_calls)
        tiny.generate(**{k: v for k, v in kw.items() if k not in COMBINED})    # no processors: no new launch
        assert len(dev_calls) == n
    finally:
        del tiny._device_processors


def _pad_to(a, n, pad):
    return torch.nn.functional.pad(a, (0, n - a.shape[1]), value=pad)


def test_sampling_against_the_torch_loop(switched, monkeypatch):
    """64 rows for this case only, so that an agreement of 0.95 has a meaning."""
    calls = _count_calls(monkeypatch)
    kw = dict(_batch(64), do_sample=True, num_beams=1, top_k=8, top_p=0.9, max_length=12, min_length=4, return_logprobs=True, **COMBINED)
    torch.manual_seed(17)
    a, la = switched.generate(**kw)
    assert calls["device"] >= 1 and calls["host"] == 0
    switched._device_sampling = False
    try:
        torch.manual_seed(17)
        c, lc = switched.generate(**kw)
    finally:
        del switched._device_sampling
    assert calls["host"] >= 1
    n, pad = max(a.shape[1], c.shape[1]), switched.config.pad_token_id
    same = (_pad_to(a, n, pad) == _pad_to(c, n, pad)).all(dim=1)
    agree = float(same.float().mean())
    ta, tc = _pad_to(la.token_logprobs, n - 1, 0.0), _pad_to(lc.token_logprobs, n - 1, 0.0)
    dt = (ta - tc)[same].abs().max().item()
    ds = (la.sum_logprobs - lc.sum_logprobs)[same].abs().max().item()
    print("sampling with processors: %d of %d rows equal, token_logprobs %.3e, sum_logprobs %.3e" % (int(same.sum()), len(same), dt, ds))
    assert agree >= 0.95, (a[:4].tolist(), c[:4].tolist())
    assert dt <= ATOL and ds <= ATOL, (dt, ds)
    # log-probabilities of the processed, filtered distribution: finite, <= 0, the banned single token never drawn
    assert bool(torch.isfinite(la.token_logprobs).all()) and bool((la.token_logprobs <= 0).all())
    assert not bool((a[:, 1:] == BAD[0][0]).any())
    assert (la.sum_logprobs - la.token_logprobs.sum(1)).abs().max().item() <= ATOL


def test_fold_stays_intact_behind_process_logits(tiny):
    eng = tiny._need_engine()
    b = _batch(5)
    start = torch.full((5,), tiny.config.decoder_start_token_id, dtype=torch.long, device=DEV)
    ids = torch.full((5, 6), 1, dtype=torch.long, device=DEV)
    ids[:, 0] = start
    bad = (torch.tensor([40, 29, 52], dtype=torch.int32, device=DEV), torch.tensor([0, 1, 3], dtype=torch.int32, device=DEV))
    eng.gen_begin(b["input_ids"], b["image_features"], b["attention_mask"], 1, 6)
    lg = eng.gen_step(start, 0)
    version = lg._version
    before = lg.clone()
    out = eng.process_logits(lg, ids, 1, 1.3, 1, bad)
    assert out is lg and lg._version == version == eng._gen_logits_version       # torch saw no in-place op
    nxt = eng.greedy_step(lg, ids=ids, t=1, embed_step=1)
    assert eng.lib.kmb_gen_embedded_step(eng.h) == 1                             # the kmb_gen_* form ran and folded the embedding
    torch.cuda.synchronize()
    V = tiny.config.vocab_size
    s = int(start[0])
    assert bool((lg[:, s] == -float("inf")).all()) and bool((lg[:, 40] == -float("inf")).all())   # n == 1 bans the start token
    keep = torch.ones(lg.shape[1], dtype=torch.bool, device=DEV)
    keep[[s, 40]] = False
    assert torch.equal(lg[:, keep], before[:, keep])
    assert not bool((nxt == s).any()) and not bool((nxt == 40).any()) and torch.equal(ids[:, 1], nxt)
    lg2 = eng.gen_step(nxt, 1)                                                   # runs on the folded rows
    assert eng.lib.kmb_gen_embedded_step(eng.h) == -1 and bool(torch.isfinite(lg2[:, :V]).all())


def test_statistics_are_cleared(tiny):
    """300 rows, one beam: the step's vocabulary projection leaves its per-block statistics; the edit drops them."""
    eng = tiny._need_engine()
    b = _batch(300)
    start = torch.full((300,), tiny.config.decoder_start_token_id, dtype=torch.long, device=DEV)
    ids = start.view(300, 1).clone()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    eng.gen_begin(b["input_ids"], b["image_features"], b["attention_mask"], 1, 4)
    lg = eng.gen_step(start, 0)
    assert eng.lib.kmb_gen_stats_blocks(eng.h, _p(lg)) > 0
    other = lg.clone()                                                           # other logits: the statistics stay
    from kmbart._lib import check
    check(eng.lib.kmb_gen_logits_process(eng.h, _p(other), other.stride(0), _p(ids), 1, 1, 1.3, 0, None, None, 0, stream))
    assert eng.lib.kmb_gen_stats_blocks(eng.h, _p(lg)) > 0
    # a refused call changes nothing
    assert eng.lib.kmb_gen_logits_process(eng.h, _p(lg), lg.stride(0), _p(ids), 1, 2, 1.3, 0, None, None, 0, stream) != 0
    assert eng.lib.kmb_last_error().decode().startswith("kmb_gen_logits_process: ")
    assert eng.lib.kmb_gen_stats_blocks(eng.h, _p(lg)) > 0
    check(eng.lib.kmb_gen_logits_process(eng.h, _p(lg), lg.stride(0), _p(ids), 1, 1, 1.3, 0, None, None, 0, stream))
    assert eng.lib.kmb_gen_stats_blocks(eng.h, _p(lg)) == 0
    torch.cuda.synchronize()
    assert torch.equal(lg, other)                                                # the two forms make the same edit


def test_gen_form_needs_one_beam(tiny):
    eng = tiny._need_engine()
    b = _batch(2)
    eng.gen_begin(b["input_ids"], b["image_features"], b["attention_mask"], 3, 4)
    lg = eng.gen_step(torch.zeros(6, dtype=torch.long, device=DEV), 0)
    ids = torch.zeros((6, 1), dtype=torch.long, device=DEV)
    with pytest.raises(Exception, match="kmb_gen_logits_process: needs num_beams == 1"):
        eng.process_logits(lg, ids, 1, 1.3)


def test_host_fallbacks_with_the_switch_on(switched, monkeypatch):
    calls = _count_calls(monkeypatch)
    kwb = _repeating_batch()
    # beam search and beam sampling with processors: the host beam loop
    for extra in (dict(num_beams=3, early_stopping=True), dict(num_beams=2, do_sample=True, top_k=8)):
        calls.update(device=0, host=0)
        torch.manual_seed(5)
        switched.generate(max_length=12, **extra, **COMBINED, **kwb)
        assert calls["device"] == 0 and calls["host"] >= 1, extra
    # the fp32 validation mode: the torch one-beam loop
    switched._engine.set_precision(True)
    try:
        calls.update(device=0, host=0)
        switched.generate(num_beams=1, max_length=12, **COMBINED, **kwb)
        assert calls["device"] == 0 and calls["host"] >= 1
    finally:
        switched._engine.set_precision(False)
    # bad words the table cannot hold (a token outside the vocabulary): the torch loop as well
    calls.update(device=0, host=0)
    V = switched.config.vocab_size
    switched.generate(num_beams=1, max_length=12, bad_words_ids=[[40], [V + 3, 41]], **kwb)
    assert calls["device"] == 0 and calls["host"] >= 1
