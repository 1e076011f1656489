"""GPU: generate() with greedy beam search and its score processors on the device (model._device_beam_processors = True): the
golden beam cases' ids with no host processing, equality with the host beam loop, the folded embedding behind a processed step,
the benchmarked 64 x 5 rows at vcg_base dimensions against the host loop, the searches that keep the host loop with the switch
on, and the unchanged default."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAD = [[40], [29, 52]]
COMBINED = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, bad_words_ids=BAD)


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
    tiny._device_beam_processors = True
    yield tiny
    del tiny._device_beam_processors


@pytest.fixture(scope="module")
def base():
    """vcg_base dimensions, random weights re-scaled as tests/test_decode_fused_gpu.py does (the searches depend on the item
    and move along the sequence)."""
    from oracle import goldenlib as G
    from oracle import kmbart_oracle as O
    from src.model import MultiModalBartConfig, MultiModalBartForConditionalGeneration
    from test_fullsize_parity_gpu import BASE
    sd = G.golden_state_dict(O.OracleConfig.from_dict(BASE), seed=11)
    sd["model.shared.weight"] = sd["model.shared.weight"] * 8.0
    sd["model.decoder.embed_positions.weight"] = sd["model.decoder.embed_positions.weight"] * 40.0
    for k_ in list(sd):
        if k_.endswith("out_proj.weight") or k_.endswith("fc2.weight"):
            sd[k_] = sd[k_] * 3.0
    model = MultiModalBartForConditionalGeneration(MultiModalBartConfig.from_dict(BASE))
    model.load_state_dict(sd, strict=False)
    return model.to(DEV).eval()


def _dev(b):
    return dict(input_ids=b["input_ids"].to(DEV), image_features=[f.to(DEV) for f in b["image_features"]],
                attention_mask=b["attention_mask"].to(DEV))


def _repeating_batch():
    from oracle.make_golden_reference_api import processors_batch
    return _dev(processors_batch())


def _count_calls(monkeypatch):
    """Counts Engine.beam_step_processed and _postprocess_next_token_scores (both still run)."""
    import src.model.model as M
    from kmbart.engine import Engine
    calls = dict(device=0, host=0)
    real_dev, real_host = Engine.beam_step_processed, M._postprocess_next_token_scores

    def dev(self, *a, **k):
        calls["device"] += 1
        return real_dev(self, *a, **k)

    def host(*a, **k):
        calls["host"] += 1
        return real_host(*a, **k)

    monkeypatch.setattr(Engine, "beam_step_processed", dev)
    monkeypatch.setattr(M, "_postprocess_next_token_scores", host)
    return calls


def _beam_cases(gold_dir):
    fx = json.load(open(os.path.join(gold_dir, "tiny_generate_processors.json")))
    cases = [c for c in fx["cases"] if c["kwargs"].get("num_beams", 1) > 1]
    assert len(cases) == 4
    return cases


def test_golden_beam_cases_on_the_device_and_against_the_host_loop(switched, gold_dir, monkeypatch):
    calls = _count_calls(monkeypatch)
    kwb = _repeating_batch()
    for case in _beam_cases(gold_dir):
        kw = case["kwargs"]
        calls.update(device=0, host=0)
        ids, sc = switched.generate(return_scores=True, **kw, **kwb)
        assert calls["device"] >= 1 and calls["host"] == 0, kw
        assert ids.cpu().tolist() == case["ids"], (kw, ids.cpu().tolist(), case["ids"])
        gold = torch.tensor(case["scores"])
        print("%s: score difference to the fixture %.3e" % (sorted(kw), (sc.float().cpu() - gold).abs().max().item()))
        assert torch.allclose(sc.float().cpu(), gold, atol=3e-2), kw
        del switched._device_beam_processors                      # the host loop: the same ids
        try:
            hid, hsc = switched.generate(return_scores=True, **kw, **kwb)
        finally:
            switched._device_beam_processors = True
        assert calls["host"] >= 1
        assert torch.equal(ids, hid) and torch.allclose(sc.float().cpu(), hsc.float().cpu(), atol=3e-2), kw


def test_without_the_switch_nothing_changes(tiny, gold_dir, monkeypatch):
    calls = _count_calls(monkeypatch)
    kwb = _repeating_batch()
    assert not hasattr(tiny, "_device_beam_processors")
    case = _beam_cases(gold_dir)[3]
    for setting in ("absent", False, 0, None):
        if setting != "absent":
            tiny._device_beam_processors = setting
        try:
            calls.update(device=0, host=0)
            ids = tiny.generate(**case["kwargs"], **kwb)
        finally:
            if setting != "absent":
                del tiny._device_beam_processors
        assert calls["device"] == 0 and calls["host"] >= 1 and ids.cpu().tolist() == case["ids"], setting
    # the switch without processors: the plain pipelined loop, no processed step
    tiny._device_beam_processors = True
    try:
        calls.update(device=0, host=0)
        plain = tiny.generate(num_beams=3, max_length=12, early_stopping=True, **kwb)
    finally:
        del tiny._device_beam_processors
    fx = json.load(open(os.path.join(gold_dir, "tiny_generate_processors.json")))
    assert calls == dict(device=0, host=0) and plain.cpu().tolist() == fx["plain_ids"]


def test_routing_exclusions_take_the_host_loop(switched, monkeypatch):
    calls = _count_calls(monkeypatch)
    kwb = _repeating_batch()
    cfg = switched.config
    V = cfg.vocab_size
    beams = dict(num_beams=3, max_length=12, early_stopping=True)
    for extra in (dict(no_repeat_ngram_size=1),                                    # bans the start token
                  dict(bad_words_ids=[[40], [29, cfg.bos_token_id]]),              # a bad word ending in BOS
                  dict(do_sample=True, top_k=8, **COMBINED),                       # beam sampling
                  dict(bad_words_ids=[[40], [V + 3, 41]])):                        # a table the packer cannot hold
        calls.update(device=0, host=0)
        torch.manual_seed(5)
        switched.generate(**beams, **extra, **kwb)
        assert calls["device"] == 0 and calls["host"] >= 1, extra
    switched._engine.set_precision(True)                                           # the fp32 validation mode
    try:
        calls.update(device=0, host=0)
        switched.generate(**beams, **COMBINED, **kwb)
        assert calls["device"] == 0 and calls["host"] >= 1
    finally:
        switched._engine.set_precision(False)
    calls.update(device=0, host=0)                                                 # one beam: the other switch's business
    switched.generate(num_beams=1, max_length=12, **COMBINED, **kwb)
    assert calls["device"] == 0 and calls["host"] >= 1
    calls.update(device=0, host=0)
    switched.generate(**beams, **COMBINED, **kwb)
    assert calls["device"] >= 1 and calls["host"] == 0


def test_embedding_is_folded_behind_a_processed_reordering_step(base):
    from src.data.synthetic import make_batch
    eng = base._need_engine()
    B, nb, L = 2, 3, 6
    b = _dev(make_batch(B, seed=4321))
    R, k = B * nb, 2 * nb
    start = torch.full((R,), base.config.decoder_start_token_id, dtype=torch.long, device=DEV)
    ids = [torch.full((R, L), int(start[0]), dtype=torch.long, device=DEV) for _ in range(2)]
    add = torch.tensor([0.0, -1e9, -1e9] * B, dtype=torch.float32, device=DEV)
    eng.gen_begin(b["input_ids"], b["image_features"], b["attention_mask"], nb, L)
    lg = eng.gen_step(start, 0)
    cand, add, tok, idx = eng.beam_step_processed(lg, nb, k, add, ids[0], ids[1], 1, 1.3, 2, None, reorder_step=0)
    assert eng.lib.kmb_gen_embedded_step(eng.h) == 1                 # the kmb_gen_* form ran and embedded the chosen tokens
    torch.cuda.synchronize()
    assert torch.equal(ids[1][:, 1], tok) and bool((ids[1][:, 0] == start).all())
    assert bool((idx.view(B, nb) == (torch.arange(B, device=DEV) * nb).view(B, 1)).all())   # every beam continues beam 0
    lg2 = eng.gen_step(tok, 1)                                       # runs on the folded rows
    assert eng.lib.kmb_gen_embedded_step(eng.h) == -1 and bool(torch.isfinite(lg2[:, :base.config.vocab_size]).all())
    cand, add, tok2, idx2 = eng.beam_step_processed(lg2, nb, k, add, ids[1], ids[0], 2, 1.3, 2, None, reorder_step=1)
    assert eng.lib.kmb_gen_embedded_step(eng.h) == 2
    torch.cuda.synchronize()
    assert torch.equal(ids[0][:, :2], ids[1][idx2.long(), :2]) and torch.equal(ids[0][:, 2], tok2)


def _host_score_of(model, kwb, seqs, nb, max_length, p, n, length_penalty=1.0):
    """The host loop's score of given sequences (one per batch item, pad-stripped lists): teacher forced on the same number of
    rows as the search (every beam of an item is fed the item's sequence), torch.log_softmax +
    _postprocess_next_token_scores on the rows' histories as _host_beam_loop does, forced steps counting 0; the sum over the
    tokens / len ** length_penalty with len = the length before a final EOS (BeamHypotheses.add as the search reaches it)."""
    from src.model.model import _postprocess_next_token_scores
    eng, cfg = model._need_engine(), model.config
    B, V = len(seqs), cfg.vocab_size
    eng.gen_begin(kwb["input_ids"], kwb["image_features"], kwb["attention_mask"], nb, max_length)
    total = [0.0] * B
    for t in range(1, max(len(s) for s in seqs)):
        toks = torch.tensor([s[min(t - 1, len(s) - 1)] for s in seqs for _ in range(nb)], dtype=torch.long, device=DEV)
        sc = torch.log_softmax(eng.gen_step(toks, t - 1)[:, :V].float(), dim=-1)
        hist = [list(s[:min(t, len(s))]) for s in seqs for _ in range(nb)]
        _postprocess_next_token_scores(sc, hist, t, 0, cfg.eos_token_id, p, n, None)
        forced = t == 1 or t == max_length - 1
        for b, s in enumerate(seqs):
            if t < len(s) and not forced:
                total[b] += float(sc[b * nb, s[t]])
    out = []
    for b, s in enumerate(seqs):
        hyp_len = len(s) - 1 if s[-1] == cfg.eos_token_id else len(s)
        out.append(total[b] / hyp_len ** length_penalty)
    return out


def test_rows_320_at_base_dimensions_equal_the_host_loop(base, monkeypatch):
    from src.data.synthetic import make_batch
    calls = _count_calls(monkeypatch)
    p, n, nb, L = 1.3, 2, 5, 6
    kwb = _dev(make_batch(64, seed=4321))
    kw = dict(num_beams=nb, max_length=L, early_stopping=True, repetition_penalty=p, no_repeat_ngram_size=n, return_scores=True)
    base._device_beam_processors = True
    try:
        ids, sc = base.generate(**kw, **kwb)
    finally:
        del base._device_beam_processors
    assert calls["device"] >= 1 and calls["host"] == 0
    hid, hsc = base.generate(**kw, **kwb)
    assert calls["host"] >= 1
    pad = base.config.pad_token_id
    m = max(ids.shape[1], hid.shape[1])
    a = torch.nn.functional.pad(ids, (0, m - ids.shape[1]), value=pad).cpu()
    h = torch.nn.functional.pad(hid, (0, m - hid.shape[1]), value=pad).cpu()
    differ = torch.nonzero((a != h).any(dim=1)).flatten().tolist()
    print("64 x 5 with processors: %d of 64 rows differ from the host loop; distinct sequences %d; score difference %.3e"
          % (len(differ), len({tuple(r) for r in h.tolist()}), (sc.float().cpu() - hsc.float().cpu()).abs().max().item()))
    assert len({tuple(r) for r in h.tolist()}) > 1                      # the searches depend on the item
    assert len(differ) <= 2, differ
    if differ:   # a differing row must be a tie by the host loop's own arithmetic
        seqs = []
        for r in range(64):
            s = a[r].tolist()
            while len(s) > 1 and s[-1] == pad:
                s.pop()
            seqs.append(s)
        mine = _host_score_of(base, kwb, seqs, nb, L, p, n)
        for r in differ:
            print("row %d: device %s host %s; host score %.6f, the host arithmetic's score of the device's sequence %.6f"
                  % (r, a[r].tolist(), h[r].tolist(), float(hsc[r]), mine[r]))
            assert abs(mine[r] - float(hsc[r])) <= 1e-4 * p, r
