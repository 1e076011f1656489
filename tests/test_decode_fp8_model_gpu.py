"""GPU: FP8 (e4m3) decoder weights through the engine and the model.

The FP8 path on a model M must return BIT FOR BIT what the bf16 path returns on M', the model whose six per-layer decoder matrices
are replaced by their dequantised values (tests/fp8_ref.py): teacher-forced logits, and ids with scores / log-probabilities of
generate() on every route.  The bf16 path is pinned to the oracle by tests/test_decode_fused_gpu.py and
tests/test_decode_rows_oracle_gpu.py; the FP8 mode inherits that chain.  Also: the pack cache keys on the format (bf16 -> FP8 ->
bf16 on one model), an edit of a weight repacks, the three loud refusals, and the untouched bf16 default.

Model: the smallest configuration the fused blocks take -- d = 768, 12 heads, FFN 3072, one encoder layer, two decoder layers, a
vocabulary of 1024 -- with golden weights (oracle.goldenlib), re-scaled as tests/test_decode_fused_gpu.py does so that the searches
move along the sequence."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import fp8_ref as Q  # noqa: E402
from gpu_util import DEV  # noqa: E402
from kmbart._lib import KmbError  # noqa: E402
from oracle import goldenlib as G  # noqa: E402
from oracle import kmbart_oracle as O  # noqa: E402
from src.data.synthetic import make_batch  # noqa: E402
from src.model import MultiModalBartConfig, MultiModalBartForConditionalGeneration  # noqa: E402

SPECIAL = 1000
CFG = dict(activation_dropout=0.0, attention_dropout=0.0, d_model=768, decoder_attention_heads=12, decoder_ffn_dim=3072,
           decoder_layers=2, dropout=0.0, encoder_attention_heads=12, encoder_ffn_dim=3072, encoder_layers=1, init_std=0.02,
           max_position_embeddings=64, vocab_size=1024, img_feat_id=SPECIAL + 8, cls_token_id=SPECIAL + 11)
# kmb_gen_workspace_bytes(B = 64, S = 100, num_beams = 5, max_length = 20, n_features = 2304) of this configuration as the PARENT
# commit's library returns it (taken from a run of the parent): the bf16 default sizes what it sized
PARENT_WS_BYTES_64_100_5_20 = 316254464


def _batch(B, seed=77):
    regions = ([9, 4, 12] * B)[:B]
    events = ([11, 7, 3] * B)[:B]
    return make_batch(B, enc_len=32, dec_len=8, seed=seed, regions=regions, event_lens=events, vocab_hi=SPECIAL,
                      img_feat_id=SPECIAL + 8, special_base=SPECIAL)


def _model(sd):
    m = MultiModalBartForConditionalGeneration(MultiModalBartConfig.from_dict(CFG))
    m.load_state_dict(sd, strict=False)
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def world():
    """(state dict of M, model M, model M' with the dequantised decoder matrices in bf16); built once, never changed"""
    ocfg = O.OracleConfig.from_dict(CFG)
    sd = G.golden_state_dict(ocfg, seed=11)
    sd["model.shared.weight"] = sd["model.shared.weight"] * 8.0
    sd["model.decoder.embed_positions.weight"] = sd["model.decoder.embed_positions.weight"] * 40.0
    for k in list(sd):
        if k.endswith("out_proj.weight") or k.endswith("fc2.weight"):
            sd[k] = sd[k] * 3.0
    sdq = Q.quantize_model_state(sd, CFG["decoder_layers"])
    changed = [k for k in sd if not torch.equal(sd[k].to(torch.bfloat16), sdq[k].to(torch.bfloat16))]
    assert len(changed) == 8 * CFG["decoder_layers"], changed
    return sd, _model(sd), _model(sdq)


def _gen(model, b, **kw):
    torch.manual_seed(1234)
    out = model.generate(input_ids=b["input_ids"].to(DEV), image_features=[f.to(DEV) for f in b["image_features"]],
                         attention_mask=b["attention_mask"].to(DEV), max_length=8, **kw)
    torch.cuda.synchronize()
    return out


def _flat(out):
    """generate()'s return value as a flat list of tensors (ids, then scores / log-probabilities)"""
    if torch.is_tensor(out):
        return [out]
    flat = []
    for o in out:
        flat += _flat(o)
    return flat


def _same(a, b):
    fa, fb = _flat(a), _flat(b)
    return len(fa) == len(fb) and all(x.shape == y.shape and torch.equal(x.cpu(), y.cpu()) for x, y in zip(fa, fb))


def _teacher_forced_logits(model, b, nb, T):
    eng = model._engine
    B = b["input_ids"].shape[0]
    eng.gen_begin(b["input_ids"].to(DEV), [f.to(DEV) for f in b["image_features"]], b["attention_mask"].to(DEV), nb, T + 1)
    eng.check_inputs()
    out = []
    for t in range(T):
        tok = b["decoder_input_ids"][:, t].repeat_interleave(nb).to(DEV)
        out.append(eng.gen_step(tok, t)[:, : model.config.vocab_size].float().clone())
        eng.gen_reorder(torch.arange(B * nb, dtype=torch.int32, device=DEV), t)   # identity: the cache ping-pong of generate()
    torch.cuda.synchronize()
    return torch.stack(out, dim=1).cpu()


def test_format_setting_and_bf16_default(world):
    _, m, _ = world
    fresh = MultiModalBartForConditionalGeneration(MultiModalBartConfig.from_dict(CFG))
    assert fresh.decoder_weight_format == "bf16" and m.decoder_weight_format == "bf16"
    assert "decoder_weight_format" not in " ".join(fresh.state_dict())
    with pytest.raises(ValueError):
        fresh.set_decoder_weight_format("int8")
    fresh.set_decoder_weight_format("fp8_e4m3")                     # before .to(device): kept, applied when the engine exists
    assert fresh.decoder_weight_format == "fp8_e4m3"
    eng = m._engine
    ws = eng.lib.kmb_gen_workspace_bytes(eng.h, 64, 100, 5, 20, 2304)
    assert ws == PARENT_WS_BYTES_64_100_5_20, ws
    m.set_decoder_weight_format("fp8_e4m3")
    try:
        assert m.decoder_weight_format == "fp8_e4m3"
        d, F, L = 768, 3072, CFG["decoder_layers"]
        assert ws - eng.lib.kmb_gen_workspace_bytes(eng.h, 64, 100, 5, 20, 2304) == L * (6 * d * d + 2 * d * F) - L * (7 * d + F)
    finally:
        m.set_decoder_weight_format("bf16")
    assert eng.lib.kmb_gen_workspace_bytes(eng.h, 64, 100, 5, 20, 2304) == ws


def test_teacher_forced_logits_bit_for_bit(world):
    _, m, mq = world
    b = _batch(2)
    want = _teacher_forced_logits(mq, b, 3, 6)
    plain = _teacher_forced_logits(m, b, 3, 6)
    m.set_decoder_weight_format("fp8_e4m3")
    try:
        got = _teacher_forced_logits(m, b, 3, 6)
    finally:
        m.set_decoder_weight_format("bf16")
    assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0
    assert not torch.equal(plain, want), "quantising the decoder changed nothing: the comparison would show nothing"
    rel = float((want - plain).norm() / plain.norm())
    print("[fp8 decoder weights] teacher-forced logits, FP8 vs bf16 weights on the same model: norm-wise rel %.2e" % rel)
    assert torch.equal(got, want), "%d of %d logits differ" % (int((got != want).sum()), want.numel())


@pytest.mark.parametrize("name,kw", [("greedy", dict(num_beams=1, return_logprobs=True)),
                                     ("beam4", dict(num_beams=4, return_scores=True, early_stopping=True)),
                                     ("sample_top_p", dict(num_beams=1, do_sample=True, top_p=0.9, return_logprobs=True)),
                                     ("beam_sample_top_k", dict(num_beams=3, do_sample=True, top_k=2, return_scores=True))])
def test_generate_bit_for_bit(world, name, kw):
    _, m, mq = world
    b = _batch(3)
    want = _gen(mq, b, **kw)
    m.set_decoder_weight_format("fp8_e4m3")
    try:
        got = _gen(m, b, **kw)
    finally:
        m.set_decoder_weight_format("bf16")
    ids = _flat(want)[0]
    assert ids.shape[0] == 3 and len(_flat(want)) >= 2, "ids and scores / log-probabilities"
    print("[fp8 decoder weights] generate %s ids %s" % (name, ids.cpu().tolist()))
    assert _same(got, want), (name, [t.cpu().tolist() for t in _flat(got)], [t.cpu().tolist() for t in _flat(want)])


def test_switching_formats_in_one_process(world):
    """bf16 -> FP8 -> bf16 on one model: the packed copies live at the same place in both formats, so the `already packed` test has
    to key on the format."""
    _, m, mq = world
    b = _batch(3)
    kw = dict(num_beams=4, return_scores=True)
    first = _gen(m, b, **kw)
    m.set_decoder_weight_format("fp8_e4m3")
    try:
        fp8 = _gen(m, b, **kw)
    finally:
        m.set_decoder_weight_format("bf16")
    last = _gen(m, b, **kw)
    assert _same(last, first)
    assert _same(fp8, _gen(mq, b, **kw))
    lf, lq = _teacher_forced_logits(m, b, 1, 3), _teacher_forced_logits(mq, b, 1, 3)
    assert not torch.equal(lf, lq)                                  # (the two formats do differ on this model)


def test_weight_edit_repacks(world):
    """A decoder weight changed through its parameter, the mirror rewritten as an optimizer step rewrites it: the next FP8
    generation quantises the new weights (the result of a freshly built reference model M'')."""
    sd, _, _ = world
    key = "model.decoder.layers.1.fc1.weight"
    m = _model(sd)
    b = _batch(2)
    m.set_decoder_weight_format("fp8_e4m3")
    before = _teacher_forced_logits(m, b, 2, 3)
    sd2 = dict(sd)
    sd2[key] = sd[key].clone()
    sd2[key][5:40] *= -1.5
    with torch.no_grad():
        dict(m.named_parameters())[key].copy_(sd2[key].to(DEV))
    m._engine.sync_params()                                         # rewrites the bf16 mirror and bumps its version
    after = _teacher_forced_logits(m, b, 2, 3)
    ref = _model(Q.quantize_model_state(sd2, CFG["decoder_layers"]))
    want = _teacher_forced_logits(ref, b, 2, 3)
    assert not torch.equal(before, after)
    assert torch.equal(after, want)


def test_loud_refusals(world):
    _, m, _ = world
    b = _batch(2)
    eng = m._engine
    args = (b["input_ids"].to(DEV), [f.to(DEV) for f in b["image_features"]], b["attention_mask"].to(DEV))
    m.set_decoder_weight_format("fp8_e4m3")
    try:
        os.environ["KMB_GEN_FUSED"] = "0"
        try:
            with pytest.raises(KmbError, match="KMB_GEN_FUSED=0"):
                _gen(m, b, num_beams=1)
        finally:
            os.environ.pop("KMB_GEN_FUSED", None)
        big = _batch(345)                                           # 345 x 3 beams = 1035 rows
        with pytest.raises(KmbError, match="more than 1024 rows"):
            _gen(m, big, num_beams=3)
        eng.set_precision(True)
        try:
            with pytest.raises(KmbError, match="fp32 validation mode"):
                eng.gen_begin(*args, 1, 8)
        finally:
            eng.set_precision(False)
        # the environment changes between gen_begin and a step: the step refuses, it does not decode on bf16 weights
        eng.gen_begin(*args, 2, 8)
        os.environ["KMB_GEN_FUSED"] = "0"
        try:
            with pytest.raises(KmbError, match="KMB_GEN_FUSED=0"):
                eng.gen_step(torch.zeros(4, dtype=torch.int64, device=DEV), 0)
        finally:
            os.environ.pop("KMB_GEN_FUSED", None)
    finally:
        m.set_decoder_weight_format("bf16")
    assert _flat(_gen(m, b, num_beams=1))[0].shape[0] == 2          # and the model still generates in bf16
