"""CPU: host-side logic of the drop-in surface (config, synthetic batches, feature packing,
fine_tune loop order and log format, generate_text record schema)."""
import json
import types

import pytest
import torch

from src.data.synthetic import IMG_FEAT, make_batch
from src.model.config import MultiModalBartConfig


def test_config_defaults_and_roundtrip(tmp_path):
    cfg = MultiModalBartConfig.from_dict({"d_model": 768, "encoder_layers": 6, "partial_load": ["final_logits_bias"]})
    assert cfg.image_feature_size == 2052 and cfg.img_feat_id == 50273 and cfg.cls_token_id == 50276
    assert cfg.max_length == 20 and cfg.num_beams == 1 and cfg.extra_pos_embeddings == 2
    cfg.dropout = 0.3  # vcg_train.py:76-83 writes these attributes after construction
    cfg.save_pretrained(str(tmp_path))
    again = MultiModalBartConfig.from_pretrained(str(tmp_path))
    assert again.dropout == 0.3 and again.d_model == 768 and list(again.partial_load) == ["final_logits_bias"]
    d = json.loads(again.to_json_string())
    assert d["model_type"] == "bart"


def test_synthetic_batch_shape():
    b = make_batch(4, seed=1234)
    assert b["input_ids"].shape == (4, 64) and b["decoder_input_ids"].shape == (4, 32) and b["labels"].shape == (4, 32)
    assert all(f.shape == (36, 2052) for f in b["image_features"])
    assert int((b["input_ids"] == IMG_FEAT).sum()) == 4 * 36
    assert torch.all(b["decoder_input_ids"][:, 0] == 0) and torch.all(b["labels"][:, -1] == 2)
    assert torch.equal(b["labels"][:, :-1], b["decoder_input_ids"][:, 1:])
    f = b["image_features"][0]
    assert float(f[:, :2048].min()) >= 0 and torch.all(f[:, 2050] > f[:, 2048]) and torch.all(f[:, 2051] > f[:, 2049])
    r = make_batch(2, regions=[36, 20], event_lens=[23, 7], label_lens=[32, 9], seed=1)
    assert r["attention_mask"][1].sum() == 5 + 20 + 7 and int((r["labels"][1] == -100).sum()) == 32 - 9
    assert r["input_ids"][1, 32:].eq(1).all()
    assert torch.equal(make_batch(2, seed=7)["input_ids"], make_batch(2, seed=7)["input_ids"])


def test_pack_features_handles_empty_samples():
    from kmbart.engine import pack_features
    feats = [torch.ones(3, 8), torch.empty(0), torch.full((2, 8), 2.0)]
    packed, offs, n = pack_features(feats, 8, "cpu")
    assert n == 5 and offs.tolist() == [0, 3, 3, 5] and packed.shape == (5, 8) and float(packed[3:].mean()) == 2.0
    packed, offs, n = pack_features([torch.empty(0)], 8, "cpu")
    assert n == 0 and offs.tolist() == [0, 0]


class _FakeLoss:
    def __init__(self, log, v):
        self.log, self.v = log, v

    def item(self):
        self.log.append("item")
        return self.v

    def backward(self):
        self.log.append("backward")

    def detach(self):
        return self


class _FakeModel:
    def __init__(self, log):
        self.log = log

    def train(self):
        self.log.append("train")

    def forward(self, **kw):
        assert set(kw) >= {"input_ids", "image_features", "attention_mask", "labels", "answer_ids"}
        self.log.append("forward")
        return (_FakeLoss(self.log, 1.5),)


class _FakeOpt:
    def __init__(self, log):
        self.log = log

    def zero_grad(self):
        self.log.append("zero_grad")

    def step(self):
        self.log.append("step")


def test_fine_tune_order_and_log_line():
    """reference src/training.py:118-153: forward -> zero_grad -> backward -> step, log format; the loss of step i is
    read (`.item()`, a host synchronisation) only after step i+1 has been enqueued -- or before the callback runs."""
    from src.training import fine_tune
    log, lines = [], []
    b = make_batch(2, enc_len=16, dec_len=8, num_regions=3)
    logger = types.SimpleNamespace(info=lambda m, pad=False: lines.append(m))
    seen = []
    fine_tune(0, _FakeModel(log), [b, b], _FakeOpt(log), "cpu", types.SimpleNamespace(amp=False, epochs=3), logger=logger,
              callback=lambda **kw: seen.append(sorted(kw)))
    assert log == ["train"] + ["forward", "zero_grad", "backward", "step", "item"] * 2   # a callback sees step i reported
    assert lines[0].startswith("Epoch [1/3], Step [1/2], Loss: 1.5000, ETA: ")
    assert lines[1].startswith("Epoch [1/3], Step [2/2], Loss: 1.5000, ETA: ") and len(lines) == 2
    assert seen[0] == ["args", "epoch", "logger", "model", "optimizer", "step", "train_loader"]
    # without a callback the read trails the enqueue by one step; every step is still reported, in order
    log.clear()
    lines.clear()
    mean = fine_tune(0, _FakeModel(log), [b, b, b], _FakeOpt(log), "cpu", types.SimpleNamespace(amp=False, epochs=3),
                     logger=logger)
    one = ["forward", "zero_grad", "backward", "step"]
    assert log == ["train"] + one + one + ["item"] + one + ["item", "item"]
    assert [ln.split(",")[1].strip() for ln in lines] == ["Step [1/3]", "Step [2/3]", "Step [3/3]"] and mean == 1.5


def test_generate_text_record_schema():
    from src.generation import generate_text

    class M:
        def eval(self):
            pass

        def generate(self, **kw):
            assert kw["early_stopping"] is True and kw["num_return_sequences"] == 2 and kw["top_k"] == 0
            return torch.arange(4 * 3).view(4, 3)

    tok = types.SimpleNamespace(decode=lambda seq, skip_special_tokens=True: " ".join(str(int(x)) for x in seq))
    b = make_batch(2, enc_len=16, dec_len=8, num_regions=3)
    out = generate_text(M(), [b], tok, types.SimpleNamespace(num_beams=3, num_gen=2), "cpu",
                        logger=types.SimpleNamespace(info=lambda m: None))
    assert [r["index"] for r in out] == [0, 1] and out[1]["generations"] == ["6 7 8", "9 10 11"]
    assert set(out[0]) == {"index", "task_type", "generations"}


def test_config_equals_the_reference_class_dump(gold_dir):
    """tests/golden/config_reference.json was written by the REFERENCE's own MultiModalBartConfig (imported from
    /root/reference/src/model/config.py by oracle/make_golden_reference_api.py): defaults, from_dict of both shipped JSON
    files, and the attribute writes vcg_train.py:71-83 makes afterwards.  The product class must hold the same values."""
    import os
    ref = json.load(open(os.path.join(gold_dir, "config_reference.json")))
    vcg = {"d_model": 768, "decoder_attention_heads": 12, "decoder_ffn_dim": 3072, "decoder_layers": 6,
           "encoder_attention_heads": 12, "encoder_ffn_dim": 3072, "encoder_layers": 6,
           "partial_load": ["final_logits_bias", "model.shared.weight", "model.encoder.embed_tokens.weight",
                            "model.decoder.embed_tokens.weight"]}
    pre = dict(vcg, num_labels=1601, num_attributes=129, num_relations=129, lm_loss_factor=5, mrm_loss_factor=1,
               attribute_loss_factor=1, relation_loss_factor=1)

    def same(cfg, want, tag):
        for k, v in want.items():
            got = getattr(cfg, k)
            got = list(got) if isinstance(got, tuple) else got
            assert got == v and type(got) is type(v), (tag, k, got, v)

    same(MultiModalBartConfig(), ref["defaults"], "defaults")
    same(MultiModalBartConfig.from_dict(vcg), ref["vcg_base"], "vcg_base")
    same(MultiModalBartConfig.from_dict(pre), ref["pretrain_base"], "pretrain_base")
    cfg = MultiModalBartConfig.from_dict(vcg)
    cfg.dropout, cfg.attention_dropout, cfg.classif_dropout, cfg.activation_dropout = 0.3, 0.2, 0.1, 0.05
    same(cfg, ref["vcg_base_after_cli_writes"], "cli writes")
    # every attribute the product defines is either dumped from the reference or declared as restated
    from src.model.config import _DEFAULTS
    assert set(_DEFAULTS) == set(ref["defaults"]) | set(ref["restated_not_dumped"])


def test_generate_text_equals_the_reference_function(gold_dir):
    """tests/golden/generate_text_reference.json: the REFERENCE's own generate_text (src/generation.py:6-52) driven over
    the oracle's beam search on the trained tiny fixture.  The product's generate_text over the SAME adapter must pass
    the same keyword arguments to `generate`, return the same records and log the same lines."""
    import os
    from oracle import goldenlib as G
    from oracle.make_golden_reference_api import OracleGenerateAdapter, gen_loader
    from src.generation import generate_text
    ref = json.load(open(os.path.join(gold_dir, "generate_text_reference.json")))
    cfg, sd = G.tiny_config(), G.trained_state_dict()
    for case in ref["cases"]:
        calls, lines = [], []
        recs = generate_text(OracleGenerateAdapter(cfg, sd, calls), gen_loader(), G.IdTokenizer(),
                             types.SimpleNamespace(amp=False, **case["args"]), torch.device("cpu"),
                             logger=types.SimpleNamespace(info=lambda m: lines.append(m)), log_interval=1)
        assert calls == case["generate_kwargs"]
        assert recs == case["records"]
        assert [ln.split(", ETA")[0] for ln in lines] == case["log_prefixes"]


def test_pretrain_loop_uses_the_loss_dict():
    """reference src/training.py:9-93: outputs[0] is a dict; 'loss' drives backward; kwargs of the forward call."""
    from src.data.synthetic import make_pretrain_batch
    from src.training import pretrain
    log, lines = [], []

    class M:
        def train(self):
            log.append("train")

        def forward(self, **kw):
            assert {"mrm_labels", "mrm_mask", "attribute_labels", "attribute_mask", "relation_labels", "labels"} <= set(kw)
            assert isinstance(kw["mrm_labels"], list) and kw["mrm_mask"].dtype == torch.bool
            log.append("forward")
            return ({"loss": _FakeLoss(log, 2.0), "lm_loss": _FakeLoss([], 1.5), "mrm_loss": _FakeLoss([], 0.5)},)

    b = make_pretrain_batch(2, enc_len=24, dec_len=16, num_regions=6, num_labels=11, num_attributes=5, num_relations=4)
    assert b["mrm_labels"][0].shape == (int(b["mrm_mask"][0].sum()), 11)
    assert abs(float(b["mrm_labels"][0].sum(-1)[0]) - 1.0) < 1e-5 and len(b["relation_labels"][1]) == 3
    assert int(b["attribute_mask"][0].sum()) == len(b["attribute_labels"][0])
    logger = types.SimpleNamespace(info=lambda m, pad=False: lines.append(m))
    pretrain(0, M(), [b], _FakeOpt(log), "cpu", types.SimpleNamespace(amp=False, epochs=2), logger=logger)
    assert log == ["train", "forward", "zero_grad", "backward", "step", "item"]
    assert lines[0].startswith("Epoch [1/2], Step [1/1], Loss: 2.0000, ETA: ")


def test_packed_features_roundtrip():
    from kmbart.data import PackedFeatures
    from kmbart.engine import pack_features
    feats = [torch.ones(3, 8), torch.empty(0), torch.full((2, 8), 2.0)]
    pf = PackedFeatures.from_list(feats, 8)
    assert len(pf) == 3 and pf.n_total == 5 and pf.offsets.tolist() == [0, 3, 3, 5]
    packed, offs, n = pack_features(pf, 8, "cpu")
    assert n == 5 and torch.equal(packed, pf.packed) and offs.dtype == torch.int32


def test_reference_parameter_order_matches_bart_registration_order():
    """A torch-format optimizer state of the reference is indexed by the position of a parameter in `model.parameters()`
    (reference vcg_train.py:100, src/utils.py:20-39).  `reference_parameter_order` restates that order; its BART part is
    pinned here on the installed transformers' BartForConditionalGeneration, whose module registration order for these
    modules is the one of 3.0.2 (k_proj, v_proj, q_proj, out_proj; layernorm_embedding after the layers), and the
    KM-BART additions on the reference source: embed_images is registered right after embed_tokens
    (src/model/modules.py:73-74), the heads after the model (src/model/model.py:131-158)."""
    from transformers import BartConfig, BartForConditionalGeneration
    from kmbart.optim import reference_parameter_order
    from oracle import kmbart_oracle as O
    ocfg = O.OracleConfig(vocab_size=64, d_model=64, encoder_layers=2, decoder_layers=3, encoder_attention_heads=1,
                          decoder_attention_heads=1, encoder_ffn_dim=64, decoder_ffn_dim=64, max_position_embeddings=16,
                          num_labels=7, num_attributes=5, num_relations=3)
    names = O.param_names(ocfg) + O.head_param_names(ocfg)
    order = reference_parameter_order(names)
    assert sorted(order) == sorted(names)
    hf = BartForConditionalGeneration(BartConfig(
        vocab_size=64, d_model=64, encoder_layers=2, decoder_layers=3, encoder_attention_heads=1,
        decoder_attention_heads=1, encoder_ffn_dim=64, decoder_ffn_dim=64, max_position_embeddings=16))
    hf_names = [n for n, _ in hf.named_parameters()]
    bart_part = [n for n in order if "embed_images" not in n and "_head." not in n]
    assert bart_part == hf_names
    i = order.index("model.encoder.embed_images.linear.weight")
    assert order[i - 1] == "model.shared.weight" and order[i + 1] == "model.encoder.embed_images.linear.bias"
    assert order[i + 2] == "model.encoder.embed_positions.weight"
    assert order[-12:] == [h + s for h in ("mrm_head", "attribute_head", "relation_head")
                           for s in (".dense.weight", ".dense.bias", ".out_proj.weight", ".out_proj.bias")]


def test_validate_generation_score_is_importable_and_says_what_it_needs():
    """reference vcg_train.py:28 imports `validate_generation_score` from src.validation; the metric package behind it
    (src/evaluation.py + Java tools) is out of scope, so without it the call must fail loudly BEFORE generating."""
    import pytest
    from src.validation import validate_fine_tune_loss, validate_generation_score, validate_pretraining_loss  # noqa: F401
    with pytest.raises(NotImplementedError) as e:
        validate_generation_score(0, object(), [], [], None, "cpu", types.SimpleNamespace(cpu=True))
    assert "evaluation" in str(e.value)


def test_forward_pretrain_refuses_ignored_labels_for_the_hard_label_heads():
    """-100 never reaches the attribute / relation heads on the reference's data path (its collator writes class ids there and masks
    only the LM labels); the engine's head loss and gradient would average such a batch differently, so forward_pretrain refuses it
    before anything is sent to the device (no engine state is touched: an unconstructed Engine is enough to show that)."""
    from kmbart.engine import Engine, refuse_ignored_head_labels
    rows = torch.arange(3, dtype=torch.int32)
    good, bad = torch.tensor([4, 0, 7]), torch.tensor([4, -100, 7])
    refuse_ignored_head_labels("attribute", good)
    refuse_ignored_head_labels("relation", None)
    refuse_ignored_head_labels("relation", torch.zeros(0, dtype=torch.int64))
    eng = object.__new__(Engine)
    with pytest.raises(ValueError, match="attribute labels hold -100"):
        Engine.forward_pretrain(eng, None, None, None, None, None, None, attr=(rows, bad))
    with pytest.raises(ValueError, match="relation labels hold -100"):
        Engine.forward_pretrain(eng, None, None, None, None, None, None, attr=(rows, good), rel=(rows, rows, bad))
