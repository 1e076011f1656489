"""CPU: several targets per input (targets_per_input / samples_per_input) -- everything that needs no GPU.

* leave_one_out_baseline (src/training.py) against a float64 loop; each group's advantages sum to zero within fp32 rounding; G = 1 raises.
* The model's shape checks raise before the engine is touched: the models here live on the CPU, where any engine call raises RuntimeError
  ("runs on an MI355X only"), so a ValueError / NotImplementedError proves the check came first.
* kmb_forward_opts.targets_per_input: the ctypes mirror's word sits behind loss_reduction inside the library's sizeof, a zeroed record reads 0.
* kmb_workspace_bytes_grouped equals kmb_workspace_bytes at G <= 1 and grows with G on the decoder side only.
"""
import ctypes as C

import pytest
import torch

from kmbart import _lib
from kmbart._lib import KmbConfig, KmbForwardOpts, check
from src.model import MultiModalBartConfig, MultiModalBartForConditionalGeneration, MultiModalBartForPreTraining
from src.training import leave_one_out_baseline, self_critical_step

TINY = dict(vocab_size=512, d_model=128, encoder_layers=1, decoder_layers=1, encoder_attention_heads=2, decoder_attention_heads=2,
            encoder_ffn_dim=128, decoder_ffn_dim=128, max_position_embeddings=64, img_feat_id=488, cls_token_id=491)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    return _lib.load()


# ------------------------------------------------------------------------------------------------ the baseline arithmetic
@pytest.mark.parametrize("B,G", [(1, 2), (3, 4), (7, 5)])
def test_leave_one_out_baseline_against_a_float64_loop(B, G):
    g = torch.Generator().manual_seed(100 * B + G)
    r = (torch.rand(B * G, generator=g) * 3.0).float()
    base = leave_one_out_baseline(r, G)
    assert base.shape == r.shape and base.dtype == torch.float32
    want = torch.empty(B * G, dtype=torch.float64)
    for i in range(B):
        for j in range(G):
            others = [float(r[i * G + k]) for k in range(G) if k != j]
            want[i * G + j] = sum(others) / (G - 1)
    # fp32: a sum of G values below 3 and one division: a few ulps of the group's sum
    assert float((base.double() - want).abs().max()) <= 4 * G * 2.0 ** -24 * 3.0 * G
    adv = (r - base).view(B, G)
    assert float(adv.sum(dim=1).abs().max()) <= 8 * G * 2.0 ** -24 * 3.0 * G   # each group's advantages sum to zero


def test_leave_one_out_baseline_refuses_one_sample_and_ragged_groups():
    with pytest.raises(ValueError, match="samples_per_input >= 2"):
        leave_one_out_baseline(torch.ones(4), 1)
    with pytest.raises(ValueError):
        leave_one_out_baseline(torch.ones(7), 2)


def test_self_critical_step_refuses_mean_with_one_sample():
    """before the model is touched (model = None)"""
    batch = dict(input_ids=torch.zeros((2, 4), dtype=torch.long), image_features=[torch.empty(0)] * 2, attention_mask=torch.ones((2, 4), dtype=torch.long))
    with pytest.raises(ValueError, match="samples_per_input >= 2"):
        self_critical_step(None, batch, lambda ids: None, "cpu", baseline="mean", samples_per_input=1)
    with pytest.raises(ValueError, match="num_return_sequences"):
        self_critical_step(None, batch, lambda ids: None, "cpu", baseline=None, samples_per_input=2, sample_kwargs=dict(num_return_sequences=3))


# ------------------------------------------------------------------------------------------------ the model's shape checks
def _inputs(B, rows, T=8):
    return dict(input_ids=torch.zeros((B, 6), dtype=torch.long), image_features=[torch.empty(0)] * B,
                attention_mask=torch.ones((B, 6), dtype=torch.long), decoder_input_ids=torch.zeros((rows, T), dtype=torch.long),
                decoder_attention_mask=torch.ones((rows, T), dtype=torch.long), labels=torch.zeros((rows, T), dtype=torch.long))


def test_model_checks_raise_before_any_engine_call():
    model = MultiModalBartForConditionalGeneration(MultiModalBartConfig.from_dict(TINY))
    with pytest.raises(RuntimeError, match="MI355X"):          # the control: a well-formed grouped call reaches the (absent) engine
        model(**_inputs(2, 6), targets_per_input=3)
    with pytest.raises(ValueError, match="3 x 2 = 6 rows"):    # decoder rows not G x inputs
        model(**_inputs(2, 5), targets_per_input=3)
    kw = _inputs(2, 6)
    kw["labels"] = kw["labels"][:4]
    with pytest.raises(ValueError, match="labels"):
        model(**kw, targets_per_input=3)
    with pytest.raises(ValueError, match="loss_weights"):
        model(**_inputs(2, 6), targets_per_input=3, loss_weights=torch.ones(2), loss_reduction="sum")
    kw = _inputs(2, 6)
    kw.pop("labels")
    with pytest.raises(NotImplementedError, match="cached"):
        model(**kw, targets_per_input=3, use_cache=True)
    with pytest.raises(NotImplementedError, match="attention / hidden-state"):
        model(**_inputs(2, 6), targets_per_input=3, output_attentions=True)
    with pytest.raises(NotImplementedError, match="attention / hidden-state"):
        model(**_inputs(2, 6), targets_per_input=3, output_hidden_states=True)
    with pytest.raises(ValueError, match="positive"):
        model(**_inputs(2, 6), targets_per_input=-1)
    kw = _inputs(2, 6)
    kw.pop("decoder_input_ids")
    with pytest.raises(ValueError, match="decoder_input_ids"):
        model(**kw, targets_per_input=3)
    for g in (None, 1):                                        # one target per input: today's path, i.e. straight to the engine
        with pytest.raises(RuntimeError, match="MI355X"):
            model(**_inputs(2, 2), targets_per_input=g)


def test_pretraining_model_has_no_grouped_forward():
    cfg = MultiModalBartConfig.from_dict(dict(TINY, num_labels=5, num_attributes=4, num_relations=3))
    model = MultiModalBartForPreTraining(cfg)
    with pytest.raises(NotImplementedError, match="grouped"):
        model(**_inputs(2, 4), targets_per_input=2)
    with pytest.raises(RuntimeError, match="MI355X"):
        model(**_inputs(2, 2), targets_per_input=1)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_forward_opts_word(lib):
    assert C.sizeof(KmbForwardOpts) == lib.kmb_abi_sizeof_forward_opts()
    off = KmbForwardOpts._TPI_OFFSET
    assert off == KmbForwardOpts.loss_reduction.offset + C.sizeof(C.c_int32), "the int32 right behind loss_reduction"
    assert off + C.sizeof(C.c_int32) <= lib.kmb_abi_sizeof_forward_opts()
    z = KmbForwardOpts()
    assert z.targets_per_input == 0 and z.loss_reduction == 0
    z.targets_per_input = 5
    assert z.targets_per_input == 5 and z.loss_reduction == 0 and not z.row_weights
    assert bytes(z)[off:off + 4] == (5).to_bytes(4, "little")


def test_workspace_bytes_grouped(lib):
    h = C.c_void_p()
    cfg = KmbConfig(**dict(TINY, extra_pos_embeddings=2, image_feature_size=2052, pad_token_id=1, bos_token_id=0, eos_token_id=2,
                           scale_embedding=0, dropout=0.0, attention_dropout=0.0, activation_dropout=0.0, layer_norm_eps=1e-5))
    check(lib.kmb_create(C.byref(cfg), C.byref(h)))
    try:
        one = lib.kmb_workspace_bytes(h, 8, 24, 16, 40)
        assert lib.kmb_workspace_bytes_grouped(h, 8, 24, 16, 40, 0) == one
        assert lib.kmb_workspace_bytes_grouped(h, 8, 24, 16, 40, 1) == one
        g4 = lib.kmb_workspace_bytes_grouped(h, 8, 24, 16, 40, 4)
        rep = lib.kmb_workspace_bytes(h, 32, 24, 16, 160)
        print("workspace bytes: one target %d, grouped G=4 %d, replicated %d" % (one, g4, rep))
        assert one < g4 < rep, "the grouped layout holds the decoder side of 32 targets and the encoder side of 8 inputs"
    finally:
        lib.kmb_destroy(h)
