"""GPU: gradient accumulation over micro-batches through the engine, the model classes, the optimizer, the training loops and the
data-parallel wrapper, on the tiny configuration.

The micro-batches differ in batch size, source / target length and region counts, so the workspace is laid out anew between them
(and filled with 0xFF under --poison): whatever survives from one micro-step to the next lives in the two arenas, not there.

Two rules are checked after every backward of an accumulating engine (`micro_step`):
 (1) fold identity: over the WHOLE arena, bit for bit, `grads == grads_before + grad_stage` -- `== grad_stage` on the first backward
     after zero_grad -- with torch's fp32 add on the right (one correctly rounded add per element, as the fold kernel's);
 (2) the stage is a plain backward: a second, non-accumulating model with the same weights, the same seed and the same call leaves
     the stage's bits in its gradient arena everywhere except `model.shared.weight`, whose embedding scatter-adds are fp32 atomics
     (DESIGN.md section 3).  Its bound comes from two PLAIN backwards of that call on the second model, a code path accumulation does
     not touch: 4 x their worst element-wise difference, at least one ulp of the tensor's largest magnitude.  That the two plain
     runs agree bit for bit elsewhere -- dropout 0.1, masks replayed by setting the seed before each forward -- is asserted first.

Batches whose result is compared between two RUNS beyond the tied matrix (the pre-training model; the training loops against a
hand-written loop at the AdamW op tolerance) are chosen so that no fp32 atomic meets a third addend: no token id twice in a batch and
no decoder row twice among a relation head's object (or subject) rows.  Two atomic adds onto a value commute only when it is zero."""
import os
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "km-bart_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import goldenlib as G  # noqa: E402
from oracle.make_golden import tiny_batch  # noqa: E402
from kmbart.optim import AdamW  # noqa: E402
from src.data.synthetic import make_pretrain_batch  # noqa: E402
from src.model import MultiModalBartForPreTraining  # noqa: E402
from test_model_gpu import build, cfg_from_oracle, run_fwd  # noqa: E402

DEV = "cuda:0"
LR = 1e-3
ATOL, RTOL = 2e-7, 1e-6     # tests/test_grad_clip_model_gpu.py's AdamW op tolerance
TIED = "model.shared.weight"
PRE_KW = dict(num_labels=37, num_attributes=11, num_relations=9, lm_loss_factor=5.0, mrm_loss_factor=1.0, attribute_loss_factor=2.0,
              relation_loss_factor=0.5)

# three ragged micro-batches: B / S / T / region counts all differ
MICRO = [dict(seed=5),
         dict(regions=(4, 2, 5), event_lens=(6, 3, 5), label_lens=(9, 5, 14), enc_len=20, dec_len=16, seed=6),
         dict(regions=(7,), event_lens=(5,), label_lens=(6,), enc_len=28, dec_len=8, seed=7)]


def micro_batch(k):
    return tiny_batch(**MICRO[k])


def to_dev(b):
    out = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in b.items()}
    out["image_features"] = [f.to(DEV) for f in b["image_features"]]
    return out


def bits(t):
    return t.contiguous().view(torch.int32)


def tied_range(eng):
    off, rows, cols = eng.index[TIED]
    return off, off + rows * cols


def ulp_of(x):
    return float(np.spacing(np.float32(x)))


def plain_backward_twice(plain, do):
    """the plain model's gradient arena after `do`, twice; asserts rule (2)'s precondition and returns (first run, tied bound)"""
    eng = plain._engine
    do(plain)
    torch.cuda.synchronize()
    g1 = eng.grads.clone()
    do(plain)
    torch.cuda.synchronize()
    g2 = eng.grads
    lo, hi = tied_range(eng)
    same = bits(g1) == bits(g2)
    same[lo:hi] = True
    assert bool(same.all()), "two plain backwards differ outside the tied matrix at %d elements" % int((~same).sum())
    spread = float((g1[lo:hi] - g2[lo:hi]).abs().max())
    bound = max(4.0 * spread, ulp_of(float(g1[lo:hi].abs().max())))
    return g1, spread, bound


def micro_step(acc, plain, do, first, tag):
    """one backward of the accumulating model under rules (1) and (2); returns the tied matrix's (difference, spread, bound)"""
    eng = acc._engine
    torch.cuda.synchronize()
    before = eng.grads.clone()
    do(acc)
    torch.cuda.synchronize()
    stage, total = eng.grad_stage, eng.grads
    want = stage if first else before + stage
    assert torch.equal(bits(total), bits(want)), "%s: fold identity fails at %d elements" % (tag, int((bits(total) != bits(want)).sum()))
    g1, spread, bound = plain_backward_twice(plain, do)
    lo, hi = tied_range(eng)
    same = bits(stage) == bits(g1)
    same[lo:hi] = True
    assert bool(same.all()), "%s: the stage differs from a plain backward at %d elements" % (tag, int((~same).sum()))
    diff = float((stage[lo:hi] - g1[lo:hi]).abs().max())
    print("[accum %s] tied matrix: stage vs plain %.3e, plain vs plain %.3e, bound %.3e" % (tag, diff, spread, bound))
    assert diff <= bound, (tag, diff, bound)
    return diff, spread, bound


def seeded(seed, b, scale=None, dev_scale=None, **fwd_kw):
    """`do(model)`: set the seed (the dropout masks of the next forward follow from it), forward, backward"""
    def do(model):
        model._engine.set_seed(seed)
        if scale is not None:
            model.train_step_fwd_bwd(to_dev(b), loss_scale=scale)
            return
        loss = run_fwd(model, b, **fwd_kw)[0]
        (loss if dev_scale is None else loss / dev_scale).backward()
    return do


class Ctx:
    pass


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    c.ocfg = G.tiny_config(dropout=0.1)
    c.sd = G.golden_state_dict(c.ocfg, seed=7)
    c.acc = build(c.ocfg, c.sd).train()
    c.plain = build(c.ocfg, c.sd).train()
    c.acc.accumulate_gradients(True)
    c.eng = c.acc._engine
    return c


def test_a_three_ragged_micro_batches_fold_and_equal_plain_backwards(ctx):
    eng = ctx.eng
    assert eng.accumulating and eng.grad_stage is not None and eng.grad_stage.numel() == eng.grads.numel()
    assert not ctx.plain._engine.accumulating and ctx.plain._engine.grad_stage is None
    ctx.acc.zero_grad()
    sums = mags = None
    for k in range(3):
        micro_step(ctx.acc, ctx.plain, seeded(100 + k, micro_batch(k)), first=(k == 0), tag="micro %d" % k)
        g = ctx.plain._engine.grads.double()
        sums, mags = (g, g.abs()) if sums is None else (sums + g, mags + g.abs())
    # the running total is the sum of the three plain gradients: outside the tied matrix the addends are the plain runs' own bits, and
    # two fp32 adds round twice, each by at most 2^-24 of a partial sum's magnitude
    total = eng.grads.double()
    assert bool(torch.isfinite(total).all()) and float(total.abs().max()) > 0
    ok = (total - sums).abs() <= 2.0 ** -23 * mags
    lo, hi = tied_range(eng)
    ok[lo:hi] = True
    assert bool(ok.all())
    # the alignment gaps between parameters (if the layout has any) stay zero in both arenas
    covered = torch.zeros(eng.n, dtype=torch.bool, device=DEV)
    for off, rows, cols in eng.index.values():
        covered[off: off + rows * cols] = True
    if int((~covered).sum()) > 0:
        assert float(eng.grads[~covered].abs().max()) == 0.0 and float(eng.grad_stage[~covered].abs().max()) == 0.0


def test_b_zero_grad_overwrites_a_poisoned_arena_and_later_backwards_add(ctx):
    eng = ctx.eng
    eng.grads.fill_(float("nan"))
    ctx.acc.zero_grad()
    micro_step(ctx.acc, ctx.plain, seeded(200, micro_batch(1)), first=True, tag="after zero_grad")
    assert bool(torch.isfinite(eng.grads).all()) and torch.equal(bits(eng.grads), bits(eng.grad_stage))
    # forward -> zero_grad -> backward, the reference's order: the flag is read when backward runs
    eng.grads.fill_(float("nan"))
    eng.set_seed(201)
    loss = run_fwd(ctx.acc, micro_batch(0))[0]
    AdamW(ctx.acc.parameters(), lr=LR).zero_grad()     # the optimizer's zero_grad reaches the engine too
    loss.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(eng.grads).all()) and torch.equal(bits(eng.grads), bits(eng.grad_stage))
    # without zero_grad the next backward adds
    micro_step(ctx.acc, ctx.plain, seeded(202, micro_batch(2)), first=False, tag="no zero_grad")


def test_c_without_accumulation_a_second_backward_overwrites(ctx):
    """today's behaviour, kept: passes with and without this feature"""
    plain, eng = ctx.plain, ctx.plain._engine
    seeded(300, micro_batch(0))(plain)
    torch.cuda.synchronize()
    g0 = eng.grads.clone()
    g1, _, bound = plain_backward_twice(plain, seeded(301, micro_batch(1)))
    assert not torch.equal(g0, g1)
    plain.zero_grad()                                   # a no-op in effect
    seeded(301, micro_batch(1))(plain)
    torch.cuda.synchronize()
    lo, hi = tied_range(eng)
    same = bits(eng.grads) == bits(g1)
    same[lo:hi] = True
    assert bool(same.all()) and float((eng.grads[lo:hi] - g1[lo:hi]).abs().max()) <= bound


@pytest.mark.parametrize("kind", ["float", "device"])
def test_d_scaled_backward(ctx, kind):
    """The scale multiplies the tied matrix's head gradient and the whole heads range IN PLACE: in the stage that is this micro-batch's
    gradient alone, in an arena accumulated in place it would rescale the earlier micro-batches too."""
    ctx.acc.zero_grad()
    kw = dict(scale=1.0 / 3.0) if kind == "float" else dict(dev_scale=3.0)
    for k in range(2):
        micro_step(ctx.acc, ctx.plain, seeded(400 + k, micro_batch(k), **kw), first=(k == 0), tag="%s scale, micro %d" % (kind, k))
    # and the scale really arrived: the second micro-batch's stage is a third of its unscaled gradient
    stage = ctx.eng.grad_stage.clone()
    seeded(401, micro_batch(1))(ctx.plain)
    torch.cuda.synchronize()
    full = ctx.plain._engine.grads
    assert float((stage * 3.0 - full).norm() / full.norm()) < 1e-2


def distinct_pretrain_batch(bsz, enc_len, dec_len, regions, seed0, n_rel, tokens=True):
    """the first seed >= seed0 whose batch has no decoder row twice among the relation head's object rows or among its subject rows
    and, with `tokens`, no token id twice (module docstring; a batch of several samples repeats the special tokens anyway: there the
    tied matrix is compared under its own bound)"""
    ocfg = G.tiny_config(**PRE_KW)
    for seed in range(seed0, seed0 + 200):
        b = make_pretrain_batch(bsz, enc_len=enc_len, dec_len=dec_len, num_regions=regions, seed=seed, num_labels=37, num_attributes=11,
                                num_relations=9, vocab_hi=G.TINY_SPECIAL_BASE, img_feat_id=ocfg.img_feat_id,
                                special_base=G.TINY_SPECIAL_BASE, cls_id=ocfg.cls_token_id, mrm_probability=0.3, n_rel=n_rel)
        ids = torch.cat([b["input_ids"].reshape(-1), b["decoder_input_ids"].reshape(-1)])
        ids = ids[(ids != 1) & (ids != ocfg.img_feat_id)]
        T = b["decoder_input_ids"].shape[1]
        obj = [i * T + r["object_index"] for i, rels in enumerate(b["relation_labels"]) for r in rels]
        sub = [i * T + r["subject_index"] for i, rels in enumerate(b["relation_labels"]) for r in rels]
        if ((not tokens or len(set(ids.tolist())) == ids.numel()) and len(set(obj)) == len(obj) and len(set(sub)) == len(sub)
                and int(b["mrm_mask"].sum()) > 0 and int(b["attribute_mask"].sum()) > 0):
            b["image_features"] = G.golden_features([regions] * bsz)
            return b
    raise AssertionError("no batch without repeated tokens / relation rows in 200 seeds")


def pre_fwd_bwd(seed, b, dev_scale=None):
    def do(model):
        model._engine.set_seed(seed)
        losses = model(input_ids=b["input_ids"].to(DEV), image_features=[f.to(DEV) for f in b["image_features"]],
                       attention_mask=b["attention_mask"].to(DEV), decoder_input_ids=b["decoder_input_ids"].to(DEV),
                       decoder_attention_mask=b["decoder_attention_mask"].to(DEV), labels=b["labels"].to(DEV),
                       mrm_labels=b["mrm_labels"], mrm_mask=b["mrm_mask"], attribute_labels=b["attribute_labels"],
                       attribute_mask=b["attribute_mask"], relation_labels=b["relation_labels"])[0]
        (losses["loss"] if dev_scale is None else losses["loss"] / dev_scale).backward()
    return do


def pre_model(sd, **over):
    m = MultiModalBartForPreTraining(cfg_from_oracle(G.tiny_config(**PRE_KW), **PRE_KW, **over))
    m.load_state_dict(sd, strict=False)
    return m.to(DEV).train()


def test_e_pretraining_heads_written_by_forward_fold_too():
    sd = G.golden_state_dict(G.tiny_config(**PRE_KW), seed=33)
    acc, plain = pre_model(sd, dropout=0.1, classif_dropout=0.1), pre_model(sd, dropout=0.1, classif_dropout=0.1)
    acc.accumulate_gradients(True)
    eng = acc._engine
    b0 = distinct_pretrain_batch(2, 24, 16, 6, seed0=77, n_rel=2, tokens=False)
    b1 = distinct_pretrain_batch(3, 20, 12, 4, seed0=90, n_rel=0, tokens=False)       # no relation rows: that head's gradients are zeroed by forward
    assert sum(len(r) for r in b0["relation_labels"]) > 0 and sum(len(r) for r in b1["relation_labels"]) == 0
    acc.zero_grad()
    micro_step(acc, plain, pre_fwd_bwd(500, b0, dev_scale=2.0), first=True, tag="pretrain 0")
    heads0 = {n: eng.view(eng.grads, n).clone() for n in eng.index if "_head." in n}
    assert len(heads0) == 12 and all(float(g.abs().max()) > 0 for g in heads0.values())
    micro_step(acc, plain, pre_fwd_bwd(501, b1, dev_scale=2.0), first=False, tag="pretrain 1")
    for n, g0 in heads0.items():
        now, st = eng.view(eng.grads, n), eng.view(eng.grad_stage, n)
        if n.startswith("relation_head."):
            assert float(st.abs().max()) == 0.0 and torch.equal(now, g0), n
        else:
            assert float(st.abs().max()) > 0 and torch.equal(bits(now), bits(g0 + st)), n


def test_f_forward_from_given_encoder_states_as_a_micro_step(ctx):
    """The second micro-step starts from given encoder states: its encoder buckets are zeros (a memset of the stage), so the total's
    equal the first micro-step's; the decoder side adds."""
    acc, eng = ctx.acc, ctx.eng
    b = micro_batch(0)
    acc.zero_grad()
    micro_step(acc, ctx.plain, seeded(600, b), first=True, tag="encoder micro 0")
    first = eng.grads.clone()
    with torch.no_grad():
        enc = run_fwd(acc.eval(), b)[2].detach().clone()
    acc.train()
    ctx.plain.train()
    micro_step(acc, ctx.plain, seeded(601, b, encoder_outputs=(enc,)), first=False, tag="encoder micro 1")
    Ld, Le = ctx.ocfg.decoder_layers, ctx.ocfg.encoder_layers
    buckets = eng.buckets()
    assert len(buckets) == Ld + Le + 3
    for i, (off, cnt) in enumerate(buckets):
        enc_side = Ld + 1 <= i <= Ld + 1 + Le
        if enc_side:    # (values, not bits: x + 0 turns a -0 into +0)
            assert torch.equal(eng.grads[off: off + cnt], first[off: off + cnt]), i
            assert float(eng.grad_stage[off: off + cnt].abs().max()) == 0.0, i
        elif i < Ld:
            assert not torch.equal(eng.grads[off: off + cnt], first[off: off + cnt]), i


def arenas(eng):
    return (eng.params, eng.exp_avg, eng.exp_avg_sq, eng.params_bf16)


def snapshot(eng):
    torch.cuda.synchronize()
    return [t.clone() for t in arenas(eng)]


def restore(eng, snap, steps):
    for t, s in zip(arenas(eng), snap):
        t.copy_(s)
    eng.step_count = steps
    eng.set_device_steps(steps)


def same_bits(a, b):
    return all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))


def optimizer_ordering(guarded):
    """Three accumulated micro-steps, then the overlapped step straight behind the last backward: every piece waits for its bucket's
    event only, which must lie behind that bucket's fold.  The non-overlapped step from restored state on a copy of the same gradients
    must give the same bits."""
    ocfg = G.tiny_config(dropout=0.1)
    model = build(ocfg, G.golden_state_dict(ocfg, seed=7)).train()
    eng = model._engine
    model.accumulate_gradients(True)
    kw = dict(max_grad_norm=1e-3, skip_nonfinite=True) if guarded else {}
    opt = AdamW(model.parameters(), lr=LR, **kw)
    opt.allow_overlap(True)
    assert opt.overlap, "KMB_ADAMW_OVERLAP=0 is set: the overlapped path cannot be tested"
    s0 = snapshot(eng)
    waits = []
    real_wait = eng.stream_wait_bucket
    eng.stream_wait_bucket = lambda i, s: (waits.append(i), real_wait(i, s))[1]
    try:
        opt.zero_grad()
        for k in range(3):
            eng.set_seed(700 + k)
            (run_fwd(model, micro_batch(k))[0] / 3).backward()
        grads = eng.grads.clone()                      # (enqueued behind backward on the caller's stream; the step below does not wait for it)
        opt.step()
    finally:
        del eng.stream_wait_bucket
    assert len(waits) >= len(eng.buckets()), "the overlapped path was not taken"
    over = snapshot(eng)
    assert torch.equal(bits(eng.grads), bits(grads)), "the optimizer wrote the gradients"
    assert not same_bits(over[:1], s0[:1])
    rec_over = eng.step_state() if guarded else None
    restore(eng, s0, 0)
    eng.grads.copy_(grads)
    opt.allow_overlap(False)
    opt.step()
    plain = snapshot(eng)
    assert same_bits(over, plain)
    if guarded:
        rec = eng.step_state()
        assert rec == rec_over and rec["applied"] == 1 and rec["steps"] == 1 and rec["coef"] < 1.0
        g = grads.double()
        assert abs(rec["norm"] - float(torch.sqrt((g * g).sum()))) <= 2e-7 * rec["norm"]
    else:
        assert eng.step_count == 1


@pytest.mark.parametrize("guarded", [True, False])
def test_g_overlapped_optimizer_waits_for_the_folds(guarded):
    optimizer_ordering(guarded)


@pytest.mark.parametrize("guarded", [True, False])
def test_g_overlapped_optimizer_without_a_side_stream(guarded, monkeypatch):
    """KMB_NO_SIDE_STREAM=1 is read when a handle first needs its side stream: a model built under it folds on the caller's stream"""
    monkeypatch.setenv("KMB_NO_SIDE_STREAM", "1")
    optimizer_ordering(guarded)


def distinct_batch(seed0, regions=5, event=6, label=9, enc_len=20, dec_len=10):
    """a one-sample batch without a repeated token id (module docstring): the first seed >= seed0 that gives one"""
    for seed in range(seed0, seed0 + 200):
        b = tiny_batch(regions=(regions,), event_lens=(event,), label_lens=(label,), enc_len=enc_len, dec_len=dec_len, seed=seed)
        ids = torch.cat([b["input_ids"].reshape(-1), b["decoder_input_ids"].reshape(-1)])
        ids = ids[(ids != 1) & (ids != G.TINY["img_feat_id"])]
        if len(set(ids.tolist())) == ids.numel():
            return b
    raise AssertionError("no batch without repeated tokens in 200 seeds")


def test_h_fine_tune_groups_micro_batches():
    from src.training import fine_tune
    ocfg = G.tiny_config(dropout=0.1)
    sd = G.golden_state_dict(ocfg, seed=7)
    shapes = [dict(), dict(regions=3, event=4, label=7, enc_len=16, dec_len=8), dict(regions=6, event=7, label=11, enc_len=24, dec_len=12),
              dict(), dict(regions=4, event=5, label=6, enc_len=18, dec_len=8)]
    loader = [distinct_batch(800 + 10 * i, **kw) for i, kw in enumerate(shapes)]
    lines = []
    logger = types.SimpleNamespace(info=lambda m, pad=False: lines.append(m))
    model = build(ocfg, sd).train()
    eng = model._engine
    opt = AdamW(model.parameters(), lr=LR, max_grad_norm=0.05, skip_nonfinite=True)
    mean = fine_tune(0, model, loader, opt, DEV, types.SimpleNamespace(amp=False, epochs=1, accumulation_steps=2), logger=logger)
    torch.cuda.synchronize()
    assert opt.step_state()["steps"] == 3 and opt.step_state()["skipped"] == 0
    loss_lines = [ln for ln in lines if ", Loss: " in ln]
    norm_lines = [ln for ln in lines if "Grad norm" in ln]
    assert [ln.split(",")[1].strip() for ln in loss_lines] == ["Step [%d/5]" % (i + 1) for i in range(5)]
    assert [ln.split(",")[1].strip() for ln in norm_lines] == ["Step [2/5]", "Step [4/5]", "Step [5/5]"]
    assert not eng.accumulating
    # the same through the API by hand: the same seeds and step numbers (two fresh engines), hence the same dropout masks
    twin = build(ocfg, sd).train()
    teng = twin._engine
    topt = AdamW(twin.parameters(), lr=LR, max_grad_norm=0.05, skip_nonfinite=True)
    twin.accumulate_gradients(True)
    losses = []
    for i, b in enumerate(loader):
        loss = run_fwd(twin, b)[0]
        if i % 2 == 0:
            topt.zero_grad()
        (loss / 2).backward()
        losses.append(loss.detach())
        if i % 2 == 1 or i == 4:
            topt.step()
    twin.accumulate_gradients(False)
    torch.cuda.synchronize()
    assert topt.step_state()["steps"] == 3
    want_mean = sum(float(x) for x in losses) / 5
    assert abs(mean - want_mean) <= 1e-6 * abs(want_mean)             # the unscaled losses, per micro-batch
    for got, want in zip(arenas(eng)[:3], arenas(teng)[:3]):
        worst = float((got - want).abs().max())
        print("[accum loop] fine_tune vs hand-written loop: worst difference %.3e" % worst)
        assert torch.allclose(got, want, atol=ATOL, rtol=RTOL)
    # a plain backward overwrites again
    eng.set_seed(9)
    run_fwd(model, loader[0])[0].backward()
    torch.cuda.synchronize()
    g0 = eng.grads.clone()
    eng.set_seed(9)
    run_fwd(model, loader[0])[0].backward()
    torch.cuda.synchronize()
    assert torch.equal(bits(eng.grads), bits(g0))                     # (no repeated token: the tied matrix is reproducible too)


def test_i_pretrain_groups_micro_batches():
    from src.training import pretrain
    sd = G.golden_state_dict(G.tiny_config(**PRE_KW), seed=33)
    loader = [distinct_pretrain_batch(1, 24, 16, 6, seed0=820, n_rel=2), distinct_pretrain_batch(1, 20, 12, 4, seed0=840, n_rel=2)]
    lines = []
    logger = types.SimpleNamespace(info=lambda m, pad=False: lines.append(m))
    model = pre_model(sd, dropout=0.1)
    eng = model._engine
    opt = AdamW(model.parameters(), lr=LR)
    before = eng.params.clone()
    pretrain(0, model, loader, opt, DEV, types.SimpleNamespace(amp=False, epochs=1, accumulation_steps=2), logger=logger)
    torch.cuda.synchronize()
    assert eng.step_count == 1 and len([ln for ln in lines if ", Loss: " in ln]) == 2 and not eng.accumulating
    assert not torch.equal(eng.params, before)
    twin = pre_model(sd, dropout=0.1)
    teng = twin._engine
    topt = AdamW(twin.parameters(), lr=LR)
    twin.accumulate_gradients(True)
    topt.zero_grad()
    for i, b in enumerate(loader):
        # (both engines count their training forwards from the same default seed: the same dropout masks)
        losses = twin(input_ids=b["input_ids"].to(DEV), image_features=[f.to(DEV) for f in b["image_features"]],
                      attention_mask=b["attention_mask"].to(DEV), decoder_input_ids=b["decoder_input_ids"].to(DEV),
                      decoder_attention_mask=b["decoder_attention_mask"].to(DEV), labels=b["labels"].to(DEV),
                      mrm_labels=b["mrm_labels"], mrm_mask=b["mrm_mask"], attribute_labels=b["attribute_labels"],
                      attribute_mask=b["attribute_mask"], relation_labels=b["relation_labels"])[0]
        (losses["loss"] / 2).backward()
    topt.step()
    torch.cuda.synchronize()
    for got, want in zip(arenas(eng)[:3], arenas(teng)[:3]):
        print("[accum loop] pretrain vs hand-written loop: worst difference %.3e" % float((got - want).abs().max()))
        assert torch.allclose(got, want, atol=ATOL, rtol=RTOL)


@pytest.mark.parametrize("mode", ["native", "torch"])
def test_j_no_sync_reduces_once_per_group(mode):
    import torch.distributed as dist
    from kmbart.parallel import DistributedDataParallel
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str({"native": 29561, "torch": 29562}[mode])
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    ddp = None
    try:
        ocfg = G.tiny_config(dropout=0.0)
        sd = G.golden_state_dict(ocfg, seed=7)
        batches = [to_dev(micro_batch(k)) for k in range(3)]
        # the unreduced total: the same three micro-steps without the wrapper
        ref = build(ocfg, sd).train()
        ref.accumulate_gradients(True)
        ref.zero_grad()
        for b in batches:
            ref.train_step_fwd_bwd(b, loss_scale=1.0 / 3.0)
        torch.cuda.synchronize()
        want = ref._engine.grads.clone()
        model = build(ocfg, sd).train()
        eng = model._engine
        ddp = DistributedDataParallel(model, device_ids=[0], reduce_single_rank=True, native=(mode == "native"))
        assert ddp.native == (mode == "native")
        opt = AdamW(model.parameters(), lr=LR)
        opt.allow_overlap(True)
        assert ddp.attach_optimizer(opt)
        model.accumulate_gradients(True)
        p0 = eng.params.clone()
        opt.zero_grad()
        assert ddp.comm_report()["steps_measured"] == 0
        with ddp.no_sync():
            for b in batches[:2]:
                ddp.train_step_fwd_bwd(b, loss_scale=1.0 / 3.0)     # twice, optimizer attached: no error, nothing exchanged, nothing stepped
            assert ddp.comm_report()["steps_measured"] == 0 and eng.step_count == 0
            assert torch.equal(eng.params, p0)
        ddp.train_step_fwd_bwd(batches[2], loss_scale=1.0 / 3.0)      # reduces the sum, and steps it piece by piece
        torch.cuda.synchronize()
        got = eng.grads.clone()
        assert ddp.comm_report()["steps_measured"] == 1 and eng.step_count == 1
        opt.step()
        torch.cuda.synchronize()
        assert eng.step_count == 1 and not torch.equal(eng.params, p0)
        # AVG over one rank is the identity (tests/test_dp_rccl_gpu.py's tolerance: bits, 1e-6 inside the tied matrix)
        lo, hi = tied_range(eng)
        same = got == want
        same[lo:hi] = True
        assert bool(same.all())
        assert torch.allclose(got[lo:hi], want[lo:hi], rtol=0, atol=1e-6)
        # outside no_sync a second backward without a step is still refused, with a message that names what works
        ddp.train_step_fwd_bwd(batches[0])
        with pytest.raises(RuntimeError, match="no_sync"):
            ddp.train_step_fwd_bwd(batches[0])
    finally:
        if ddp is not None:
            ddp.detach_optimizer()
        dist.destroy_process_group()
