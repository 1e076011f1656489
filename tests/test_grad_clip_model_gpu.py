"""GPU: kmbart.optim.AdamW(max_grad_norm=..., skip_nonfinite=...) on the tiny model (batch 2, ragged): the clipped step against
tests/clip_ref.py, the overlapped path against the plain one bit for bit, the skipped step, gradient scaling, checkpoints, and the step
count's survival of a poisoned workspace.

Bit-for-bit comparisons are made on ONE gradient arena: the optimizer never writes the gradients, so a second step from restored
parameters / moments sees exactly the bytes the first one saw (two backward passes do not: the tied matrix's token-gradient scatter
uses fp32 atomics and differs run to run in the last bit, tests/test_dp_rccl_gpu.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "km-bart_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import clip_ref  # noqa: E402
from oracle import goldenlib as G  # noqa: E402
from oracle.make_golden import tiny_batch  # noqa: E402
from kmbart.optim import AdamW  # noqa: E402
from test_model_gpu import build  # noqa: E402

DEV = "cuda:0"
LR = 1e-3
ATOL, RTOL = 2e-7, 1e-6     # tests/test_ops_gpu.py's AdamW tolerance (the same fp32 arithmetic)
RECORD = ("norm", "coef", "step_size", "applied", "steps", "skipped")


def device_batch(seed=5):
    b = tiny_batch(seed=seed)
    batch = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in b.items()}
    batch["image_features"] = [f.to(DEV) for f in b["image_features"]]
    return batch


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


def norm64(eng, scale=1.0):
    g = eng.grads.cpu().numpy().astype(np.float64) * scale
    return float(np.sqrt(np.dot(g, g)))


class Ctx:
    pass


@pytest.fixture(scope="module")
def ctx():
    """One model, one batch, its initial state, and path (a): a step with max_grad_norm far above the norm."""
    c = Ctx()
    ocfg = G.tiny_config(dropout=0.0)
    c.ocfg, c.sd = ocfg, G.golden_state_dict(ocfg, seed=7)
    c.model = build(ocfg, c.sd).train()
    c.eng = c.model._engine
    c.batch = device_batch()
    c.s0 = snapshot(c.eng)
    opt = AdamW(c.model.parameters(), lr=LR, max_grad_norm=1e9)
    c.model.train_step_fwd_bwd(c.batch)
    opt.step()
    c.state_a = opt.step_state()
    c.after_a = snapshot(c.eng)
    c.grads_a = c.eng.grads.clone()
    c.norm_a = norm64(c.eng)
    return c


def test_a_unclipped_step_equals_the_plain_optimizer(ctx):
    """coef == 1.0 exactly; the parameters equal the host-state optimizer's on the same gradients within the op tolerance.  The two can
    differ in the last bit where the device's pow() and the host's differ in step_size: the count is printed, not bounded."""
    st = ctx.state_a
    assert st["coef"] == 1.0 and st["applied"] == 1 and st["steps"] == 1 and st["skipped"] == 0
    assert abs(st["norm"] - ctx.norm_a) <= 2e-7 * ctx.norm_a
    restore(ctx.eng, ctx.s0, 0)
    plain = AdamW(ctx.model.parameters(), lr=LR)
    plain.step()                       # the gradients of the fixture's backward are still in the arena
    after = snapshot(ctx.eng)
    assert ctx.eng.step_count == 1
    for got, want in zip(ctx.after_a[:3], after[:3]):
        assert torch.allclose(got, want, atol=ATOL, rtol=RTOL)
    differ = int((ctx.after_a[0] != after[0]).sum())
    print("[clip a] parameters differing from the plain optimizer: %d of %d" % (differ, after[0].numel()))


def test_b_clipped_step_overlapped_equals_plain_and_the_reference(ctx):
    eng, model = ctx.eng, ctx.model
    max_norm = 0.5 * ctx.norm_a
    opt = AdamW(model.parameters(), lr=LR, max_grad_norm=max_norm)
    opt.allow_overlap(True)
    assert opt.overlap, "KMB_ADAMW_OVERLAP=0 is set: the overlapped path cannot be tested"
    restore(eng, ctx.s0, 0)
    waits = []
    real_wait = eng.stream_wait_bucket
    eng.stream_wait_bucket = lambda i, s: (waits.append(i), real_wait(i, s))[1]
    try:
        model.train_step_fwd_bwd(ctx.batch)
        opt.step()                     # each piece's sum behind its bucket's event, on the side stream
    finally:
        del eng.stream_wait_bucket
    assert len(waits) >= len(eng.buckets()), "the overlapped path was not taken"
    over, rec_over = snapshot(eng), eng.step_state()
    # the norm: the double partial sums against numpy float64 (n * 2^-53 bounds the accumulation: 1e-9); the record's fp32 value
    # is that norm rounded once
    ref_norm = norm64(eng)
    _, nslots = eng.step_pieces([(off, cnt) for _, off, cnt in opt._engine_ranges(opt.param_groups[0])])
    total = float(eng._step_buf[64: 64 + 8 * nslots].view(torch.float64).sum().cpu())
    print("[clip b] norm %.17g reference %.17g" % (np.sqrt(total), ref_norm))
    assert abs(np.sqrt(total) - ref_norm) <= 1e-9 * ref_norm
    assert abs(np.float32(float(opt.grad_norm)) - np.float32(ref_norm)) <= np.spacing(np.float32(ref_norm))
    assert rec_over["coef"] < 1.0 and abs(rec_over["coef"] - clip_ref.clip_coef(ref_norm, max_norm)) <= 2e-7
    # parameters and moments against the float64 restatement
    g = eng.grads.cpu().numpy()
    p = ctx.s0[0].cpu().numpy().astype(np.float64)
    m, v = np.zeros_like(p), np.zeros_like(p)
    st = clip_ref.decide(clip_ref.RefState(), [g], LR, max_norm=max_norm)
    clip_ref.adamw_update(p, g, m, v, st, LR)
    for got, want in zip(over[:3], (p, m, v)):
        assert np.allclose(got.cpu().numpy(), want, atol=ATOL, rtol=RTOL)
    assert torch.equal(over[3][: eng.n], over[0].to(torch.bfloat16))
    # the plain path on the same gradients: the same pieces into the same slots, hence the same bits
    restore(eng, ctx.s0, 0)
    opt.allow_overlap(False)
    opt.step()
    plain, rec_plain = snapshot(eng), eng.step_state()
    assert same_bits(over, plain)
    assert [rec_over[k] for k in RECORD] == [rec_plain[k] for k in RECORD]
    ctx.after_b, ctx.max_norm_b = over, max_norm


def test_c_nonfinite_step_is_skipped_and_leaves_no_trace(ctx):
    eng, model = ctx.eng, ctx.model
    max_norm = 0.5 * ctx.norm_a
    opt = AdamW(model.parameters(), lr=LR, max_grad_norm=max_norm, skip_nonfinite=True)
    restore(eng, ctx.s0, 0)
    model.train_step_fwd_bwd(ctx.batch)
    opt.step()
    s1 = snapshot(eng)
    assert opt.step_state()["steps"] == 1
    # the bad step
    model.train_step_fwd_bwd(ctx.batch)
    grad = dict(model.named_parameters())["model.decoder.layers.1.fc1.weight"].grad
    grad[3, 5] = float("inf")
    opt.step()
    assert same_bits(snapshot(eng), s1)
    bad = opt.step_state()
    assert bad["applied"] == 0 and bad["skipped"] == 1 and bad["steps"] == 1 and np.isinf(bad["norm"])
    # the next ordinary step ...
    model.train_step_fwd_bwd(ctx.batch)
    opt.step()
    after, rec = snapshot(eng), eng.step_state()
    g3 = eng.grads.clone()
    assert rec["applied"] == 1 and rec["steps"] == 2 and rec["skipped"] == 1
    # ... on a twin that never saw the bad one: the state after step 1, the same gradients
    twin = build(ctx.ocfg, ctx.sd).train()
    teng = twin._engine
    topt = AdamW(twin.parameters(), lr=LR, max_grad_norm=max_norm, skip_nonfinite=True)
    restore(teng, s1, 1)
    teng.grads.copy_(g3)
    topt.step()
    trec = teng.step_state()
    assert same_bits(snapshot(teng), after)
    assert trec["skipped"] == 0 and [trec[k] for k in RECORD[:5]] == [rec[k] for k in RECORD[:5]]


def test_d_loss_scale_folded_into_grad_scale_gives_the_same_record(ctx):
    """backward(loss_scale=1024) with grad_scale = 1 / 1024: powers of two are exact, so the record -- and every parameter and moment --
    is, bit for bit, the one of the unscaled gradients with grad_scale = 1.  "The unscaled gradients" are the scaled arena times 2^-10
    (exact): a second, unscaled backward pass is NOT bit-identical to the first (measured: it is not; the token-gradient scatter's fp32
    atomics), so its record is compared at 1e-6 relative -- ten times the 6e-8 per element that a reordered fp32 sum can move."""
    eng, model = ctx.eng, ctx.model
    opt = AdamW(model.parameters(), lr=LR, max_grad_norm=0.5 * ctx.norm_a, skip_nonfinite=True)
    restore(eng, ctx.s0, 0)
    model.train_step_fwd_bwd(ctx.batch, loss_scale=1024.0)
    opt.grad_scale = 1.0 / 1024.0
    opt.step()
    scaled, rec_scaled = snapshot(eng), eng.step_state()
    assert float(eng.grads.abs().max()) > 10.0 * float(ctx.grads_a.abs().max())      # the arena really holds scaled gradients
    restore(eng, ctx.s0, 0)
    eng.grads.mul_(1.0 / 1024.0)
    opt.grad_scale = 1.0
    opt.step()
    plain, rec_plain = snapshot(eng), eng.step_state()
    assert [rec_scaled[k] for k in RECORD] == [rec_plain[k] for k in RECORD]
    assert same_bits(scaled, plain)
    # a separate, unscaled backward pass
    restore(eng, ctx.s0, 0)
    model.train_step_fwd_bwd(ctx.batch)
    opt.step()
    rec_other = eng.step_state()
    print("[clip d] scaled %s | separate unscaled backward %s" % (rec_scaled, rec_other))
    for k in ("norm", "coef", "step_size"):
        assert abs(rec_other[k] - rec_scaled[k]) <= 1e-6 * abs(rec_scaled[k])
    assert [rec_other[k] for k in RECORD[3:]] == [rec_scaled[k] for k in RECORD[3:]]


def test_e_state_dict_round_trip_keeps_the_device_step_count(ctx):
    eng, model = ctx.eng, ctx.model
    opt = AdamW(model.parameters(), lr=LR, skip_nonfinite=True)
    restore(eng, ctx.after_a, 7)
    eng.step_count = 0                 # the host count is NOT the authority while an option is on
    sd = opt.state_dict()
    assert sd["step"] == [7]
    restore(eng, ctx.s0, 0)
    opt2 = AdamW(model.parameters(), lr=LR, max_grad_norm=1.0)
    opt2.load_state_dict(sd)
    assert opt2.step_state()["steps"] == 7
    assert torch.equal(eng.exp_avg, ctx.after_a[1]) and torch.equal(eng.exp_avg_sq, ctx.after_a[2])
    # the next step is step 8: its step size says so
    eng.grads.copy_(ctx.grads_a)
    opt2.step()
    r = eng.step_state()
    want = clip_ref.decide(clip_ref.RefState(steps=7), [ctx.grads_a.cpu().numpy()], LR, max_norm=1.0)
    assert r["steps"] == 8 and abs(r["step_size"] - want.step_size) <= 2e-7 * want.step_size


def test_h_first_guarded_step_continues_the_host_step_count(ctx):
    """An engine that took plain steps gets a guarded, overlapped optimizer: the first bind copies the host's count to the device on the
    caller's stream, and the side stream's finish launch is ordered behind that write -- the first guarded step is step 3, not step 1."""
    model = build(ctx.ocfg, ctx.sd).train()
    eng = model._engine
    plain = AdamW(model.parameters(), lr=LR)
    for _ in range(2):
        model.train_step_fwd_bwd(ctx.batch)
        plain.step()
    assert eng.step_count == 2
    opt = AdamW(model.parameters(), lr=LR, max_grad_norm=1e9)
    opt.allow_overlap(True)
    model.train_step_fwd_bwd(ctx.batch)
    opt.step()
    r = eng.step_state()
    want = clip_ref.decide(clip_ref.RefState(steps=2), [eng.grads.cpu().numpy()], LR, max_norm=1e9)
    assert r["steps"] == 3 and r["applied"] == 1 and abs(r["step_size"] - want.step_size) <= 2e-7 * want.step_size


_POISON_CHILD = r"""
import json, os, sys
root = sys.argv[1]
for p in (root, os.path.join(root, "km-bart_amd"), os.path.join(root, "tests")):
    sys.path.insert(0, p)
import torch
from oracle import goldenlib as G
from kmbart.optim import AdamW
from test_model_gpu import build
from test_grad_clip_model_gpu import device_batch
ocfg = G.tiny_config(dropout=0.0)
model = build(ocfg, G.golden_state_dict(ocfg, seed=7)).train()
opt = AdamW(model.parameters(), lr=1e-3, max_grad_norm=1.0, skip_nonfinite=True)
batch = device_batch()
losses = []
for _ in range(2):
    losses.append(float(model.train_step_fwd_bwd(batch)))
    opt.step()
st = opt.step_state()
st["losses"] = losses
st["poison"] = os.environ.get("KMB_POISON")
print("CLIP_POISON " + json.dumps(st))
"""


def test_f_step_count_survives_a_poisoned_workspace(tmp_path):
    """KMB_POISON=1 fills the workspace with 0xFF before every forward: the record lives in a buffer of its own, so two steps count two."""
    script = tmp_path / "poison_child.py"
    script.write_text(_POISON_CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, KMB_POISON="1"))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    line = [l for l in r.stdout.splitlines() if l.startswith("CLIP_POISON ")]
    assert line, r.stdout[-1500:]
    st = json.loads(line[0][len("CLIP_POISON "):])
    assert st["steps"] == 2 and st["skipped"] == 0 and st["applied"] == 1
    assert st["poison"] == "1" and all(np.isfinite(x) and x > 0 for x in st["losses"])


def test_g_one_rank_data_parallel_declines_the_fused_tail(ctx):
    """A one-rank DistributedDataParallel with attach_optimizer: the per-piece fused tail is declined, the wrapper all-reduces as without an
    optimizer, and step() clips the reduced gradients -- path (b)'s result (AVG over one rank is the identity; the tied matrix's gradient
    differs between two backward passes in the last bit, hence the op tolerance and not bits)."""
    import torch.distributed as dist
    from kmbart.parallel import DistributedDataParallel
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = "29551"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        model = build(ctx.ocfg, ctx.sd).train()
        eng = model._engine
        ddp = DistributedDataParallel(model, device_ids=[0], reduce_single_rank=True)
        max_norm = 0.5 * ctx.norm_a
        opt = AdamW(model.parameters(), lr=LR, max_grad_norm=max_norm)
        opt.allow_overlap(True)
        assert ddp.attach_optimizer(opt)
        ddp.train_step_fwd_bwd(ctx.batch)
        assert not getattr(opt, "_fused_pending", False) and eng.step_count == 0
        opt.step()
        rec = opt.step_state()
        after = snapshot(eng)
        assert rec["steps"] == 1 and rec["applied"] == 1 and rec["coef"] < 1.0
        ref_norm = norm64(eng)
        assert abs(np.float32(rec["norm"]) - np.float32(ref_norm)) <= np.spacing(np.float32(ref_norm))
        g = eng.grads.cpu().numpy()
        p = ctx.s0[0].cpu().numpy().astype(np.float64)
        m, v = np.zeros_like(p), np.zeros_like(p)
        st = clip_ref.decide(clip_ref.RefState(), [g], LR, max_norm=max_norm)
        clip_ref.adamw_update(p, g, m, v, st, LR)
        for got, want in zip(after[:3], (p, m, v)):
            assert np.allclose(got.cpu().numpy(), want, atol=ATOL, rtol=RTOL)
        # path (b)'s parameters, as tests/test_dp_rccl_gpu.py compares two runs: the op tolerance, 1e-5 inside the tied matrix
        assert hasattr(ctx, "after_b"), "path (b) has not run"
        off, rows, cols = eng.index["model.shared.weight"]
        close = torch.isclose(after[0], ctx.after_b[0], atol=ATOL, rtol=RTOL)
        close[off: off + rows * cols] = True
        assert bool(close.all())
        assert torch.allclose(after[0][off: off + rows * cols], ctx.after_b[0][off: off + rows * cols], rtol=0, atol=1e-5)
    finally:
        ddp.detach_optimizer() if "ddp" in locals() else None
        dist.destroy_process_group()
