"""GPU: training, generation and eval calls interleaved on ONE engine give what each call gives alone on a fresh engine.

Generation runs its encoder over buffers of its own workspace layout (engine_gen.cpp, EncoderBufs) and no longer borrows the training
layout's members; the status word (kmb_read_status) follows whichever call ran last.  Tiny configuration of test_model_gpu.py, b = 2.
Everything is compared bit for bit except the tied matrix's gradient, whose last bit is not run-to-run stable:
that one at test_model_gpu.py's gradient tolerance."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import goldenlib as G  # noqa: E402
from oracle.make_golden import tiny_batch  # noqa: E402  (batch builder only)
from test_model_gpu import DEV, GRAD_TOL, build, rel, run_fwd  # noqa: E402

TIED = "model.shared.weight"


def _tensors(x):
    if torch.is_tensor(x):
        return [x.detach().clone().cpu()]
    if isinstance(x, (tuple, list)):
        return [t for y in x for t in _tensors(y)]
    return []


def _train_step(model, b):
    model.train()
    model._engine.set_seed(123)
    loss = run_fwd(model, b)[0]
    loss.backward()
    torch.cuda.synchronize()
    return {"loss": _tensors(loss), "grads": {n: p.grad.detach().clone().cpu() for n, p in model.named_parameters()}}


def _generate(model, b, **kw):
    model.eval()
    out = model.generate(input_ids=b["input_ids"].to(DEV), image_features=[f.to(DEV) for f in b["image_features"]],
                         attention_mask=b["attention_mask"].to(DEV), max_length=6, return_scores=True, **kw)
    return {"out": _tensors(out), "status": model._engine.read_status()}


def _eval_hidden(model, b):
    model.eval()
    with torch.no_grad():
        return {"out": _tensors(run_fwd(model, b, output_hidden_states=True))}


def _same(got, ref, what):
    assert len(got) == len(ref) and len(ref) > 0, what
    for i, (a, r) in enumerate(zip(got, ref)):
        assert a.shape == r.shape and torch.equal(a, r), (what, i)


def _same_step(got, ref, what):
    _same(got["loss"], ref["loss"], what + " loss")
    assert got["grads"].keys() == ref["grads"].keys() and TIED in ref["grads"]
    for n, r in ref["grads"].items():
        if n == TIED:
            e = rel(got["grads"][n], r)
            print(f"[{what}] {n} gradient rel {e:.3e}")
            assert e < GRAD_TOL, (what, n, e)
        else:
            assert torch.equal(got["grads"][n], r), (what, n)


def test_interleaved_training_generation_and_eval_match_fresh_engines():
    ocfg = G.tiny_config()
    sd = G.golden_state_dict(ocfg)
    b = tiny_batch(seed=41)
    assert b["input_ids"].shape[0] == 2
    fresh = lambda: build(ocfg, sd, dropout=0.1)  # noqa: E731
    ref_step = _train_step(fresh(), b)
    ref_beam = _generate(fresh(), b, num_beams=3)
    ref_hidden = _eval_hidden(fresh(), b)
    ref_greedy = _generate(fresh(), b, num_beams=1)

    model = fresh()
    first = _train_step(model, b)
    beam = _generate(model, b, num_beams=3)            # (its read_status is step 3 of the sequence)
    hidden = _eval_hidden(model, b)
    greedy = _generate(model, b, num_beams=1)
    last = _train_step(model, b)

    _same_step(first, ref_step, "first step")
    _same(beam["out"], ref_beam["out"], "beam ids / scores")
    assert beam["status"] == ref_beam["status"] == 0
    _same(hidden["out"], ref_hidden["out"], "eval loss / hidden states")
    assert len(hidden["out"]) > 3   # loss, encoder states and the hidden states of both stacks
    _same(greedy["out"], ref_greedy["out"], "greedy ids / scores")
    assert greedy["status"] == ref_greedy["status"] == 0
    _same_step(last, ref_step, "last step")
    _same_step(last, first, "last step against the first")
