"""float64 restatement of the clipped / guarded optimizer step (kmbart.optim.AdamW(max_grad_norm=..., skip_nonfinite=...)):
the global L2 norm, torch.nn.utils.clip_grad_norm_'s coefficient, and the transformers-3.0.2 AdamW update under them with the
bias-correction step count FROZEN on a skipped step.  numpy only; shared by the CPU and the GPU tests."""
import math

import numpy as np


def global_norm(grads, grad_scale=1.0):
    """sqrt(sum (g * grad_scale)^2) over every array of `grads`, in float64."""
    total = 0.0
    for g in grads:
        x = np.asarray(g, dtype=np.float64).reshape(-1) * float(grad_scale)
        total += float(np.dot(x, x))
    return math.sqrt(total)   # (inf stays inf, NaN stays NaN)


def clip_coef(norm, max_norm):
    """min(1, max_norm / (norm + 1e-6)); max_norm None or <= 0: no clipping.  A NaN norm gives a NaN coefficient."""
    if max_norm is None or max_norm <= 0:
        return 1.0
    c = float(max_norm) / (norm + 1e-6)
    if c != c:
        return c
    return c if c < 1.0 else 1.0


class RefState:
    """The device record's counters."""

    def __init__(self, steps=0, skipped=0):
        self.steps, self.skipped = steps, skipped
        self.norm = self.coef = self.step_size = 0.0
        self.applied = 0


def decide(state, grads, lr, betas=(0.9, 0.999), correct_bias=True, max_norm=None, skip_nonfinite=False, grad_scale=1.0):
    """What the finish kernel decides: fills `state` and returns it."""
    norm = global_norm(grads, grad_scale)
    state.norm, state.coef = norm, clip_coef(norm, max_norm)
    if math.isfinite(norm) or not skip_nonfinite:
        state.steps += 1
        ss = float(lr)
        if correct_bias:
            ss = ss * math.sqrt(1.0 - betas[1] ** state.steps) / (1.0 - betas[0] ** state.steps)
        state.step_size, state.applied = ss, 1
    else:
        state.step_size, state.applied = 0.0, 0
        state.skipped += 1
    return state


def adamw_update(p, g, m, v, state, lr, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, grad_scale=1.0):
    """HF-3.0.2 AdamW.step on float64 arrays under a decided `state` (in place; untouched when the step is skipped):
    exp_avg = b1 exp_avg + (1 - b1) g;  exp_avg_sq = b2 exp_avg_sq + (1 - b2) g^2;  p -= step_size exp_avg / (sqrt(exp_avg_sq) + eps);
    p -= lr wd p, with g = grad * (grad_scale * coef)."""
    if not state.applied:
        return
    gr = np.asarray(g, dtype=np.float64) * (float(grad_scale) * state.coef)
    m *= betas[0]
    m += (1.0 - betas[0]) * gr
    v *= betas[1]
    v += (1.0 - betas[1]) * gr * gr
    p -= state.step_size * (m / (np.sqrt(v) + eps))
    if weight_decay > 0.0:
        p -= lr * weight_decay * p
