"""One greedy beam-search step with generate()'s score processors, on the host (the rule of kmb_beam_step_processed, DESIGN.md
6n): float64 log_softmax of the unedited rows, rounded to fp32; tests/process_ref.py's edit of those log-probabilities (which
tokens are penalised, which banned); the min_length ban; + the beam scores; per batch item a stable sort of its num_beams * V
scores (value descending, beam * V + token ascending); the next beams as the reference's bookkeeping sends them on (in candidate
order, the first num_beams whose token is not EOS).  tests/test_beam_process_cpu.py pins it to the host beam loop's arithmetic."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import process_ref  # noqa: E402


def scores(logits, rows, add, V, penalty=1.0, ngram=0, bad_words=None, ban_token=-1, force_token=-1):
    """The edited scores [R, V] fp32 of one step: logits numpy [R, >= V], rows R token lists, add fp32 [R]."""
    x = np.asarray(logits)[:, :V].astype(np.float64)
    if force_token >= 0:   # adjust_logits_during_generation: every other logit is -inf
        keep = x[:, force_token].copy()
        x[:] = -np.inf
        x[:, force_token] = keep
    m = x.max(axis=1, keepdims=True)
    lse = m + np.log(np.exp(x - m).sum(axis=1, keepdims=True))
    s = (x - lse).astype(np.float32)
    process_ref.process(s, rows, V, penalty, ngram, bad_words)
    if ban_token >= 0:
        s[:, ban_token] = -np.inf
    return s + np.asarray(add, dtype=np.float32)[:, None]


def step(logits, rows, add, B, nb, V, k, penalty=1.0, ngram=0, bad_words=None, ban_token=-1, eos=-1, force_token=-1, extra=1):
    """-> dict: s [R, V]; val / idx [B, k + extra]: the item's best candidates in order (idx = beam * V + token);
    next_scores / next_tokens / next_beam_idx [R]; ids_out: the R next histories (token lists)."""
    s = scores(logits, rows, add, V, penalty, ngram, bad_words, ban_token, force_token)
    flat = s.reshape(B, nb * V)
    order = np.argsort(-flat, axis=1, kind="stable")[:, :k + extra]
    val = np.take_along_axis(flat, order, axis=1)
    nscore, ntok, nidx, ids_out = [], [], [], []
    for b in range(B):
        n = 0
        for j in range(k):
            beam, tok = divmod(int(order[b, j]), V)
            if tok == eos or n == nb:
                continue
            nscore.append(val[b, j]); ntok.append(tok); nidx.append(b * nb + beam)
            ids_out.append(list(rows[b * nb + beam]) + [tok])
            n += 1
        assert n == nb, "fewer than num_beams candidates without EOS"
    return dict(s=s, val=val, idx=order, next_scores=np.array(nscore, dtype=np.float32), next_tokens=np.array(ntok, dtype=np.int64),
                next_beam_idx=np.array(nidx, dtype=np.int32), ids_out=ids_out)
