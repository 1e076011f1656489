"""The rule of kmb_logits_process (csrc/logits_process.hip), row by row on the host: which tokens of a row are penalised (the
first occurrence of each), which are banned (window compare for the n-grams, tail compare for the bad words), and the edit of
a numpy fp32 buffer.  tests/test_logits_process_cpu.py pins it to _postprocess_next_token_scores; it knows nothing of torch."""
import numpy as np


def kept(row, V):
    """The row as the kernel holds it: tokens outside [0, V) are dropped."""
    return [int(x) for x in row if 0 <= int(x) < V]


def penalised(row):
    """Position j acts only when no i < j holds the same token: every distinct token once, in order of first appearance."""
    return [x for j, x in enumerate(row) if all(row[i] != x for i in range(j))]


def banned(row, n_rows, ngram, bad_words, V):
    """The set of tokens of one row (already `kept`) that phase B sets to -inf."""
    t = len(row)
    out = set()
    if ngram > 0 and t + 1 >= ngram:
        tail = t + 1 - ngram
        for j in range(0, t - ngram + 1):
            if all(row[j + k] == row[tail + k] for k in range(ngram - 1)):
                out.add(row[j + ngram - 1])
    for seq in bad_words or []:
        head, last = list(seq[:-1]), int(seq[-1])
        if not 0 <= last < V:
            continue
        h = len(head)
        if h == 0 or (h <= n_rows and h <= t and all(row[t - h + k] == head[k] for k in range(h))):
            out.add(last)
    return out


def penalise(v, p):
    """fp32: v < 0 ? v * p : v * (1 / p), the reciprocal rounded to fp32 once."""
    p = np.float32(p)
    inv = np.float32(1.0) / p
    v = np.float32(v)
    return v * p if v < 0 else v * inv


def process(scores, rows, V, penalty=1.0, ngram=0, bad_words=None):
    """Edits `scores` (numpy fp32 [R, ld]) in place from rows (R token lists): phase A, then phase B."""
    R = len(rows)
    for r, raw in enumerate(rows):
        row = kept(raw, V)
        if penalty != 1.0:
            for x in penalised(row):
                scores[r, x] = penalise(scores[r, x], penalty)
        for x in banned(row, R, ngram, bad_words, V):
            scores[r, x] = -np.inf
    return scores
