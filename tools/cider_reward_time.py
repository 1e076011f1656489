"""Times the CIDEr-D reward on the device (kmb_cider_reward, one launch per [B, L] id matrix) beside the same reward computed on the
host from ids.cpu() with dictionaries, on a synthetic corpus of VCG-like size.

    python tools/cider_reward_time.py [--items 240000] [--refs_per_item 5] [--batch 1024] [--out profiles/cider_reward_time.txt]

Corpus: `items` items with `refs_per_item` references each (default 1.2 M references) of 6-14 tokens drawn from a 50265-token
vocabulary with a heavy head (token = floor(V * u^3)), so that unigrams and bigrams repeat across items as words do.  Rows: a
reference of the row's item with up to three edits at L = 32; at L = 100 the same followed by random tokens up to 90-98 tokens
(the kernel's compare sweep and lookups grow with the row, whatever its score).  The host side is given every advantage: the
reference vectors and the idf of every n-gram of the batch are dictionaries built BEFORE the clock starts; it pays for ids.cpu(),
the token rule, the n-gram counts and the score of each row."""
import argparse
import math
import os
import sys
import time
from collections import Counter

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "km-bart_amd"))

from src.rewards import CiderReward, reward_tokens  # noqa: E402

PAD, BOS, EOS, V = 1, 0, 2, 50265


def corpus(n_items, per_item, rng):
    n = n_items * per_item
    lens = rng.integers(6, 15, size=n)
    tok = (3 + np.floor((V - 3) * rng.random(int(lens.sum())) ** 3)).astype(np.int64)
    refs = np.split(tok, np.cumsum(lens)[:-1])
    return [[refs[i * per_item + k].tolist() for k in range(per_item)] for i in range(n_items)]


def rows_for(groups, items, L, fill, rng):
    out = []
    for i in items:
        h = list(groups[i][int(rng.integers(len(groups[i])))])
        for _ in range(int(rng.integers(0, 4))):
            j = int(rng.integers(len(h)))
            h[j] = int(3 + (V - 3) * rng.random() ** 3)
        if fill:
            h += (3 + np.floor((V - 3) * rng.random(int(rng.integers(90, 99)) - len(h)) ** 3)).astype(np.int64).tolist()
        h = h[:L - 2]
        out.append([EOS] + h + [EOS] + [PAD] * (L - 2 - len(h)))
    return out


def pack(w):
    k = 0
    for t in w:
        k = (k << 16) | t
    return k


def ngrams(t, n):
    return Counter(tuple(t[j:j + n]) for j in range(len(t) - n + 1))


class HostCider:
    """the dictionary implementation: reference vectors of the batch's items and the idf of the batch's n-grams, from the tables"""

    def __init__(self, tables, items, rows):
        t = self.t = tables
        self.refs = {}
        for i in set(items):
            rs = []
            for r in range(int(t["item_ref_offsets"][i]), int(t["item_ref_offsets"][i + 1])):
                vec = []
                for n in range(4):
                    lo, hi = int(t["ref_ng_offsets"][4 * r + n]), int(t["ref_ng_offsets"][4 * r + n + 1])
                    vec.append((dict(zip(t["ref_keys"][lo:hi].tolist(), t["ref_w"][lo:hi].tolist())), float(t["ref_norm"][r, n])))
                rs.append((int(t["ref_len"][r]), vec))
            self.refs[i] = rs
        self.idf, off, miss = {}, t["df_offsets"], float(t["idf_miss"])
        for row in rows:
            tok = reward_tokens(row, PAD, BOS, EOS)
            for n in range(1, 5):
                keys = t["df_keys"][off[n - 1]:off[n]]
                for w in ngrams(tok, n):
                    k = pack(w)
                    at = int(np.searchsorted(keys, np.uint64(k)))
                    self.idf[(n, k)] = float(t["df_idf"][off[n - 1] + at]) if at < len(keys) and int(keys[at]) == k else miss

    def score(self, ids_cpu, items, sigma=6.0, variant="D"):
        out = []
        for row, i in zip(ids_cpu.tolist(), items):
            h = reward_tokens(row, PAD, BOS, EOS)
            refs = self.refs[i]
            gh, nh = [], []
            for n in range(1, 5):
                g = {pack(w): c * self.idf[(n, pack(w))] for w, c in ngrams(h, n).items()}
                gh.append(g)
                nh.append(math.sqrt(sum(v * v for v in g.values())))
            total = 0.0
            for length, vec in refs:
                s = 0.0
                for n in range(4):
                    gr, nr = vec[n]
                    if nh[n] > 0 and nr > 0:
                        s += sum((min(g, gr.get(k, 0.0)) if variant == "D" else g) * gr.get(k, 0.0) for k, g in gh[n].items()) / (nh[n] * nr)
                total += (math.exp(-((len(h) - length) ** 2) / (2 * sigma * sigma)) if variant == "D" else 1.0) * 0.25 * s
            out.append(10.0 / len(refs) * total if refs and h else 0.0)
        return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--items", type=int, default=240000)
    p.add_argument("--refs_per_item", type=int, default=5)
    p.add_argument("--batch", type=int, default=1024)
    p.add_argument("--launches", type=int, default=200, help="back-to-back launches of a timed window")
    p.add_argument("--windows", type=int, default=7)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "cider_reward_time.txt"))
    a = p.parse_args()
    rng = np.random.default_rng(17)
    t0 = time.time()
    groups = corpus(a.items, a.refs_per_item, rng)
    rew = CiderReward(groups, V, PAD, BOS, EOS, device="cuda:0")
    lines = ["CIDEr-D reward over token ids: %d items x %d references = %d references, %d reference n-grams, %d df entries, "
             "tables %.1f MB on the device, built on the host in %.1f s" % (a.items, a.refs_per_item, rew.n_refs, rew.n_ref_entries,
                                                                          len(rew.tables["df_keys"]), rew.table_bytes() / 2 ** 20, time.time() - t0)]
    items = rng.integers(0, a.items, size=a.batch).tolist()
    items_dev = torch.tensor(items, dtype=torch.int32, device="cuda:0")
    for L, fill in ((32, False), (100, True)):
        rows = rows_for(groups, items, L, fill, rng)
        ids = torch.tensor(rows, dtype=torch.int64, device="cuda:0")
        for _ in range(10):
            out = rew.reward(ids, items_dev)
        torch.cuda.synchronize()
        times = []                                   # per-launch time of a WINDOW of back-to-back launches between one event pair:
        for _ in range(a.windows):                   # the stream stays busy, so the host's enqueue gap is not in the figure
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                out = rew.reward(ids, items_dev)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3 / a.launches)
        times.sort()
        host = HostCider(rew.tables, items, rows)
        h0 = time.perf_counter()
        want = host.score(ids.cpu(), items)
        host_ms = (time.perf_counter() - h0) * 1e3
        got = out.double().cpu().tolist()
        rel = [abs(g - w) / w for g, w in zip(got, want) if w > 1e-20]
        absolute = max(abs(g - w) for g, w in zip(got, want))
        rew.variant = "plain"                        # the same rows without the length penalty: scores that do not underflow at L = 100
        got_p = rew.reward(ids, items_dev).double().cpu().tolist()
        rew.variant = "D"
        want_p = host.score(ids.cpu(), items, variant="plain")
        rel_p = [abs(g - w) / w for g, w in zip(got_p, want_p) if w > 1e-20]
        mean_len = sum(len(reward_tokens(r, PAD, BOS, EOS)) for r in rows) / len(rows)
        lines.append("B = %d, L = %3d (mean %.1f scored tokens, mean reward %.3f): device %.1f us per launch (median of %d windows of %d "
                     "back-to-back launches; min %.1f, max %.1f); host ids.cpu() + dictionaries %.1f ms; device against host: largest "
                     "relative difference %.1e over the %d rows scoring > 1e-20, largest absolute difference %.1e over all %d rows%s; "
                     "plain CIDEr on the same rows: largest relative difference %.1e over %d rows"
                     % (a.batch, L, mean_len, sum(got) / len(got), times[len(times) // 2], len(times), a.launches, times[0], times[-1],
                        host_ms, max(rel, default=0.0), len(rel), absolute, len(got),
                        "" if rel else " (every penalty underflows at these lengths: both sides score 0 or a denormal, nothing relative to compare)",
                        max(rel_p, default=0.0), len(rel_p)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
