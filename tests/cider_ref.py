"""The CIDEr / CIDEr-D reward of src/rewards.py restated with dictionaries in float64, over token lists: once from the raw
groups (checks build_cider_tables) and once from the built tables (checks the kernel, so that the tables' float32 rounding is
not part of the kernel's error).  Also the seeded corpus and hypothesis recipe the CPU and GPU tests share.

Definition (the issue's text): N items, item i with m_i references; df_n(w) = items with a reference holding n-gram w;
idf_n(w) = log N - log max(1, df_n(w)); g_x,n(w) = count_x(w) idf_n(w);
s_n(h, r) = sum_{w in h} num / (||g_h,n|| ||g_r,n||), 0 when a norm is 0; num = min(g_h, g_r) g_r (D) or g_h g_r (plain);
pen = exp(-(L_h - L_r)^2 / (2 sigma^2)) (D) or 1; score = (10 / m_i) sum_r pen 1/4 sum_n s_n, 0 when m_i = 0.

Bound of a score computed in fp32: score * (4 L_h + m + 24) * 2^-24.  All summands are non-negative, so the relative error of
a sum is at most the number of roundings on the longest path times 2^-24: at most 4 L_h additions over the n-grams of the four
orders, m over the references, and 24 for the rest of a term's path -- count * idf, the square, sqrt and product of the norms,
min, two multiplications, the division, the penalty's argument (its error enters exp multiplied by |argument|: the recipe keeps
|L_h - L_r| small where the penalty is not 0 outright) and a correctly-rounded-to-1-ulp expf, 1/4 and 10 / m."""
import math
import random
from collections import Counter

import numpy as np

ORDERS = 4
EPS24 = 2.0 ** -24
HEADROOM = 0.5        # the project's rule: a measured error uses at most half of its bound


def ngrams(tokens, n):
    return Counter(tuple(tokens[j:j + n]) for j in range(len(tokens) - n + 1))


def pack(w):
    key = 0
    for t in w:
        key = (key << 16) | int(t)
    return key


def bound(score, len_h, m):
    return score * (4 * len_h + m + 24) * EPS24


def _score(hyp, refs, idf_of, variant, sigma, ref_vec=None):
    """refs: list of (length, [per order: (dict n-gram -> g_r, norm)]) when ref_vec is None, else token lists"""
    m = len(refs)
    if m == 0 or len(hyp) == 0:
        return 0.0
    gh, nh = [], []
    for n in range(1, ORDERS + 1):
        g = {w: c * idf_of(n, w) for w, c in ngrams(hyp, n).items()}
        gh.append(g)
        nh.append(math.sqrt(sum(v * v for v in g.values())))
    total = 0.0
    for length, vecs in refs:
        s = 0.0
        for n in range(ORDERS):
            gr, nr = vecs[n]
            if nh[n] == 0.0 or nr == 0.0:
                continue
            num = 0.0
            for w, g in gh[n].items():
                r = gr.get(w, 0.0)
                num += (min(g, r) * r) if variant == "D" else g * r
            s += num / (nh[n] * nr)
        pen = math.exp(-((len(hyp) - length) ** 2) / (2.0 * sigma * sigma)) if variant == "D" else 1.0
        total += pen * 0.25 * s
    return 10.0 / m * total


class RawReference:
    """from the raw groups: everything in float64"""

    def __init__(self, groups):
        self.groups = groups
        self.N = len(groups)
        self.df = [Counter() for _ in range(ORDERS)]
        for g in groups:
            for n in range(1, ORDERS + 1):
                seen = set()
                for r in g:
                    seen.update(ngrams(r, n))
                self.df[n - 1].update(seen)

    def idf(self, n, w):
        return math.log(self.N) - math.log(max(1, self.df[n - 1].get(w, 0)))

    def ref_vectors(self, r):
        out = []
        for n in range(1, ORDERS + 1):
            g = {w: c * self.idf(n, w) for w, c in ngrams(r, n).items()}
            out.append((g, math.sqrt(sum(v * v for v in g.values()))))
        return out

    def score(self, hyp, item, variant="D", sigma=6.0):
        refs = [(len(r), self.ref_vectors(r)) for r in self.groups[item]] if 0 <= item < self.N else []
        return _score(hyp, refs, self.idf, variant, sigma)


class TableReference:
    """from the tables of build_cider_tables: their float32 values, taken as exact, combined in float64"""

    def __init__(self, t):
        self.t = t
        self.N = int(t["n_items"])
        self.idf_miss = float(t["idf_miss"])
        off = t["df_offsets"]
        self.idf_tab = [{int(k): float(v) for k, v in zip(t["df_keys"][off[n]:off[n + 1]], t["df_idf"][off[n]:off[n + 1]])}
                        for n in range(ORDERS)]

    def idf(self, n, w):
        return self.idf_tab[n - 1].get(pack(w), self.idf_miss)

    def refs_of(self, item):
        t = self.t
        if not 0 <= item < self.N:
            return []
        out = []
        for r in range(int(t["item_ref_offsets"][item]), int(t["item_ref_offsets"][item + 1])):
            vecs = []
            for n in range(ORDERS):
                lo, hi = int(t["ref_ng_offsets"][4 * r + n]), int(t["ref_ng_offsets"][4 * r + n + 1])
                vecs.append(({int(k): float(v) for k, v in zip(t["ref_keys"][lo:hi], t["ref_w"][lo:hi])}, float(t["ref_norm"][r, n])))
            out.append((int(t["ref_len"][r]), vecs))
        return out

    def score(self, hyp, item, variant="D", sigma=6.0):
        refs = [(length, [(_Packed(g), nr) for g, nr in vecs]) for length, vecs in self.refs_of(item)]
        return _score(hyp, refs, self.idf, variant, sigma)

    def score_fp32(self, hyp, item, variant="D", sigma=6.0):
        """the same from the tables in float32 with SEQUENTIAL sums (the worst order a kernel could take)"""
        f = np.float32
        refs = self.refs_of(item)
        m = len(refs)
        if m == 0 or len(hyp) == 0:
            return 0.0
        gh, nh = [], []
        for n in range(1, ORDERS + 1):
            g = {pack(w): f(c) * f(self.idf(n, w)) for w, c in ngrams(hyp, n).items()}
            sq = f(0)
            for v in g.values():
                sq = f(sq + f(v * v))
            gh.append(g)
            nh.append(f(np.sqrt(sq)))
        total = f(0)
        inv = f(-1.0 / (2.0 * sigma * sigma))
        for length, vecs in refs:
            s = f(0)
            for n in range(ORDERS):
                gr, nr = vecs[n]
                nr = f(nr)
                if not nh[n] > 0 or not nr > 0:
                    continue
                num = f(0)
                for w, g in gh[n].items():
                    r = f(gr.get(w, 0.0))
                    num = f(num + (f(min(g, r) * r) if variant == "D" else f(g * r)))
                s = f(s + f(num / f(nh[n] * nr)))
            d = len(hyp) - length
            pen = f(np.exp(f(f(d * d) * inv))) if variant == "D" else f(1)
            total = f(total + f(pen * f(f(0.25) * s)))
        return float(f(total * f(f(10) / f(m))))


class _Packed(dict):
    """a reference vector keyed by packed keys, looked up by n-gram tuples"""

    def get(self, w, default=0.0):
        return dict.get(self, pack(w), default)


# ------------------------------------------------------------------------------------------------ the shared corpus and cases
V_BIG = 65536
REF_COUNTS = (1, 2, 3, 5, 17)
COMMON = (40000, 7, 50001, 12)      # an n-gram run present in every item that has references; two first tokens >= 32768


def make_corpus(seed=5, n_items=40, vocab=V_BIG, empty_item=7, long_item=0):
    """n_items items whose reference counts cycle through 1, 2, 3, 5, 17 (item `empty_item` has none); references of 4-16 tokens
    from a small working vocabulary (so that n-grams repeat across items and inside a reference), a third of it >= 32768 and
    none of it 65535 or below 10; every item with references holds the run COMMON in its first reference.  long_item = T > 0
    appends one more item with two references of about T tokens (the widest row a kernel takes)."""
    rng = random.Random(seed)
    words = [rng.randrange(10, 32768) for _ in range(40)] + [rng.randrange(32768, vocab - 1) for _ in range(20)]
    groups = []
    for i in range(n_items):
        m = 0 if i == empty_item else REF_COUNTS[i % len(REF_COUNTS)]
        base = [rng.choice(words) for _ in range(rng.randrange(5, 11))]
        refs = []
        for k in range(m):
            r = list(base)
            for _ in range(rng.randrange(0, 4)):
                r = edit(r, rng, words)
            if k == 0:
                at = rng.randrange(0, len(r) + 1)
                r = r[:at] + list(COMMON) + r[at:]
            refs.append(r[:16])
        groups.append(refs)
    if long_item:
        r = list(COMMON) + [rng.choice(words) for _ in range(long_item - len(COMMON))]
        groups.append([r, edit(edit(r, rng, words), rng, words)[:long_item]])
    return groups, words


def edit(tokens, rng, words):
    """one substitution, duplication or deletion"""
    t = list(tokens)
    if not t:
        return [rng.choice(words)]
    j = rng.randrange(len(t))
    kind = rng.randrange(3)
    if kind == 0:
        t[j] = rng.choice(words)
    elif kind == 1:
        t.insert(j, t[j])
    else:
        del t[j]
    return t


def make_hypotheses(groups, words, seed=9, per_item=2):
    """(tokens, item) pairs: one of the item's references with up to three edits (items without references get random tokens)"""
    rng = random.Random(seed)
    out = []
    for i, g in enumerate(groups):
        for _ in range(per_item):
            h = list(rng.choice(g)) if g else [rng.choice(words) for _ in range(6)]
            for _ in range(rng.randrange(0, 4)):
                h = edit(h, rng, words)
            out.append((h, i))
    return out


def as_row(tokens, width, start, eos, pad, with_eos=True):
    """an id row as generate() returns it: start token, the tokens, eos, pad"""
    row = [start] + list(tokens) + ([eos] if with_eos else [])
    assert len(row) <= width, (len(row), width)
    return row + [pad] * (width - len(row))
