"""GPU: kmb_cider_reward (csrc/cider_reward.hip) against the table-side float64 restatement (tests/cider_ref.py TableReference),
row by row within score * (4 L_h + m + 24) * 2^-24, CIDEr-D and plain CIDEr on the same corpus: the seeded 40-item corpus of the
CPU test plus one item with two 255-token references, at V = 65536.

Rows: the recipe's hypotheses (a reference with up to three edits), lengths 0 to 5 and KMB_CIDER_MAX_T - 1 = 255 (a full-width
row, so also one without EOS), EOS at column 1, no EOS with and without padding, pad / bos inside a row, n-grams whose keys lie
one below the first and one above the last entry of each order's df slice and equal to each of them, an out-of-range item
(-1, N, 2^31 - 1) and the item without references.  A second, two-item corpus has one-entry df slices whose only n-gram is
token 65535 in every slot (order 4: the key with all 64 bits set).  for_batch with a non-identity item order and repeats = 2,
ld > L at an odd L, two launches bitwise equal, the words behind `out` untouched.

No pair (hypothesis, reference) of these rows has a length difference d with 80 <= |d| < 232, where exp(-d^2 / 72) is a
float32 denormal or zero but a non-zero float64 (asserted below): a relative bound says nothing about an underflowed penalty.

Measured on the MI355X (112 rows, 80 of the 82 recipe rows score > 0, largest score 10.0000): worst error / bound 0.036 for
CIDEr-D and 0.046 for plain CIDEr (test_kernel_against_the_table_side_reference prints both); the sequential-sum fp32 emulation
of tests/test_cider_reward_cpu.py measures 0.053 on the recipe rows."""
import os
import random
import sys
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cider_ref as R  # noqa: E402
from src.rewards import MAX_T, CiderReward, reward_tokens  # noqa: E402

DEV = "cuda:0"
PAD, BOS, EOS = 1, 0, 2
START = EOS


def _unpack(key, n):
    return [(key >> (16 * (n - 1 - k))) & 0xFFFF for k in range(n)]


def _boundary_hyps(tables, base):
    """per order: the first and the last n-gram of the df slice, the key one below the first and one above the last, each appended
    to `base` (a reference of the row's item: a wrong idf of the appended n-gram changes ||g_h|| and with it the score)"""
    off, out = tables["df_offsets"], []
    for n in range(1, 5):
        keys = [int(k) for k in tables["df_keys"][off[n - 1]:off[n]]]
        assert len(keys) >= 2
        for key in (keys[0], keys[0] - 1, keys[-1], keys[-1] + 1):
            w = _unpack(key, n)
            assert all(t not in (PAD, BOS, EOS) for t in w) and R.pack(w) == key, (n, key, w)
            assert (key in keys) == (key in (keys[0], keys[-1]))
            out.append(list(base) + w)
    return out


@pytest.fixture(scope="module")
def case():
    groups, words = R.make_corpus(long_item=MAX_T - 1)
    N = len(groups)
    keys = [(100 + i, "intent" if i % 2 else "before") for i in range(N)]
    rew = {v: CiderReward(groups, R.V_BIG, PAD, BOS, EOS, variant=v, device=DEV, group_keys=keys) for v in ("D", "plain")}
    tab = R.TableReference(rew["D"].tables)
    W = MAX_T
    rows, items = [], []

    def add(row, item, tokens=None):
        assert len(row) == W
        rows.append(row)
        items.append(item)
        if tokens is not None:
            assert reward_tokens(row, PAD, BOS, EOS) == list(tokens), (row[:12], tokens)

    for h, i in R.make_hypotheses(groups, words):                      # the recipe, two rows per item in item order
        h = h[:W - 2]                                                  # (the long item's: room for the start token and the EOS)
        add(R.as_row(h, W, START, EOS, PAD), i, h)
    n_recipe = len(rows)
    ref0 = groups[4][0]                                                # item 4 has 17 references
    assert len(groups[4]) == 17 and len(ref0) >= 6
    for k in range(6):                                                 # lengths 0 .. 5
        add(R.as_row(ref0[:k], W, START, EOS, PAD), 4, ref0[:k])
    rng = random.Random(3)
    long_h = R.edit(R.edit(groups[N - 1][0], rng, words), rng, words)[:W - 1]
    long_h += [words[0]] * (W - 1 - len(long_h))
    add([START] + long_h, N - 1, long_h)                               # 255 tokens, the full width, no EOS
    add([START, EOS] + ref0 + [PAD] * (W - 2 - len(ref0)), 4, [])      # EOS at column 1
    add(R.as_row(ref0, W, START, EOS, PAD, with_eos=False), 4, ref0)   # no EOS, padded
    inside = [START, ref0[0], PAD, ref0[1], BOS, BOS] + ref0[2:] + [EOS, ref0[0], ref0[1]]
    add(inside + [PAD] * (W - len(inside)), 4, ref0)                   # pad / bos inside, tokens behind the EOS
    for h in _boundary_hyps(rew["D"].tables, groups[3][0]):
        add(R.as_row(h, W, START, EOS, PAD), 3, h)
    for bad in (-1, N, 2 ** 31 - 1):                                   # items outside [0, N)
        add(R.as_row(ref0, W, START, EOS, PAD), bad, ref0)
    add(R.as_row(ref0, W, START, EOS, PAD), 7, ref0)                   # the item without references
    assert len(groups[7]) == 0
    toks = [reward_tokens(r, PAD, BOS, EOS) for r in rows]
    for t, i in zip(toks, items):                                      # the penalty never underflows between float32 and float64
        for length, _ in tab.refs_of(i):
            assert not 80 <= abs(len(t) - length) < 232, (len(t), length)
    want = {v: [tab.score(t, i, v) for t, i in zip(toks, items)] for v in ("D", "plain")}
    bounds = {v: [R.bound(s, len(t), len(tab.refs_of(i))) for s, t, i in zip(want[v], toks, items)] for v in ("D", "plain")}
    return types.SimpleNamespace(groups=groups, words=words, keys=keys, rew=rew, tab=tab, rows=rows, items=items, toks=toks, want=want,
                                 bounds=bounds, n_recipe=n_recipe, N=N)


def _check(got, want, bounds, what):
    worst = 0.0
    for r, (g, w, b) in enumerate(zip(got, want, bounds)):
        if w == 0.0:
            assert g == 0.0, (what, r, g)
        else:
            assert abs(g - w) <= b, (what, r, g, w, abs(g - w) / b)
            worst = max(worst, abs(g - w) / b)
    return worst


@pytest.mark.parametrize("variant", ["D", "plain"])
def test_kernel_against_the_table_side_reference(case, variant):
    c = case
    ids = torch.tensor(c.rows, dtype=torch.int64, device=DEV)
    items = torch.tensor(c.items, dtype=torch.int64).to(torch.int32).to(DEV)
    B = ids.shape[0]
    out = torch.full((B + 8,), -7.25, dtype=torch.float32, device=DEV)
    c.rew[variant].reward(ids, items, out=out)
    again = c.rew[variant].reward(ids, items)
    torch.cuda.synchronize()
    got = out[:B].double().cpu().tolist()
    assert bool((out[B:] == -7.25).all()), "words behind out were written"
    assert torch.equal(out[:B].view(torch.int32), again.view(torch.int32)), "two launches differ"
    worst = _check(got, c.want[variant], c.bounds[variant], variant)
    positive = sum(1 for w in c.want[variant][:c.n_recipe] if w > 0)
    print("CIDEr-%s: %d rows, %d of the %d recipe rows score > 0, largest score %.4f, worst error / bound %.4f"
          % (variant, B, positive, c.n_recipe, max(got), worst))
    assert positive >= 0.9 * (c.n_recipe - 2)
    assert worst <= 1.0


def test_variants_differ_and_scores_are_not_trivial(case):
    d, p = case.want["D"], case.want["plain"]
    assert sum(1 for a, b in zip(d, p) if a > 0 and abs(a - b) > 1e-3 * max(a, b)) >= 0.5 * sum(1 for a in d if a > 0)
    assert max(d) > 5.0 and case.want["D"][case.n_recipe] == 0.0          # the length-0 row


def test_one_entry_df_table_and_token_65535_in_all_four_slots():
    top = 65535
    groups = [[[top] * 5], []]
    hyps = [[top] * 5, [top] * 4, [top], [top, 9, top, top, top, top], [9, 10, 11], [top] * 8]
    for variant in ("D", "plain"):
        rew = CiderReward(groups, R.V_BIG, PAD, BOS, EOS, variant=variant, device=DEV)
        t = rew.tables
        assert t["df_offsets"].tolist() == [0, 1, 2, 3, 4] and int(t["df_keys"][3]) == 2 ** 64 - 1
        tab = R.TableReference(t)
        ids = torch.tensor([R.as_row(h, 12, START, EOS, PAD) for h in hyps], dtype=torch.int64, device=DEV)
        got = rew.reward(ids, torch.zeros(len(hyps), dtype=torch.int32, device=DEV)).double().cpu().tolist()
        want = [tab.score(h, 0, variant) for h in hyps]
        assert abs(want[0] - 10.0) < 1e-5 and want[4] == 0.0 and 0 < want[3] < 10
        _check(got, want, [R.bound(w, len(h), 1) for w, h in zip(want, hyps)], variant)


def test_for_batch_with_repeats_and_a_row_stride(case):
    """a batch whose groups come in another order than the items, two rows per group (generate(num_return_sequences=2)'s layout),
    an id matrix of odd width inside a wider buffer whose other columns hold real tokens"""
    c = case
    order = [5, 0, 39, 7, 12, 4]
    batch = {"index": [c.keys[i][0] for i in order], "task_type": [c.keys[i][1] for i in order]}
    L, ld = 23, 31
    rows, toks, items = [], [], []
    for i in order:
        for k in range(2):
            h = c.toks[2 * i + k]
            assert c.items[2 * i + k] == i and len(h) + 2 <= L
            rows.append(R.as_row(h, L, START, EOS, PAD) + [c.words[3]] * (ld - L))
            toks.append(h)
            items.append(i)
    buf = torch.tensor(rows, dtype=torch.int64, device=DEV)
    ids = buf[:, :L]
    assert ids.stride(0) == ld
    for variant in ("D", "plain"):
        fn = c.rew[variant].for_batch(batch, repeats=2)
        got = fn(ids).double().cpu().tolist()
        want = [c.tab.score(t, i, variant) for t, i in zip(toks, items)]
        assert sum(1 for w in want if w > 0) >= 8
        _check(got, want, [R.bound(w, len(t), len(c.groups[i])) for w, t, i in zip(want, toks, items)], variant)
        assert torch.equal(fn(ids.contiguous()).view(torch.int32), fn(ids).view(torch.int32))
    with pytest.raises(KeyError):
        c.rew["D"].for_batch({"index": [1], "task_type": ["nothing"]})


def test_a_wider_matrix_fails_loudly(case):
    ids = torch.full((2, MAX_T + 1), PAD, dtype=torch.int64, device=DEV)
    with pytest.raises(Exception, match="KMB_CIDER_MAX_T"):
        case.rew["D"].reward(ids, torch.zeros(2, dtype=torch.int32, device=DEV))


def test_default_device_scores():
    """CiderReward() with its default device ("cuda", no index) and from a torch.device: the tables land on the current device, whose
    tensors report an index -- reward() and for_batch() take them"""
    groups = [[[11, 12, 13, 14, 15]], [[21, 22, 23, 24, 25]]]
    batch = {"index": [1, 0], "task_type": ["intent", "intent"]}
    rows = [R.as_row(groups[1][0], 9, START, EOS, PAD), R.as_row(groups[0][0], 9, START, EOS, PAD)]
    for kw in ({}, dict(device="cuda"), dict(device=torch.device("cuda")), dict(device=torch.device("cuda", 0))):
        rew = CiderReward(groups, 100, PAD, BOS, EOS, group_keys=[(0, "intent"), (1, "intent")], **kw)
        assert rew.device == torch.device("cuda", torch.cuda.current_device())
        ids = torch.tensor(rows, dtype=torch.int64, device="cuda")
        got = rew.reward(ids, torch.tensor([1, 0], dtype=torch.int32, device="cuda")).cpu().tolist()
        assert all(abs(g - 10.0) <= R.bound(10.0, 5, 1) for g in got), got
        assert rew.for_batch(batch)(ids).cpu().tolist() == got
