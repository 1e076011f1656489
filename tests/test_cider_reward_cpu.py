"""CPU: the host side of the CIDEr reward on the device (src/rewards.py) -- build_cider_tables against the dictionary restatement
of the definition (tests/cider_ref.py), known answers, an fp32 emulation of the kernel's arithmetic with sequential sums against
the bound the GPU test uses, the honesty of the case recipe, kmb_cider_reward's validation through the loaded library (no launch),
for_batch's mapping and the command line.

Measured here (seed 5 corpus, 80 hypotheses): 100 % of the 78 rows with references score > 0, D and plain differ by more than 1e-3
relative on 90 % of them; the worst fp32-emulation error / bound ratio is 0.053 (sequential sums; the rule allows 0.5)."""
import ctypes as C
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cider_ref as R  # noqa: E402
from src.rewards import MAX_T, CiderReward, build_cider_tables, reward_tokens  # noqa: E402

PAD, BOS, EOS = 1, 0, 2


@pytest.fixture(scope="module")
def corpus():
    groups, words = R.make_corpus()
    tables = build_cider_tables(groups, R.V_BIG)
    return types.SimpleNamespace(groups=groups, words=words, tables=tables, raw=R.RawReference(groups),
                                 tab=R.TableReference(tables), hyps=R.make_hypotheses(groups, words))


def _ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


# ------------------------------------------------------------------------------------------------ 1. the builder
def test_tables_against_the_restatement(corpus):
    g, t, raw = corpus.groups, corpus.tables, corpus.raw
    N = len(g)
    assert N == 40 and t["n_items"] == N and t["idf_miss"] == np.float32(math.log(N))
    counts = [len(x) for x in g]
    assert counts[7] == 0 and sorted(set(counts)) == [0, 1, 2, 3, 5, 17]
    assert t["item_ref_offsets"].dtype == np.int32 and t["item_ref_offsets"].tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    refs = [r for x in g for r in x]
    assert t["ref_len"].dtype == np.int32 and t["ref_len"].tolist() == [len(r) for r in refs]
    assert t["df_keys"].dtype == np.uint64 and t["ref_keys"].dtype == np.uint64
    assert t["df_idf"].dtype == np.float32 and t["ref_w"].dtype == np.float32 and t["ref_norm"].dtype == np.float32
    off = t["df_offsets"]
    assert off[0] == 0 and len(off) == 5 and off[4] == len(t["df_keys"]) == len(t["df_idf"])
    top_bit = 0
    for n in range(1, 5):
        keys = [int(k) for k in t["df_keys"][off[n - 1]:off[n]]]
        assert all(a < b for a, b in zip(keys, keys[1:])), "order %d: df keys not strictly ascending unsigned" % n
        want = raw.df[n - 1]
        assert set(keys) == {R.pack(w) for w in want}
        top_bit += sum(1 for k in keys if k >> 63)
        for w, df in want.items():
            at = off[n - 1] + keys.index(R.pack(w))
            assert t["df_idf"][at] == np.float32(math.log(N) - math.log(df)), (n, w)     # float64, then one rounding
    assert top_bit > 0, "no 4-gram with its first token >= 32768: the unsigned order is not exercised"
    with_refs = sum(1 for x in g if x)
    for n in range(1, 5):          # the run present in every item that has references
        assert raw.df[n - 1][R.COMMON[:n]] == with_refs
    ngo = t["ref_ng_offsets"]
    assert ngo.dtype == np.int32 and len(ngo) == 4 * len(refs) + 1 and ngo[0] == 0 and ngo[-1] == len(t["ref_keys"]) == len(t["ref_w"])
    for r, ref in enumerate(refs):
        vecs = raw.ref_vectors(ref)
        for n in range(4):
            lo, hi = int(ngo[4 * r + n]), int(ngo[4 * r + n + 1])
            keys = [int(k) for k in t["ref_keys"][lo:hi]]
            assert all(a < b for a, b in zip(keys, keys[1:])), (r, n)
            gr, norm = vecs[n]
            assert set(keys) == {R.pack(w) for w in gr}
            for w, v in gr.items():
                got = float(t["ref_w"][lo + keys.index(R.pack(w))])
                assert abs(got - v) <= 0.5 * _ulp32(v) * (1 + 1e-9) + 1e-300, (r, n, w, got, v)
            assert abs(float(t["ref_norm"][r, n]) - norm) <= 0.5 * _ulp32(norm) * (1 + 1e-9) + 1e-300, (r, n)


def test_table_side_scores_equal_the_raw_side_up_to_table_rounding(corpus):
    """the two entry points of the restatement agree to a few float32 roundings of the table values"""
    for variant in ("D", "plain"):
        for h, i in corpus.hyps:
            a, b = corpus.raw.score(h, i, variant), corpus.tab.score(h, i, variant)
            assert abs(a - b) <= 1e-6 * max(a, b), (variant, i, a, b)


def test_builder_errors():
    with pytest.raises(ValueError, match="65536"):
        build_cider_tables([[[1, 2]]], 65537)
    with pytest.raises(ValueError, match="outside"):
        build_cider_tables([[[1, 500]]], 500)
    with pytest.raises(ValueError, match="outside"):
        build_cider_tables([[[-1]]], 500)
    with pytest.raises(ValueError):
        build_cider_tables([], 500)
    t = build_cider_tables([[], [[]]], 10)       # no n-gram at all: empty tables, not an error
    assert len(t["df_keys"]) == 0 and t["ref_len"].tolist() == [0] and t["ref_ng_offsets"].tolist() == [0] * 5


def test_reward_tokens_rule():
    assert reward_tokens([EOS, 5, 6, EOS, 7], PAD, BOS, EOS) == [5, 6]
    assert reward_tokens([EOS, EOS, 5], PAD, BOS, EOS) == []                 # eos at column 1
    assert reward_tokens([EOS, 5, PAD, BOS, 6], PAD, BOS, EOS) == [5, 6]     # no eos; pad / bos inside
    assert reward_tokens([5], PAD, BOS, EOS) == [] and reward_tokens([], PAD, BOS, EOS) == []
    assert reward_tokens([EOS, BOS, 9, 70000, -3, 8, EOS], PAD, BOS, EOS) == [9, 8]


# ------------------------------------------------------------------------------------------------ 2. known answers
def _two_items(ref):
    return [[ref], [[900, 901, 902, 903, 904]]]


@pytest.mark.parametrize("hyp,groups,want_d,want_plain", [
    ([11, 12, 13, 14, 15], _two_items([11, 12, 13, 14, 15]), 10.0, None),
    ([11, 12, 13], _two_items([11, 12, 13]), 7.5, None),
    ([11, 11, 11, 11, 11], _two_items([11, 12, 13, 14, 15]), 10.0 / 4 / (5 * math.sqrt(5)), 10.0 / 4 / math.sqrt(5)),
    ([11], [[[11]], [[11]]], 0.0, 0.0),
])
def test_known_answers(hyp, groups, want_d, want_plain):
    raw, tab = R.RawReference(groups), R.TableReference(build_cider_tables(groups, 1000))
    for ref in (raw, tab):
        got = ref.score(hyp, 0, "D")
        assert abs(got - want_d) <= 1e-6 * want_d, (got, want_d)
        if want_plain is not None:
            got = ref.score(hyp, 0, "plain")
            assert abs(got - want_plain) <= 1e-6 * want_plain, (got, want_plain)
    assert abs(10.0 / 4 / (5 * math.sqrt(5)) - 0.2236) < 5e-5 and abs(10.0 / 4 / math.sqrt(5) - 1.1180) < 5e-5


# ------------------------------------------------------------------------------------------------ 3. and 4. emulation, recipe
def test_fp32_emulation_stays_inside_the_bound_and_the_recipe_is_honest(corpus):
    worst, positive, differ, with_refs = 0.0, 0, 0, 0
    for h, i in corpus.hyps:
        m = len(corpus.groups[i])
        d = corpus.tab.score(h, i, "D")
        p = corpus.tab.score(h, i, "plain")
        if m == 0:
            assert d == 0.0 and p == 0.0
            continue
        with_refs += 1
        positive += d > 0
        differ += d > 0 and abs(d - p) > 1e-3 * max(d, p)
        for variant, want in (("D", d), ("plain", p)):
            got = corpus.tab.score_fp32(h, i, variant)
            b = R.bound(want, len(h), m)
            if want > 0:
                worst = max(worst, abs(got - want) / b)
            else:
                assert got == 0.0
    print("rows with references %d: %.0f %% score > 0, D and plain differ on %.0f %%; worst fp32 emulation error / bound %.3f"
          % (with_refs, 100.0 * positive / with_refs, 100.0 * differ / with_refs, worst))
    assert positive >= 0.9 * with_refs
    assert differ >= 0.5 * with_refs
    assert worst <= R.HEADROOM


# ------------------------------------------------------------------------------------------------ 5. validation
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from kmbart import _lib
    return _lib.load()


def test_validation_errors_launch_nothing(lib):
    """every argument is checked in front of the launch: host addresses stand in for device pointers and are never read"""
    buf = np.zeros(64, dtype=np.int64)
    p = C.c_void_p(buf.ctypes.data)
    off = (C.c_int64 * 5)(0, 0, 0, 0, 0)
    offp = C.cast(off, C.c_void_p)

    def call(ids=p, ld=8, B=1, L=8, item=p, n_items=1, dfk=p, dfi=p, dfo=offp, iro=p, n_refs=0, rl=p, rn=p, rngo=p, rk=p, rw=p,
             variant=0, sigma=6.0, out=p):
        rc = lib.kmb_cider_reward(ids, ld, B, L, PAD, BOS, EOS, item, n_items, dfk, dfi, dfo, 1.0, iro, n_refs, rl, rn, rngo, rk, rw, 0,
                                  variant, sigma, out, None)
        return rc, lib.kmb_last_error().decode()

    assert MAX_T >= 256
    cases = [(dict(ids=None), "required"), (dict(item=None), "required"), (dict(out=None), "required"), (dict(dfo=None), "df_offsets"),
             (dict(L=MAX_T + 1, ld=MAX_T + 1), "KMB_CIDER_MAX_T"), (dict(L=0), "KMB_CIDER_MAX_T"), (dict(ld=7), "ld >= L"),
             (dict(B=-1), "B >= 0"), (dict(sigma=0.0), "sigma"), (dict(sigma=-1.0), "sigma"), (dict(sigma=float("nan")), "sigma"),
             (dict(variant=2), "variant"), (dict(variant=-1), "variant")]
    cases += [({k: None}, "table pointer") for k in ("dfk", "dfi", "iro", "rl", "rn", "rngo", "rk", "rw")]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc != 0 and msg.startswith("kmb_cider_reward: ") and word in msg, (kw, rc, msg)
    bad = (C.c_int64 * 5)(0, 3, 2, 2, 2)
    rc, msg = call(dfo=C.cast(bad, C.c_void_p))
    assert rc != 0 and "ascend" in msg
    rc, msg = call(B=0)      # nothing to do is not an error, and launches nothing
    assert rc == 0


def test_python_surface_rejects_bad_arguments():
    with pytest.raises(ValueError, match="variant"):
        CiderReward([[[3]]], 10, PAD, BOS, EOS, variant="E", device="cpu")
    with pytest.raises(ValueError, match="sigma"):
        CiderReward([[[3]]], 10, PAD, BOS, EOS, sigma=0.0, device="cpu")
    with pytest.raises(ValueError, match="65536"):
        CiderReward([[[3]]], 70000, PAD, BOS, EOS, device="cpu")
    r = CiderReward([[[3]]], 10, PAD, BOS, EOS, device="cpu")
    with pytest.raises(ValueError, match="int64"):
        r.reward(torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="item_of_row"):
        r.reward(torch.zeros(1, 4, dtype=torch.int64), torch.zeros(2, dtype=torch.int32))


# ------------------------------------------------------------------------------------------------ 6. for_batch
def test_for_batch_mapping_and_errors():
    keys = [(7, "intent"), (7, "before"), (9, "intent")]
    r = CiderReward([[[3, 4]], [[5]], []], 10, PAD, BOS, EOS, device="cpu", group_keys=keys)
    batch = {"index": [9, 7, 7], "task_type": ["intent", "before", "intent"]}
    assert r.items_for_batch(batch) == [2, 1, 0]
    assert r.items_for_batch(batch, repeats=2) == [2, 2, 1, 1, 0, 0]
    assert callable(r.for_batch(batch))
    with pytest.raises(KeyError, match="after"):
        r.for_batch({"index": [7], "task_type": ["after"]})
    with pytest.raises(ValueError):
        r.items_for_batch({"index": [7, 9], "task_type": ["intent"]})
    with pytest.raises(ValueError, match="group keys"):
        CiderReward([[[3]], [[4]]], 10, PAD, BOS, EOS, device="cpu", group_keys=[1])
    with pytest.raises(ValueError, match="repeat"):
        CiderReward([[[3]], [[4]]], 10, PAD, BOS, EOS, device="cpu", group_keys=[1, 1])


def test_from_records_groups_by_index_and_task_type():
    from src.data.offline_tokenizer import load_base_tokenizer
    from src.data.tokenization import ConditionTokenizer
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    tok = ConditionTokenizer(base_tokenizer=load_base_tokenizer(os.path.join(gold, "tiny_bpe_tokenizer.json")))
    cfg = types.SimpleNamespace(vocab_size=len(tok), pad_token_id=tok.pad_token_id, bos_token_id=tok.bos_token_id,
                                eos_token_id=tok.eos_token_id, decoder_start_token_id=tok.eos_token_id)
    texts = ["a man walks", "a man runs away", "the dog", "a man walks"]
    records = [dict(index=3, task_type="intent", labels=texts[0]), dict(index=3, task_type="before", labels=texts[1]),
               dict(index=3, task_type="intent", labels=texts[2]), dict(index=4, task_type="intent", labels=texts[3]), None]
    r = CiderReward.from_records(records, tok, cfg, device="cpu")
    assert r.item_of_group == {(3, "intent"): 0, (3, "before"): 1, (4, "intent"): 2}
    assert r.tables["item_ref_offsets"].tolist() == [0, 2, 3, 4]
    want = [tok._text_ids([t])[0] for t in (texts[0], texts[2], texts[1], texts[3])]
    assert all(len(w) > 0 for w in want)
    assert r.tables["ref_len"].tolist() == [len(w) for w in want]
    off = r.tables["ref_ng_offsets"]
    assert sorted(int(k) for k in r.tables["ref_keys"][off[0]:off[1]]) == sorted(set(want[0]))
    for bad in (dict(task_type="intent", labels="a man"), dict(index=None, task_type="intent", labels="a man")):
        with pytest.raises(ValueError, match="index"):
            CiderReward.from_records(records[:2] + [bad], tok, cfg, device="cpu")


# ------------------------------------------------------------------------------------------------ 7. the command line
def test_cli_flags():
    import importlib
    mod = importlib.import_module("vcg_train")
    base = ["--checkpoint_dir", "x", "--model_config", "y", "--synthetic", "2"]
    a = mod.parse_args(base)
    assert a.self_critical is False and a.sc_reward == "cider_d" and a.sc_baseline == "greedy" and a.sc_max_length == 32
    a = mod.parse_args(base + ["--self_critical", "--sc_reward", "cider", "--sc_baseline", "none", "--sc_max_length", "20"])
    assert a.self_critical is True and a.sc_reward == "cider" and a.sc_baseline == "none" and a.sc_max_length == 20
    with pytest.raises(SystemExit):
        mod.parse_args(base + ["--sc_reward", "bleu"])
    with pytest.raises(ValueError, match="sc_max_length"):
        mod.parse_args(base + ["--self_critical", "--sc_max_length", "257"])
    assert mod.parse_args(base + ["--sc_max_length", "257"]).self_critical is False     # checked with --self_critical only
    with pytest.raises(ValueError, match="amp"):
        mod.parse_args(base + ["--self_critical", "--amp"])
    from src import training
    assert callable(training.self_critical_fine_tune)
