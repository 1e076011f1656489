"""GPU: kmb_logits_process (csrc/logits_process.hip) against _postprocess_next_token_scores run on the device on a clone's
[:, :V] view: the whole [R, ld] buffer bit for bit (torch.equal) -- penalised values, bans, the pad columns and every
untouched word -- over the shapes, lengths, penalties and n-gram sizes at which the kernel takes another path, its named edge
rows, and the argument checks."""
import ctypes as C
import random

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")
SHAPES = [(1, 50, 64), (5, 50, 64), (3, 50320, 50432)]
LENGTHS = [1, 2, 3, 63, 64, 65, 257, 1024]
PENALTIES = [1.0, 1.3, 2.0, 200.0]


def _lib():
    from kmbart import _lib
    return _lib


def _p(x):
    return None if x is None else C.c_void_p(x.data_ptr())


def _table(bad):
    """The flattened table the kernel reads (heads of any length: the model's packer is stricter than the kernel)."""
    if not bad:
        return None, None, 0
    tok = [x for seq in bad for x in seq]
    off = [0]
    for seq in bad:
        off.append(off[-1] + len(seq))
    return (torch.tensor(tok, dtype=torch.int32, device=DEV), torch.tensor(off, dtype=torch.int32, device=DEV), len(bad))


def _call(logits, V, ids, t, p=1.0, n=0, bad=None, R=None, ld=None, ld_ids=None, table=None):
    btok, boff, n_bad = _table(bad) if table is None else table
    rc = _lib().load().kmb_logits_process(_p(logits), logits.stride(0) if ld is None else ld, V, logits.shape[0] if R is None else R,
                                          _p(ids), ids.stride(0) if ld_ids is None else ld_ids, int(t), float(p), int(n), _p(btok),
                                          _p(boff), n_bad, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return rc


def _reference(x, V, rows, t, p, n, bad):
    from src.model.model import _postprocess_next_token_scores
    ref = x.clone()
    _postprocess_next_token_scores(ref[:, :V], rows, t, 0, None, p, n, bad)
    return ref


def _check(x, V, ids, t, p=1.0, n=0, bad=None, rows=None, ref_t=None):
    """Runs the kernel on a clone of x and the reference on another; returns the kernel's output."""
    got = x.clone()
    _lib().check(_call(got, V, ids, t, p, n, bad))
    rows = ids[:, :t].tolist() if rows is None else rows
    ref = _reference(x, V, rows, t if ref_t is None else ref_t, p, n, bad)
    torch.cuda.synchronize()
    if not torch.equal(got, ref):
        diff = torch.nonzero(got != ref)
        r, c = diff[0].tolist()
        raise AssertionError("t=%d p=%s n=%d bad=%s: %d words differ, first [%d, %d]: before %r kernel %r reference %r"
                             % (t, p, n, bad, diff.shape[0], r, c, x[r, c].item(), got[r, c].item(), ref[r, c].item()))
    return got


def _logits(R, V, ld, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(R, ld, generator=g) * 4
    x[:, 0], x[:, 1], x[:, 2], x[:, 3] = 0.0, -0.0, INF, -INF       # tokens 0 .. 3 are common in the rows below
    x[:, V:] = 7.25                                                 # the pad columns must keep their bits
    return x.to(DEV)


def _ids(R, V, t, rnd):
    """Rows of t tokens: half from a 6-token alphabet (repeats, n-gram hits), half anywhere in the vocabulary."""
    rows = [[rnd.randrange(6) if rnd.random() < 0.5 else rnd.randrange(V) for _ in range(t)] for _ in range(R)]
    ids = torch.full((R, 1030), -5, dtype=torch.int64)              # the columns behind t are never read
    ids[:, :t] = torch.tensor(rows, dtype=torch.int64)
    return ids.to(DEV), rows


@pytest.mark.parametrize("R,V,ld", SHAPES)
def test_matches_the_host_function_bit_for_bit(R, V, ld):
    rnd = random.Random(R * 1000 + V)
    x = _logits(R, V, ld, seed=R + V)
    for t in LENGTHS:
        ids, rows = _ids(R, V, t, rnd)
        # a single token, one whose two-token head is row 0's tail, one whose head is longer than t or equal to it
        bad = [[rows[0][-1]], ([rows[0][-2], rows[0][-1], 9] if t >= 2 else [4, 9]), [1] * t + [10], [2] * (t - 1) + [rows[0][-1], 11]]
        for p in PENALTIES:
            for n in sorted({0, 1, 2, 3, t, t + 1, t + 2}):
                _check(x, V, ids, t, p, n, bad if (n + t) % 2 else None, rows=rows)


def test_identical_tokens_are_penalised_once_and_a_penalised_token_can_be_banned():
    V, ld, t = 50, 64, 1024
    x = _logits(2, V, ld, seed=3)
    ids = torch.full((2, t), 7, dtype=torch.int64, device=DEV)
    ids[1, :] = 8
    ids[1, -1] = 0                                                   # row 1 ends ... 8 8 0
    for p in (1.3, 200.0):
        got = _check(x, V, ids, t, p)
        once = torch.where(x[0, 7] < 0, x[0, 7] * p, x[0, 7] / p)    # what torch computes for ONE application
        assert got[0, 7].item() == once.item() and got[0, 7].item() != x[0, 7].item()
    got = _check(x, V, ids, t, 1.3, n=2)                             # bigram (8, 8) was followed by 8 and by 0; the row ends in 0
    assert torch.isfinite(got[1, 8])                                 # ... so only the tokens after a 0 are banned: none
    ids[1, -1] = 8
    got = _check(x, V, ids, t, 1.3, n=2)
    assert got[1, 8].item() == -INF and got[0, 7].item() == -INF     # penalised in phase A, banned in phase B
    got = _check(x, V, ids, t, 1.3, bad=[[8, 8]])
    assert got[1, 8].item() == -INF and torch.isfinite(got[0, 8])


def test_bad_word_head_against_the_number_of_rows_and_the_length():
    V, ld, t = 50, 64, 5
    row = [11, 12, 13, 14, 15]
    bad = [[14, 15, 20], [12, 13, 14, 15, 21], [10, 11, 12, 13, 14, 15, 22], [23]]   # heads of 2, 4, 6 (longer than t) and 0 tokens
    for R, banned in ((1, [23]), (5, [20, 21, 23]), (2, [20, 23])):
        x = _logits(R, V, ld, seed=R)
        ids = torch.tensor([row] * R, dtype=torch.int64, device=DEV)
        got = _check(x, V, ids, t, bad=bad)
        assert torch.nonzero(got[0, 4:V] == -INF).flatten().add(4).tolist() == banned, (R, got[0, :V])


def test_tokens_outside_the_vocabulary_are_dropped():
    """Stateless call only (generate() never writes one): the result is that of the rows without those positions."""
    R, V, ld, t = 3, 50, 64, 9
    x = _logits(R, V, ld, seed=9)
    clean = [[4, 5, 4, 5, 6, 4, 5], [1, 1, 1, 2, 1, 1, 1], [30, 31, 32, 30, 31, 32, 30]]
    junk = [V, -1, 1 << 40, V + 5, -(1 << 35), 1 << 31]
    rows = []
    for r, row in enumerate(clean):
        row = list(row)
        row.insert((2 * r) % 7, junk[2 * r])
        row.insert(7 - r, junk[2 * r + 1])
        rows.append(row)
    ids = torch.tensor(rows, dtype=torch.int64, device=DEV)
    for p, n, bad in ((1.3, 0, None), (1.0, 2, None), (2.0, 3, [[4, 5, 7], [8]]), (1.3, 1, None), (1.0, 8, None)):
        _check(x, V, ids, t, p, n, bad, rows=clean, ref_t=7)


def test_bad_arguments_fail_with_a_message_and_launch_nothing():
    L = _lib()
    R, V, ld, t = 4, 50, 64, 6
    x = _logits(R, V, ld, seed=5)
    before = x.clone()
    ids = torch.full((R, 8), 3, dtype=torch.int64, device=DEV)
    table = _table([[3], [3, 3, 9]])
    nan = float("nan")

    def call(logits=x, ids_=ids, table_=table, **kw):
        return _call(logits, kw.pop("V", V), ids_, kw.pop("t", t), kw.pop("p", 1.3), kw.pop("n", 1), table=table_, **kw)

    cases = [dict(logits=None, ld=ld, R=R), dict(ids_=None, ld_ids=8), dict(ld=V - 1), dict(R=0), dict(R=-1), dict(t=0), dict(t=1025),
             dict(t=9), dict(ld_ids=5), dict(p=0.99), dict(p=nan), dict(p=INF), dict(n=-1), dict(table_=(table[0], table[1], -1)),
             dict(table_=(table[0], table[1], 4097)), dict(table_=(None, table[1], 2)), dict(table_=(table[0], None, 2))]
    for bad in cases:
        assert call(**bad) != 0, bad
        msg = L.load().kmb_last_error().decode()
        assert msg.startswith("kmb_logits_process: "), (bad, msg)
    torch.cuda.synchronize()
    assert torch.equal(x, before)
    assert call() == 0                                               # the same buffers with good arguments
    torch.cuda.synchronize()
    assert bool((x[:, 3] == -INF).all()) and bool((x[:, 9] == -INF).all()) and torch.equal(x[:, 4:9], before[:, 4:9])


def test_engine_form_fails_by_name_without_a_generation():
    """kmb_gen_logits_process before kmb_gen_begin (the engine-level cases live in tests/test_generate_processors_gpu.py)."""
    L = _lib()
    assert L.load().kmb_gen_logits_process(None, None, 0, None, 0, 0, 1.0, 0, None, None, 0, None) != 0
    assert L.load().kmb_last_error().decode().startswith("kmb_gen_logits_process: ")
