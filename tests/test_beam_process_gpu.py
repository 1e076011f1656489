"""GPU: kmb_beam_step_processed (csrc/beam_process.hip + the EDIT forms of csrc/beam_step.hip's beam step), stateless form through
ctypes, against tests/beam_process_ref.py: candidates, scores, the next beams and the moved token histories with the three
processors at once; bit-equality with kmb_beam_step when nothing is edited and on a forced step; a token that is both penalised
and banned; the argument checks."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_process_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")
EOS = 2
P = 1.3
ATOL = 1e-4            # tests/test_ops_gpu.py::test_logsoftmax_topk; a penalised candidate's error scales with the penalty
GAP = 1e-3             # reference candidates at least this far apart: the order is decided
#        B  nb  V      ld     t     n
CASES = [(2, 3, 517, 520, 5, 2),             # ragged last chunk, parts mostly empty
         (3, 5, 50320, 50432, 7, 2),         # the production row
         (1, 2, 50320, 50432, 1024, 3),      # the history bound: ~1000 penalised tokens per row through the combine
         (64, 5, 50320, 50432, 12, 3)]       # 320 rows, the benchmarked count
IDS = ["small", "production_row", "history_bound", "rows_320"]


def _lib():
    from kmbart import _lib
    return _lib


def _p(x):
    return None if x is None else C.c_void_p(x.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def _case(i):
    """Host inputs and the reference of case i, computed once.  Logits randn * 4 (pad columns hold a value that would win);
    every row's history cycles through that row's 6 largest logits, so the edits hit the winners -- behind, for a long history,
    distinct other tokens, so that about t tokens are penalised; bad words [[x], [y, z]] from row 0's top tokens: x a history
    token of row 0 (penalised AND banned, in every row), [y, z] the token row 0 ends with and its best token outside the history."""
    B, nb, V, ld, t, n = CASES[i]
    R, k = B * nb, 2 * nb
    g = torch.Generator().manual_seed(71)
    logits = torch.randn(R, ld, generator=g) * 4
    logits[:, V:] = 30.0
    add = -torch.rand(R, generator=g) * 3
    top = torch.topk(logits[:, :V], 7, dim=1).indices
    cyc = min(t, 24)
    rows = []
    for r in range(R):
        head = []
        if t > cyc:
            perm = torch.randperm(V, generator=g).tolist()
            mine = set(top[r].tolist())
            head = [x for x in perm if x not in mine and x != EOS][:t - cyc]
        rows.append(head + [int(top[r, j % 6]) for j in range(cyc)])
    bad = [[int(top[0, 2])], [rows[0][-1], int(top[0, 6])]]
    ban = EOS if n == 2 else -1
    ref = beam_process_ref.step(logits.numpy(), rows, add.numpy(), B, nb, V, k, P, n, bad, ban_token=ban, eos=EOS)
    return dict(B=B, nb=nb, V=V, ld=ld, t=t, n=n, R=R, k=k, logits=logits, add=add, rows=rows, bad=bad, ban=ban, ref=ref)


def _table(bad):
    if not bad:
        return None, None, 0
    tok = [x for seq in bad for x in seq]
    off = [0]
    for seq in bad:
        off.append(off[-1] + len(seq))
    return torch.tensor(tok, dtype=torch.int32, device=DEV), torch.tensor(off, dtype=torch.int32, device=DEV), len(bad)


def _run(c, p=P, n=None, bad="case", force=-1, ban=None, processed=True, ld_ids=None, t=None, k=None, raw=False):
    """One call on fresh device buffers -> (rc, dict of outputs on the host)."""
    lib = _lib().load()
    B, nb, V, R = c["B"], c["nb"], c["V"], c["R"]
    k = c["k"] if k is None else k
    t = c["t"] if t is None else t
    logits, add = c["logits"].to(DEV), c["add"].to(DEV)
    ld_buf = c["t"] + 3
    ids_in = torch.full((R, ld_buf), -7, dtype=torch.int64)
    ids_in[:, :c["t"]] = torch.tensor(c["rows"], dtype=torch.int64)
    ids_in = ids_in.to(DEV)
    ids_out = torch.full((R, ld_buf), -9, dtype=torch.int64, device=DEV)
    out = torch.full((B, c["k"], 2), -1, dtype=torch.int32, device=DEV)
    nscore = torch.full((R,), 123.0, dtype=torch.float32, device=DEV)
    ntok = torch.full((R,), -1, dtype=torch.int64, device=DEV)
    nidx = torch.full((R,), -1, dtype=torch.int32, device=DEV)
    btok, boff, n_bad = _table(c["bad"] if bad == "case" else bad)
    n = c["n"] if n is None else n
    ban = c["ban"] if ban is None else ban
    if processed:
        nscr = lib.kmb_beam_step_processed_scratch(R, c["t"], n_bad)
        scr = torch.zeros(nscr, dtype=torch.float32, device=DEV)
        rc = lib.kmb_beam_step_processed(_p(logits), logits.stride(0), V, B, nb, _p(add), force, ban, k, _p(out), EOS, _p(nscore),
                                         _p(ntok), _p(nidx), _p(scr), nscr, _p(ids_in), _p(ids_out),
                                         ld_buf if ld_ids is None else ld_ids, t, float(p), n, _p(btok), _p(boff), n_bad, _stream())
    else:
        nscr = lib.kmb_logsoftmax_topk_scratch(R)
        scr = torch.zeros(nscr, dtype=torch.float32, device=DEV)
        rc = lib.kmb_beam_step(_p(logits), logits.stride(0), V, B, nb, _p(add), force, ban, k, _p(out), EOS, _p(nscore), _p(ntok),
                               _p(nidx), _p(scr), nscr, _stream())
    torch.cuda.synchronize()
    if raw:
        return rc, lib.kmb_last_error().decode()
    return rc, dict(out=out.cpu(), val=out[:, :, 0].contiguous().view(torch.float32).cpu().numpy(), idx=out[:, :, 1].cpu().numpy(),
                    next_scores=nscore.cpu(), next_tokens=ntok.cpu(), next_beam_idx=nidx.cpu(), ids_out=ids_out.cpu(),
                    ids_in=ids_in.cpu())


def _moved(got, t):
    """ids_out as the gathered and appended history of the call's own next beams."""
    want = torch.full_like(got["ids_out"], -9)
    want[:, :t] = got["ids_in"][got["next_beam_idx"].long(), :t]
    want[:, t] = got["next_tokens"]
    return want


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_against_the_step_reference(i):
    c = _case(i)
    B, nb, V, t, k, ref = c["B"], c["nb"], c["V"], c["t"], c["k"], c["ref"]
    rc, got = _run(c)
    _lib().check(rc)
    # every returned pair has the reference's score for that pair; the sorted scores match
    worst = dict(plain=0.0, penalised=0.0, sorted=0.0)
    n_pen = 0
    for b in range(B):
        for j in range(k):
            beam, tok = divmod(int(got["idx"][b, j]), V)
            r = b * nb + beam
            pen = tok in c["rows"][r]
            n_pen += pen
            e = abs(float(got["val"][b, j]) - float(ref["s"][r, tok]))
            assert np.isfinite(ref["s"][r, tok]), (b, j, beam, tok)
            worst["penalised" if pen else "plain"] = max(worst["penalised" if pen else "plain"], e)
            assert e <= (ATOL * P if pen else ATOL), (b, j, beam, tok, got["val"][b, j], ref["s"][r, tok])
    worst["sorted"] = float(np.abs(got["val"] - ref["val"][:, :k]).max())
    gap = (ref["val"][:, :-1] - ref["val"][:, 1:]).min(axis=1)          # over the best k + 1
    decided = gap >= GAP
    print("%s: errors %s; %d of %d winners penalised; %d of %d items decided, smallest gap %.3e"
          % (IDS[i], worst, n_pen, B * k, int(decided.sum()), B, float(gap.min())))
    assert worst["sorted"] <= ATOL * P
    assert (~decided).sum() <= (B // 4 if i == 3 else 0), gap
    assert n_pen >= B * k // 3                                          # the edits decide these searches
    # exact order and next beams wherever the reference's order is decided
    rows_ok = np.repeat(decided, nb)
    assert np.array_equal(got["idx"][decided], ref["idx"][:, :k][decided])
    assert np.array_equal(got["next_tokens"].numpy()[rows_ok], ref["next_tokens"][rows_ok])
    assert np.array_equal(got["next_beam_idx"].numpy()[rows_ok], ref["next_beam_idx"][rows_ok])
    assert np.abs(got["next_scores"].numpy()[rows_ok] - ref["next_scores"][rows_ok]).max() <= ATOL * P
    # the histories moved on: exactly the gather and the append of the call's own choice, and the reference's where decided
    assert torch.equal(got["ids_out"], _moved(got, t))
    for r in np.nonzero(rows_ok)[0]:
        assert got["ids_out"][r, :t + 1].tolist() == ref["ids_out"][r]
    # a token that is penalised and banned never appears; nor the banned tail of the bad word in row 0, nor a banned EOS
    x, z = c["bad"][0][0], c["bad"][1][1]
    assert x in c["rows"][0] and not bool((got["idx"] % V == x).any())
    assert not any(int(v) == z for v in got["idx"][0] if int(v) // V == 0)
    if c["ban"] >= 0:
        assert not bool((got["idx"] % V == EOS).any())


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_nothing_to_edit_is_kmb_beam_step_bit_for_bit(i):
    c = _case(i)
    for ban in (-1, EOS):
        rc, a = _run(c, p=1.0, n=0, bad=None, ban=ban)
        _lib().check(rc)
        rc, b = _run(c, ban=ban, processed=False)
        _lib().check(rc)
        for key in ("out", "next_scores", "next_tokens", "next_beam_idx"):
            assert torch.equal(a[key], b[key]), (key, ban)
        assert torch.equal(a["ids_out"], _moved(a, c["t"]))


@pytest.mark.parametrize("i", [0, 1], ids=IDS[:2])
def test_forced_step(i):
    c = _case(i)
    force = 11
    rc, a = _run(c, force=force)
    _lib().check(rc)
    rc, b = _run(c, force=force, processed=False)
    _lib().check(rc)
    for key in ("out", "next_scores", "next_tokens", "next_beam_idx"):
        assert torch.equal(a[key], b[key]), key
    per_item = c["add"].view(c["B"], c["nb"]).sort(dim=1, descending=True).values.reshape(-1)   # log-probability exactly 0
    assert bool((a["next_tokens"] == force).all()) and torch.equal(a["next_scores"], per_item)
    assert torch.equal(a["ids_out"], _moved(a, c["t"])) and bool((a["ids_out"][:, c["t"]] == force).all())


def test_refused_arguments_launch_nothing():
    c = _case(0)
    V, t = c["V"], c["t"]
    refusals = [dict(t=0), dict(t=1025), dict(ld_ids=t), dict(p=0.5), dict(p=INF), dict(p=float("nan")), dict(n=-1),
                dict(k=17), dict(force=V), dict(ban=V)]
    for over in refusals:
        rc, msg = _run(c, raw=True, **over)
        assert rc != 0 and msg.startswith("kmb_beam_step_processed: "), (over, msg)
    rc, got = _run(c, t=0)
    assert rc != 0
    assert bool((got["ids_out"] == -9).all()) and bool((got["out"] == -1).all()) and bool((got["next_tokens"] == -1).all())
    lib = _lib().load()
    # too many bad words, a missing table, too little scratch, one buffer for both histories
    x = torch.zeros((c["R"], c["ld"]), dtype=torch.float32, device=DEV)
    ids = torch.zeros((c["R"], t + 1), dtype=torch.int64, device=DEV)
    ids2 = torch.full_like(ids, -9)
    o = torch.zeros((c["B"], c["k"], 2), dtype=torch.int32, device=DEV)
    ns = torch.zeros(c["R"], dtype=torch.float32, device=DEV)
    nt = torch.zeros(c["R"], dtype=torch.int64, device=DEV)
    ni = torch.zeros(c["R"], dtype=torch.int32, device=DEV)
    nscr = lib.kmb_beam_step_processed_scratch(c["R"], t, 0)
    scr = torch.zeros(nscr, dtype=torch.float32, device=DEV)

    def call(ids_out=ids2, n_bad=0, scratch_floats=nscr, ld=c["ld"]):
        return lib.kmb_beam_step_processed(_p(x), ld, V, c["B"], c["nb"], None, -1, -1, c["k"], _p(o), EOS, _p(ns), _p(nt), _p(ni),
                                           _p(scr), scratch_floats, _p(ids), _p(ids_out), t + 1, t, 1.3, 2, None, None, n_bad, _stream())

    for kw in (dict(ids_out=ids), dict(n_bad=4097), dict(n_bad=1), dict(scratch_floats=nscr - 1), dict(ld=c["ld"] + 2)):
        assert call(**kw) != 0 and lib.kmb_last_error().decode().startswith("kmb_beam_step_processed: "), kw
    torch.cuda.synchronize()
    assert bool((ids2 == -9).all())
    _lib().check(call())
    torch.cuda.synchronize()
    assert bool((ids2[:, :t] == 0).all())
