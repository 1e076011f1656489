"""GPU: greedy decoding on the device (kmb_greedy_step / kmb_gen_greedy_step, csrc/greedy.hip) against an fp64 host
reference with an explicit lowest-index tie rule, its edge rows, the finished-row and log-probability bookkeeping, the folded
next-step embedding, and generate(num_beams=1) on the device against the torch loop (model._device_greedy = False): equal ids,
scores within 1e-4 (the project's fp32 score tolerance, tests/test_beam_sample_gpu.py)."""
import ctypes as C
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ATOL = 1e-4
INF = float("inf")
THREADS = 1024        # lanes of a row's workgroup: 16-byte chunk c of an aligned row goes to lane c % THREADS, load c // THREADS


def _lib():
    from kmbart import _lib
    return _lib


def _p(x):
    return None if x is None else C.c_void_p(x.data_ptr())


def _call(logits, V, rows, ban, unfinished, pad, eos, tok, ids, t, flag, lsum, lout, ld=None, ld_ids=None):
    L = _lib()
    return L.load().kmb_greedy_step(_p(logits), logits.stride(0) if ld is None else ld, V, rows, int(ban), _p(unfinished), int(pad),
                                    int(eos), _p(tok), _p(ids), int(t), (ids.stride(0) if ids is not None else 0) if ld_ids is None
                                    else ld_ids, _p(flag), _p(lsum), _p(lout), C.c_void_p(torch.cuda.current_stream().cuda_stream))


def greedy(logits, V, ban=-1, unfinished=None, pad=0, eos=-1, ids=None, t=0, flag=None, lsum=None):
    """kmb_greedy_step on [rows, ld] logits; returns (tokens, logprob_out)."""
    rows = logits.shape[0]
    tok = torch.full((rows,), -7, dtype=torch.int64, device=DEV)
    lout = torch.full((rows,), 77.0, dtype=torch.float32, device=DEV)
    _lib().check(_call(logits, V, rows, ban, unfinished, pad, eos, tok, ids, t, flag, lsum, lout))
    torch.cuda.synchronize()
    return tok, lout


def reference(x, V, ban=-1):
    """fp64, on the host: (token, lp) per row of x[:, :V]; NaN read as -inf, the ban before the normalisation, the LOWEST index
    among exact ties, token 0 and lp = -inf for a row with no finite entry."""
    x = x[:, :V].detach().cpu().double().clone()
    x[x != x] = -INF
    if ban >= 0:
        x[:, ban] = -INF
    m = x.max(dim=1).values
    col = torch.arange(V).expand_as(x)
    tok = torch.where(x == m[:, None], col, torch.full_like(col, V)).min(dim=1).values
    lp = m - torch.logsumexp(x, dim=1)
    dead = m == -INF
    tok[dead] = 0
    lp[dead] = -INF
    return tok, lp


def padded(x, ld):
    """x in a [rows, ld] buffer whose pad columns hold +inf (even rows) / NaN (odd rows): reading one would win or poison a row."""
    buf = torch.full((x.shape[0], ld), INF, dtype=torch.float32, device=DEV)
    buf[1::2] = float("nan")
    buf[:, :x.shape[1]] = x
    return buf


def check_rows(buf, V, ban=-1):
    tok, lout = greedy(buf, V, ban=ban)
    rtok, rlp = reference(buf, V, ban)
    assert tok.cpu().tolist() == rtok.tolist()
    got = lout.cpu().double()
    fin = torch.isfinite(rlp)
    assert torch.equal(got[~fin], rlp[~fin])
    err = (got[fin] - rlp[fin]).abs().max().item() if bool(fin.any()) else 0.0
    assert err <= ATOL, err
    return tok, lout


@pytest.mark.parametrize("scale", [0.05, 5.0])
@pytest.mark.parametrize("V,ld", [(1, 1), (63, 64), (1025, 1027), (50265, 50432), (70001, 70001)])
def test_operator_matches_fp64_reference(V, ld, scale):
    """(1025, 1027) and (70001, 70001): rows that do not start on 16 bytes take the one-column-per-load path."""
    g = torch.Generator().manual_seed(V + int(scale * 100))
    x = (torch.randn(8, V, generator=g) * scale).to(DEV)
    check_rows(padded(x, ld), V)


def _tie_rows(V, pairs, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(len(pairs), V, generator=g).clamp_(max=4.0)
    for r, cols in enumerate(pairs):
        for c in cols:
            x[r, c] = 9.0
    return x.to(DEV)


def test_ties_and_maximum_position_aligned_rows():
    V, ld = 50265, 50432
    ch = 4 * THREADS
    pairs = [(0,), (V - 1,),                     # the maximum in the first column, and in the last (the scalar tail after the chunks)
             (5, 9),                             # two lanes
             (4 * 63 + 1, 4 * 64 + 2),           # two waves
             (40, 40 + ch),                      # two load chunks of one lane
             (43, 43 + 4 * ch),                  # ... of two unrolled groups
             (3, 4), (13, 14),                   # across and inside the 16-byte vector
             (28, 4 * (THREADS + 6)),            # the lower index in the HIGHER lane
             (4 * 70, 4 * (THREADS + 1)),        # ... in the higher wave
             (V - 5, V - 1), (0, V - 1),         # a chunk against the scalar tail
             (17, 4 * 64 + 1, 3 * ch + 2)]       # three at once
    tok, _ = check_rows(padded(_tie_rows(V, pairs, 1), ld), V)
    assert tok.cpu().tolist() == [min(p) for p in pairs]


def test_ties_unaligned_rows():
    """ld % 4 != 0: three rows of four start off 16 bytes (column i goes to lane i % THREADS there); each pair on all four."""
    V, ld = 9001, 9003
    base = [(0,), (V - 1,), (5, 6), (63, 64), (10, 10 + THREADS), (10, 10 + 4 * THREADS), (7, THREADS + 6), (70, THREADS + 1),
            (3, 4), (V - 2, V - 1)]
    pairs = [p for p in base for _ in range(4)]
    tok, _ = check_rows(padded(_tie_rows(V, pairs, 2), ld), V)
    assert tok.cpu().tolist() == [min(p) for p in pairs]


def test_edge_rows():
    V, ld = 5000, 5008
    g = torch.Generator().manual_seed(3)
    x = torch.randn(6, V, generator=g)
    x[0, 7] = 9.0; x[0, 4321] = 8.0                  # the maximum is the banned token: the runner-up wins
    x[1, 7] = -INF                                   # the banned token already -inf
    x[2, 100] = float("nan"); x[2, 7] = float("nan"); x[2, ::3] = float("nan")   # NaN is -inf, never the maximum
    x[3, :] = -INF                                   # no finite entry
    x[4, :] = -INF; x[4, 7] = 3.0                    # only the banned token is finite
    x[5, :] = float("nan"); x[5, 77] = -2.0          # one real entry: lp = 0
    buf = padded(x.to(DEV), ld)
    tok, lout = check_rows(buf, V, ban=7)
    assert tok.cpu().tolist()[0] == 4321 and tok.cpu().tolist()[3:] == [0, 0, 77]
    assert lout.cpu().tolist()[3:] == [-INF, -INF, 0.0]
    tok, lout = check_rows(buf, V)                   # without the ban
    assert tok.cpu().tolist()[0] == 7 and tok.cpu().tolist()[4] == 7
    one = torch.tensor([[1.5], [-3.0]], device=DEV)  # V = 1
    tok, lout = check_rows(one, 1)
    assert tok.cpu().tolist() == [0, 0] and lout.cpu().tolist() == [0.0, 0.0]
    tok, lout = check_rows(one, 1, ban=0)            # ... with the ban on its only column
    assert tok.cpu().tolist() == [0, 0] and lout.cpu().tolist() == [-INF, -INF]


def test_bookkeeping_scores_and_determinism():
    V, ld, R, PAD, EOS = 1000, 1000, 6, 1, 2
    g = torch.Generator().manual_seed(4)
    x = torch.randn(R, V, generator=g)
    x[2, EOS] = 7.0                                  # row 2 picks EOS; rows 1 and 4 come in finished
    x[4, EOS] = 7.0
    x = x.to(DEV)
    rtok, rlp = reference(x, V)

    def run(unf0, eos, flag0=0):
        unf = None if unf0 is None else torch.tensor(unf0, dtype=torch.int64, device=DEV)
        ids = torch.full((R, 5), -9, dtype=torch.int64, device=DEV)
        flag = torch.full((1,), flag0, dtype=torch.int32, device=DEV)
        lsum = torch.full((R,), 0.5, dtype=torch.float32, device=DEV)
        tok, lout = greedy(x, V, unfinished=unf, pad=PAD, eos=eos, ids=ids, t=3, flag=flag, lsum=lsum)
        return tok, lout, unf, ids, flag, lsum

    tok, lout, unf, ids, flag, lsum = run([1, 0, 1, 1, 0, 1], EOS)
    want = rtok.tolist()
    want[1] = want[4] = PAD
    assert want[2] == EOS and tok.cpu().tolist() == want
    assert unf.cpu().tolist() == [1, 0, 0, 1, 0, 1]                       # EOS clears its row, finished rows stay finished
    live = torch.tensor([1, 0, 1, 1, 0, 1], dtype=torch.bool)
    assert lout.cpu()[~live].tolist() == [0.0, 0.0]
    assert (lout.cpu().double()[live] - rlp[live]).abs().max().item() <= ATOL
    assert torch.equal(lsum.cpu()[~live], torch.tensor([0.5, 0.5]))      # a finished row adds nothing
    assert (lsum.cpu().double()[live] - (0.5 + rlp[live])).abs().max().item() <= ATOL   # the EOS row adds its own lp
    assert int(flag) == 1
    assert torch.equal(ids[:, 3], tok) and bool((ids[:, [0, 1, 2, 4]] == -9).all())
    # two runs, the same bits
    again = run([1, 0, 1, 1, 0, 1], EOS)
    for a, b in zip((tok, lout, unf, ids, flag, lsum), again):
        assert torch.equal(a, b)
    # the flag stays 0 when no row remains unfinished (every live row picks EOS), and is only ever OR-ed
    tok, lout, unf, ids, flag, lsum = run([0, 0, 1, 0, 1, 0], EOS)
    assert unf.cpu().tolist() == [0] * R and int(flag) == 0
    assert run([0, 0, 1, 0, 1, 0], EOS, flag0=2)[4].item() == 2
    assert run([1, 0, 1, 0, 1, 0], EOS, flag0=2)[4].item() == 3
    # no EOS, no unfinished: every row is live
    tok, lout, unf, ids, flag, lsum = run(None, -1)
    assert tok.cpu().tolist() == rtok.tolist() and int(flag) == 1
    assert (lsum.cpu().double() - (0.5 + rlp)).abs().max().item() <= ATOL


def test_bad_arguments_fail_with_a_message_and_launch_nothing():
    L = _lib()
    V, ld, R = 64, 64, 4
    x = torch.randn(R, ld, device=DEV)
    x[:, 5] = 50.0
    tok = torch.full((R,), -7, dtype=torch.int64, device=DEV)
    ids = torch.full((R, 4), -9, dtype=torch.int64, device=DEV)
    lsum = torch.full((R,), 0.5, dtype=torch.float32, device=DEV)
    lout = torch.full((R,), 77.0, dtype=torch.float32, device=DEV)
    unf = torch.ones(R, dtype=torch.int64, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)

    def call(V_=V, ld_=ld, R_=R, logits=x, tok_=tok, ids_=ids, t=1, ld_ids=4):
        return _call(logits, V_, R_, -1, unf, 1, 2, tok_, ids_, t, flag, lsum, lout, ld=ld_, ld_ids=ld_ids)

    for bad in (dict(V_=0), dict(ld_=V - 1), dict(R_=0), dict(logits=None), dict(tok_=None), dict(t=-1), dict(t=4)):
        assert call(**bad) != 0, bad
        msg = L.load().kmb_last_error().decode()
        assert msg.startswith("kmb_greedy_step: "), (bad, msg)
    torch.cuda.synchronize()
    assert bool((tok == -7).all()) and bool((ids == -9).all()) and bool((lsum == 0.5).all()) and bool((lout == 77.0).all())
    assert bool((unf == 1).all()) and int(flag) == 0
    assert call() == 0                                # the same buffers with good arguments
    torch.cuda.synchronize()
    assert tok.tolist() == [5] * R and ids[:, 1].tolist() == [5] * R


# ------------------------------------------------------------------------------------------------ the model
def _tiny_model():
    from oracle import goldenlib as G
    from src.model import MultiModalBartConfig, MultiModalBartForConditionalGeneration
    ocfg = G.tiny_config()
    keys = ("vocab_size", "d_model", "encoder_layers", "decoder_layers", "encoder_attention_heads",
            "decoder_attention_heads", "encoder_ffn_dim", "decoder_ffn_dim", "max_position_embeddings",
            "image_feature_size", "img_feat_id", "cls_token_id", "dropout", "attention_dropout", "activation_dropout")
    model = MultiModalBartForConditionalGeneration(MultiModalBartConfig.from_dict({k: getattr(ocfg, k) for k in keys}))
    model.load_state_dict(G.trained_state_dict(), strict=False)
    return model.to(DEV).eval()


@pytest.fixture(scope="module")
def tiny():
    return _tiny_model()


def _batch(n, seed=9):
    from oracle.make_golden import copy_task_batch
    gb = copy_task_batch(seed, n)
    return dict(input_ids=gb["input_ids"].to(DEV), image_features=[f.to(DEV) for f in gb["image_features"]],
                attention_mask=gb["attention_mask"].to(DEV))


def _both(model, kw):
    a = model.generate(**kw)
    model._device_greedy = False
    try:
        b = model.generate(**kw)
    finally:
        del model._device_greedy
    return a, b


def _same(a, b):
    """(ids, scores) of the device path against the torch path: the same tokens, scores within ATOL."""
    assert isinstance(a, tuple) and isinstance(b, tuple)
    assert a[0].dtype == torch.long and torch.equal(a[0], b[0]), (a[0].tolist(), b[0].tolist())
    for s in (a[1], b[1]):
        assert s.dtype == torch.float32 and s.shape == (a[0].shape[0],) and s.device == a[0].device
    assert (a[1] - b[1]).abs().max().item() <= ATOL, (a[1].tolist(), b[1].tolist())


def test_folded_embedding_is_the_embedding_launch(tiny):
    """kmb_gen_greedy_step(embed_step = 1) + gen_step(tokens = NULL, 1) against gen_step(next_tokens, 1) after a fresh gen_begin."""
    eng = tiny._need_engine()
    b = _batch(5)
    Vm = tiny.config.vocab_size
    args = (b["input_ids"], b["image_features"], b["attention_mask"], 1, 6)
    start = torch.full((5,), tiny.config.decoder_start_token_id, dtype=torch.long, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    eng.gen_begin(*args)
    lg = eng.gen_step(start, 0)
    assert eng.lib.kmb_gen_embedded_step(eng.h) == -1
    nxt = eng.greedy_step(lg, embed_step=1)
    assert eng.lib.kmb_gen_embedded_step(eng.h) == 1
    rtok, _ = reference(lg, Vm)
    assert nxt.cpu().tolist() == rtok.tolist()
    _lib().check(eng.lib.kmb_gen_step(eng.h, None, 1, _p(eng._gen_logits), stream))
    assert eng.lib.kmb_gen_embedded_step(eng.h) == -1
    folded = eng._gen_logits[:, :Vm].clone()
    eng.gen_begin(*args)
    eng.gen_step(start, 0)
    plain = eng.gen_step(nxt.clone(), 1)[:, :Vm].clone()
    assert torch.equal(folded, plain)
    # the Python loop's form: gen_step on the very tensor greedy_step returned asks for the pending rows
    eng.gen_begin(*args)
    nxt2 = eng.greedy_step(eng.gen_step(start, 0), embed_step=1)
    assert torch.equal(eng.gen_step(nxt2, 1)[:, :Vm], plain) and eng.lib.kmb_gen_embedded_step(eng.h) == -1
    # without embed_step nothing is pending, and tokens = NULL keeps failing with kmb_gen_step's message
    eng.gen_begin(*args)
    eng.greedy_step(eng.gen_step(start, 0))
    assert eng.lib.kmb_gen_embedded_step(eng.h) == -1
    assert eng.lib.kmb_gen_step(eng.h, None, 1, _p(eng._gen_logits), stream) != 0
    assert "tokens = NULL but no kmb_gen_beam_step embedded" in eng.lib.kmb_last_error().decode()
    # kmb_gen_last_hidden still returns the step's decoder states after a fold (the tiny model's end where the embedding used to go)
    eng.gen_begin(*args)
    lg = eng.gen_step(start, 0)
    before = eng.gen_last_hidden().clone()
    eng.greedy_step(lg, embed_step=1)
    assert eng.lib.kmb_gen_embedded_step(eng.h) == 1 and torch.equal(eng.gen_last_hidden(), before)


@pytest.mark.parametrize("kw", [dict(max_length=12), dict(max_length=12, min_length=6), dict(max_length=2)],
                         ids=["len12", "len12_min6", "len2"])
def test_generate_tiny_device_path_equals_torch_path(tiny, kw):
    a, b = _both(tiny, dict(_batch(16), num_beams=1, return_scores=True, **kw))
    _same(a, b)
    assert a[0].shape[0] == 16 and a[0].shape[1] <= kw["max_length"]
    if kw.get("min_length"):
        assert not bool((a[0][:, 1:kw["min_length"]] == tiny.config.eos_token_id).any())
    assert bool((a[1] <= 0).all()) and bool(torch.isfinite(a[1]).all())
    plain = tiny.generate(**dict(_batch(16), num_beams=1, **kw))          # without return_scores: the bare ids
    assert torch.is_tensor(plain) and torch.equal(plain, a[0])


def test_generate_tiny_golden_ids_and_oracle_scores(tiny, gold_dir):
    """Case 0 of the golden fixture on the device path; its score against the oracle's teacher-forced fp32 sum of
    log-probabilities may be no further off than the torch path's (the bf16-against-fp32 gap of the parent path) + ATOL."""
    from oracle import goldenlib as G
    from oracle import kmbart_oracle as O
    gen = json.load(open(os.path.join(gold_dir, "tiny_generate.json")))
    case = gen["cases"][0]
    assert case["kwargs"] == {"num_beams": 1, "max_length": 12}
    ids, am = torch.tensor(gen["input_ids"]), torch.tensor(gen["attention_mask"])
    feats = G.golden_features(gen["regions"], seed=gen["seed"])
    kw = dict(input_ids=ids.to(DEV), image_features=[f.to(DEV) for f in feats], attention_mask=am.to(DEV), return_scores=True,
              **case["kwargs"])
    a, b = _both(tiny, kw)
    assert a[0].cpu().tolist() == case["ids"]
    _same(a, b)
    out = torch.tensor(case["ids"])
    cfg = tiny.config
    with torch.no_grad():
        _, logits, _ = O.forward(G.trained_state_dict(), G.tiny_config(), ids, feats, am, out[:, :-1], torch.ones_like(out[:, :-1]))
    logits = logits.double()
    for cur_len in range(1, min(int(cfg.min_length), out.shape[1])):      # the min_length ban of step cur_len
        logits[:, cur_len - 1, cfg.eos_token_id] = -INF
    lp = torch.log_softmax(logits, dim=-1).gather(2, out[:, 1:, None]).squeeze(2)
    is_eos = (out[:, 1:] == cfg.eos_token_id).long()
    live = (torch.cumsum(is_eos, dim=1) - is_eos) == 0                    # up to and including the first EOS
    want = (lp * live).sum(dim=1)
    gap_dev = (a[1].cpu().double() - want).abs().max().item()
    gap_torch = (b[1].cpu().double() - want).abs().max().item()
    print("greedy score gap to the fp32 oracle: device path %.3e, torch path %.3e" % (gap_dev, gap_torch))
    assert gap_dev <= gap_torch + ATOL, (gap_dev, gap_torch)


@pytest.fixture(scope="module")
def full():
    import bench
    from src.data.synthetic import make_batch
    from src.model import MultiModalBartConfig, MultiModalBartForConditionalGeneration
    torch.manual_seed(0)
    model = MultiModalBartForConditionalGeneration(MultiModalBartConfig.from_dict(dict(bench.VCG_BASE, dropout=0.0)))
    model.to(DEV).eval()
    b = make_batch(16, seed=3)
    return model, dict(input_ids=b["input_ids"].to(DEV), image_features=[f.to(DEV) for f in b["image_features"]],
                       attention_mask=b["attention_mask"].to(DEV), num_beams=1, max_length=12, return_scores=True)


def test_generate_fullsize_device_path_equals_torch_path(full):
    model, kw = full
    a, b = _both(model, kw)
    _same(a, b)
    assert a[0].shape[0] == 16


def test_generate_fullsize_without_eos(full):
    model, kw = full
    a, b = _both(model, dict(kw, eos_token_id=None))
    _same(a, b)
    assert a[0].shape == (16, 12)


def test_fallback_routing_and_sampling(tiny, monkeypatch):
    from kmbart.engine import Engine
    calls = []
    real = Engine.greedy_step
    monkeypatch.setattr(Engine, "greedy_step", lambda self, *a, **k: calls.append(1) or real(self, *a, **k))
    kw = dict(_batch(4), num_beams=1, max_length=10)
    tiny.generate(**kw)
    assert len(calls) >= 1                                   # plain greedy runs the device step
    for over in (dict(repetition_penalty=1.2), dict(no_repeat_ngram_size=2), dict(bad_words_ids=[[17]])):
        del calls[:]
        a, b = _both(tiny, dict(kw, return_scores=True, **over))
        assert not calls, over                               # score processors keep the torch loop
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    del calls[:]
    for flag in (False, 0, None):                            # falsy selects the torch loop
        tiny._device_greedy = flag
        try:
            tiny.generate(**kw)
        finally:
            del tiny._device_greedy
    tiny._engine.set_precision(True)                         # the fp32 validation mode keeps it too
    try:
        out = tiny.generate(**dict(kw, return_scores=True))
    finally:
        tiny._engine.set_precision(False)
    assert not calls and isinstance(out, tuple) and out[1].shape == (4,)
    torch.manual_seed(5)
    out = tiny.generate(**dict(kw, do_sample=True, top_k=8, return_scores=True))
    assert torch.is_tensor(out) and not calls                # one-beam sampling still returns the ids only
