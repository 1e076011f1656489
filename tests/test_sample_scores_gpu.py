"""GPU: the log-probabilities of the device sampler (kmb_sample_scored_step / kmb_gen_sample_step, csrc/sample.hip) against an
fp64 torch reference (log_softmax over the reference's own kept set), their bookkeeping, degenerate rows, determinism, argument
checks, the folded next-step embedding, and generate(num_beams=1, return_logprobs=True) / sample_sentence on the device path
against the torch loop (model._device_sampling = False) and the fp32 oracle.  ATOL is the project's fp32 score tolerance
(tests/test_greedy_gpu.py)."""
import ctypes as C
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS = 64
ATOL = 1e-4
BORDER = 1e-6         # a top-p boundary token's exclusive mass this close to top_p: the fp32 masses may decide either way
MAX_BORDER_ROWS = 16
# CASES of tests/test_sample_gpu.py (temperature, top_k, top_p); its last top_k is that file's V + 7 = 50 272
CASES = [(1.0, 0, 1.0), (1.0, 0, 0.9), (0.7, 50, 0.9), (1.3, 8, 1.0), (1.0, 1, 1.0), (1.0, 0, 0.0), (1.0, 50265 + 7, 0.5)]
VS = [1000, 50265, 65536]   # the kernel's 16-, 52- and 64-values-per-lane instances


def _lib():
    from kmbart import _lib
    return _lib


def _p(x):
    return None if x is None else C.c_void_p(x.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ld(V):
    return (V + 255) // 256 * 256


@functools.lru_cache(maxsize=None)
def inputs(V, scale):
    """(x [ROWS, V], padded logits [ROWS, LD] with NaN padding, noise [ROWS, LD]) from CPU generators: the same bits everywhere."""
    x = (torch.randn((ROWS, V), generator=torch.Generator().manual_seed(11)) * scale).to(DEV)
    q = torch.empty((ROWS, _ld(V))).exponential_(1, generator=torch.Generator().manual_seed(12)).to(DEV)
    return x, padded(x), q


def padded(x):
    buf = torch.full((x.shape[0], _ld(x.shape[1])), float("nan"), dtype=torch.float32, device=DEV)
    buf[:, :x.shape[1]] = x
    return buf


def plain(logits, noise, V, T=1.0, top_k=0, top_p=1.0, ban=-1):
    """kmb_sample_step: (tokens, info)."""
    L = _lib()
    rows = logits.shape[0]
    tok = torch.empty(rows, dtype=torch.int64, device=DEV)
    info = torch.empty((rows, 2), dtype=torch.float32, device=DEV)
    L.check(L.load().kmb_sample_step(_p(logits), logits.stride(0), V, rows, float(T), int(top_k), float(top_p), int(ban), _p(noise),
                                     noise.stride(0), None, 0, -1, _p(tok), None, 0, 0, None, _p(info), _stream()))
    torch.cuda.synchronize()
    return tok, info


def scored_raw(logits, noise, V, T=1.0, top_k=0, top_p=1.0, ban=-1, unfinished=None, pad=0, eos=-1, tok=None, ids=None, t=0,
               flag=None, info=None, lsum=None, lout=None, ld_lp=1, rows=None):
    rows = logits.shape[0] if rows is None else rows
    return _lib().load().kmb_sample_scored_step(
        _p(logits), logits.stride(0), V, rows, float(T), int(top_k), float(top_p), int(ban), _p(noise), noise.stride(0),
        _p(unfinished), int(pad), int(eos), _p(tok), _p(ids), int(t), ids.stride(0) if ids is not None else 0, _p(flag), _p(info),
        _p(lsum), _p(lout), int(ld_lp), _stream())


def scored(logits, noise, V, T=1.0, top_k=0, top_p=1.0, ban=-1, unfinished=None, pad=0, eos=-1, lsum=None, want_out=True):
    """kmb_sample_scored_step: (tokens, info, logprob_out [rows])."""
    rows = logits.shape[0]
    tok = torch.empty(rows, dtype=torch.int64, device=DEV)
    info = torch.empty((rows, 2), dtype=torch.float32, device=DEV)
    lout = torch.full((rows,), 77.0, dtype=torch.float32, device=DEV) if want_out else None
    _lib().check(scored_raw(logits, noise, V, T, top_k, top_p, ban, unfinished, pad, eos, tok, None, 0, None, info, lsum, lout))
    torch.cuda.synchronize()
    return tok, info, lout


def reference(x, T, top_k, top_p, ban=-1):
    """fp64 reference on the same fp32 x / T, constructed as reference() of tests/test_sample_gpu.py: (kept mask, fp64
    log_softmax over the kept set, rows with a boundary token whose exclusive mass lies within BORDER of top_p)."""
    x = x.clone()
    if ban >= 0:
        x[:, ban] = -float("inf")
    if T != 1.0:
        x = (x.double() / float(torch.tensor(T, dtype=torch.float32))).float()   # correctly rounded fp32 x / fp32 T
    n = x.shape[1]
    keep = torch.ones_like(x, dtype=torch.bool)
    if top_k > 0:
        k = min(max(top_k, 1), n)
        keep &= ~(x < torch.topk(x, k)[0][:, -1:])
    xd = x.double().masked_fill(~keep, -float("inf"))
    border = torch.zeros(x.shape[0], dtype=torch.bool, device=x.device)
    if top_p < 1.0:
        sv, si = torch.sort(xd, dim=-1, descending=True, stable=True)
        pr = torch.softmax(sv, dim=-1)
        excl = torch.cumsum(pr, dim=-1) - pr
        rm = excl > top_p
        rm[:, 0] = False
        border = ((excl[:, 1:] - top_p).abs() <= BORDER).any(dim=-1)   # rank 0 is kept whatever its mass
        keep &= ~torch.zeros_like(rm).scatter(1, si, rm)
    logp = torch.log_softmax(x.double().masked_fill(~keep, -float("inf")), dim=-1)
    return keep, logp, border


# ------------------------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("scale", [0.05, 5.0], ids=["flat", "peaked"])
@pytest.mark.parametrize("V", VS)
def test_logprobs_match_fp64_reference_and_tokens_match_plain_step(V, scale):
    x, xp, q = inputs(V, scale)
    for T, top_k, top_p in CASES:
        for ban in ([-1, 7] if (T, top_k, top_p) == (0.7, 50, 0.9) else [-1]):
            tag = (V, scale, T, top_k, top_p, ban)
            ptok, pinfo = plain(xp, q, V, T, top_k, top_p, ban)
            tok = torch.empty(ROWS, dtype=torch.int64, device=DEV)
            info = torch.empty((ROWS, 2), dtype=torch.float32, device=DEV)
            grid = torch.full((ROWS, 7), 77.0, dtype=torch.float32, device=DEV)     # logprob_out: column 3, in place
            lsum = torch.full((ROWS,), 0.5, dtype=torch.float32, device=DEV)
            _lib().check(scored_raw(xp, q, V, T, top_k, top_p, ban, tok=tok, info=info, lsum=lsum, lout=grid[:, 3], ld_lp=7))
            torch.cuda.synchronize()
            assert torch.equal(tok, ptok) and torch.equal(info, pinfo), tag
            lp = grid[:, 3].clone()
            assert bool((grid[:, :3] == 77.0).all()) and bool((grid[:, 4:] == 77.0).all()), tag
            assert torch.equal(lsum, 0.5 + lp), tag
            assert bool(torch.isfinite(lp).all()) and bool((lp <= 0).all()), tag
            if top_k == 1 or top_p == 0.0:
                assert bool((info[:, 0] == 1).all()) and bool((lp == 0).all()), tag
            keep, logp, border = reference(x, T, top_k, top_p, ban)
            nb = int(border.sum())
            ok = ~border
            want = logp.gather(1, tok.view(-1, 1)).squeeze(1)
            err = (lp.double() - want)[ok].abs().max().item()
            print("V=%d scale=%g T=%g top_k=%d top_p=%g ban=%d: border rows %d, max |lp - fp64| %.3e" % (tag + (nb, err)))
            assert nb <= MAX_BORDER_ROWS, (tag, nb)
            assert bool(keep.gather(1, tok.view(-1, 1))[ok].all()), tag
            assert err <= ATOL, (tag, err)
            if ban >= 0:
                assert not bool((tok == ban).any())


# ------------------------------------------------------------------------------------------------ 2. bookkeeping
def test_bookkeeping_finished_rows_eos_rows_and_no_unfinished():
    V, EOS, PAD = 1000, 2, 1
    half = ROWS // 2
    x = inputs(V, 5.0)[0].clone()
    q = inputs(V, 5.0)[2].clone()
    x[:half, EOS] = x[:half].max(dim=1).values     # EOS ties with the row maximum: kept, with a real share of the mass ...
    q[:half, EOS] = 1e-6                           # ... and sure to win the race
    xp = padded(x)
    unf = torch.ones(ROWS, dtype=torch.int64, device=DEV)
    unf[ROWS - 10:] = 0                            # already finished
    live = unf.bool().clone()
    lsum = torch.full((ROWS,), 0.5, dtype=torch.float32, device=DEV)
    tok, info, lout = scored(xp, q, V, 1.0, 50, 0.9, unfinished=unf, pad=PAD, eos=EOS, lsum=lsum)
    _, logp, border = reference(x, 1.0, 50, 0.9)
    assert int(border.sum()) <= MAX_BORDER_ROWS
    assert bool((tok[~live] == PAD).all()) and bool((tok[:half] == EOS).all())
    assert bool((lout[~live] == 0).all()) and bool((lsum[~live] == 0.5).all())          # a finished row writes 0, adds nothing
    drawn = torch.where(live, tok, torch.zeros_like(tok))
    want = logp.gather(1, drawn.view(-1, 1)).squeeze(1)
    assert (lout.double() - want)[live & ~border].abs().max().item() <= ATOL
    assert torch.equal(lsum[live], (0.5 + lout)[live])                                  # the EOS rows add their own lp ...
    assert bool((lout[:half] < -0.5).all())                                             # ... which is at most log(1/2) here
    assert bool((unf[:half] == 0).all()) and torch.equal(unf[half:], (live & (tok != EOS)).long()[half:])
    # no `unfinished`: every row adds
    lsum = torch.full((ROWS,), 0.5, dtype=torch.float32, device=DEV)
    tok2, _, lout2 = scored(xp, q, V, 1.0, 50, 0.9, lsum=lsum)
    assert torch.equal(lsum, 0.5 + lout2)
    want2 = logp.gather(1, tok2.view(-1, 1)).squeeze(1)
    assert (lout2.double() - want2)[~border].abs().max().item() <= ATOL
    assert torch.equal(tok2[live], tok[live]) and torch.equal(lout2[live], lout[live])
    # only the sum, no per-step output
    lsum3 = torch.full((ROWS,), 0.5, dtype=torch.float32, device=DEV)
    tok3, _, none = scored(xp, q, V, 1.0, 50, 0.9, lsum=lsum3, want_out=False)
    assert none is None and torch.equal(lsum3, lsum) and torch.equal(tok3, tok2)


# ------------------------------------------------------------------------------------------------ 3. degenerate rows
@pytest.mark.parametrize("V", [1000, 50265])
def test_degenerate_rows(V):
    y = inputs(V, 1.0)[0].clone()
    q = inputs(V, 1.0)[2]
    y[0] = -float("inf")
    y[1] = float("nan")
    y[2, 77] = float("inf")
    y[3, ::3] = float("nan")
    yp = padded(y)
    for T, k, p in CASES:
        tok, info, lout = scored(yp, q, V, T, k, p)
        ptok, pinfo = plain(yp, q, V, T, k, p)
        assert torch.equal(tok, ptok) and torch.equal(info, pinfo)
        assert bool(((tok >= 0) & (tok < V)).all())
        assert bool(torch.isfinite(lout).all()) and bool((lout <= 0).all()), (T, k, p, lout[:4].tolist())
        for r in (0, 1):                                          # every kept token has mass 1: uniform over the kept set
            assert abs(float(lout[r]) + math.log(float(info[r, 0]))) <= ATOL, (T, k, p, r, float(lout[r]), float(info[r, 0]))
        assert int(tok[2]) == 77 and float(lout[2]) == 0.0        # a single +inf holds all the mass
        if k == 0 and p == 1.0:
            assert float(info[0, 0]) == V and float(info[1, 0]) == V


# ------------------------------------------------------------------------------------------------ 4. determinism
def test_bit_identical_reruns():
    V = 50265
    _, xp, q = inputs(V, 0.05)
    for T, k, p in [(0.7, 50, 0.9), (1.0, 0, 1.0), (1.0, 0, 0.9)]:
        runs = []
        for _ in range(2):
            lsum = torch.full((ROWS,), 0.5, dtype=torch.float32, device=DEV)
            tok, info, lout = scored(xp, q, V, T, k, p, lsum=lsum)
            runs.append((tok, info, lout, lsum))
        for a, b in zip(*runs):
            assert torch.equal(a, b)


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


def _batch(n, seed=9, dev=DEV):
    from oracle.make_golden import copy_task_batch
    gb = copy_task_batch(seed, n)
    return dict(input_ids=gb["input_ids"].to(dev), image_features=[f.to(dev) for f in gb["image_features"]],
                attention_mask=gb["attention_mask"].to(dev))


# ------------------------------------------------------------------------------------------------ 5. bad arguments
def test_bad_arguments_fail_with_the_entrys_name_and_launch_nothing(tiny):
    L = _lib()
    lib = L.load()
    V = 1000
    _, xp, q = inputs(V, 5.0)
    R = 4
    tok = torch.full((R,), -7, dtype=torch.int64, device=DEV)
    lsum = torch.full((R,), 0.5, dtype=torch.float32, device=DEV)
    lout = torch.full((R,), 77.0, dtype=torch.float32, device=DEV)
    for bad in (dict(ld_lp=0), dict(ld_lp=-3), dict(T=0.0), dict(top_p=1.5), dict(top_k=-1), dict(ban=V)):
        assert scored_raw(xp, q, V, tok=tok, lsum=lsum, lout=lout, rows=R, **bad) != 0, bad
        msg = lib.kmb_last_error().decode()
        assert msg.startswith("kmb_sample_scored_step: "), (bad, msg)
    torch.cuda.synchronize()
    assert bool((tok == -7).all()) and bool((lsum == 0.5).all()) and bool((lout == 77.0).all())
    assert scored_raw(xp, q, V, tok=tok, lsum=lsum, lout=None, ld_lp=0, rows=R) == 0      # ld_logprob matters with an output only
    torch.cuda.synchronize()
    assert bool((lsum < 0.5).all()) and bool((lout == 77.0).all()) and bool((tok >= 0).all())
    # the decode loop's form
    eng = tiny._need_engine()
    Vm = tiny.config.vocab_size
    b = _batch(R)
    start = torch.full((R,), tiny.config.decoder_start_token_id, dtype=torch.long, device=DEV)
    noise = torch.empty((R, Vm), device=DEV).exponential_(1)
    tok.fill_(-7), lsum.fill_(0.5), lout.fill_(77.0)

    def gen_call(h, lg, T=1.0, top_k=0, top_p=1.0, ban=-1, ld_lp=1, embed_step=-1):
        return lib.kmb_gen_sample_step(h, _p(lg), lg.stride(0), float(T), int(top_k), float(top_p), int(ban), _p(noise), noise.stride(0),
                                       None, 0, -1, _p(tok), None, 0, 0, None, None, _p(lsum), _p(lout), int(ld_lp), int(embed_step),
                                       _stream())

    eng.gen_begin(b["input_ids"], b["image_features"], b["attention_mask"], 1, 6)
    lg = eng.gen_step(start, 0)
    for bad in (dict(embed_step=-2), dict(ld_lp=0), dict(T=0.0), dict(top_p=1.5), dict(top_k=-1), dict(ban=Vm)):
        assert gen_call(eng.h, lg, **bad) != 0, bad
        msg = lib.kmb_last_error().decode()
        assert msg.startswith("kmb_gen_sample_step: "), (bad, msg)
        assert lib.kmb_gen_embedded_step(eng.h) == -1
    two = _batch(R // 2)
    eng.gen_begin(two["input_ids"], two["image_features"], two["attention_mask"], 2, 6)       # two beams: R rows again
    lg = eng.gen_step(start, 0)
    assert gen_call(eng.h, lg, embed_step=1) != 0
    msg = lib.kmb_last_error().decode()
    assert msg.startswith("kmb_gen_sample_step: ") and "num_beams == 1" in msg, msg
    # a handle that never saw kmb_gen_begin
    cfg = L.KmbConfig(vocab_size=50320, d_model=768, encoder_layers=6, decoder_layers=6, encoder_attention_heads=12,
                      decoder_attention_heads=12, encoder_ffn_dim=3072, decoder_ffn_dim=3072, max_position_embeddings=1024,
                      extra_pos_embeddings=2, image_feature_size=2052, pad_token_id=1, bos_token_id=0, eos_token_id=2,
                      img_feat_id=50273, cls_token_id=50276, scale_embedding=0, dropout=0.1, attention_dropout=0.0,
                      activation_dropout=0.0, layer_norm_eps=1e-5)
    h = C.c_void_p()
    L.check(lib.kmb_create(C.byref(cfg), C.byref(h)))
    try:
        assert gen_call(h, lg) != 0
        msg = lib.kmb_last_error().decode()
        assert msg.startswith("kmb_gen_sample_step: ") and "kmb_gen_begin" in msg, msg
    finally:
        lib.kmb_destroy(h)
    torch.cuda.synchronize()
    assert bool((tok == -7).all()) and bool((lsum == 0.5).all()) and bool((lout == 77.0).all())
    eng.gen_begin(b["input_ids"], b["image_features"], b["attention_mask"], 1, 6)           # the same buffers, good arguments
    lg = eng.gen_step(start, 0)
    assert gen_call(eng.h, lg, embed_step=1) == 0 and lib.kmb_gen_embedded_step(eng.h) == 1
    torch.cuda.synchronize()
    assert bool(((tok >= 0) & (tok < Vm)).all()) and bool((lout <= 0).all()) and torch.equal(lsum, 0.5 + lout)


# ------------------------------------------------------------------------------------------------ 6. the fold
def test_folded_embedding_is_the_embedding_launch(tiny):
    """sample_step(embed_step = 1) + kmb_gen_step(tokens = NULL, 1) against gen_step(next_tokens, 1) after a fresh gen_begin."""
    eng = tiny._need_engine()
    b = _batch(5)
    Vm = tiny.config.vocab_size
    args = (b["input_ids"], b["image_features"], b["attention_mask"], 1, 6)
    start = torch.full((5,), tiny.config.decoder_start_token_id, dtype=torch.long, device=DEV)
    noise = torch.empty((5, Vm)).exponential_(1, generator=torch.Generator().manual_seed(3)).to(DEV)
    kw = dict(top_k=8, top_p=0.9)
    eng.gen_begin(*args)
    lg = eng.gen_step(start, 0)
    assert eng.lib.kmb_gen_embedded_step(eng.h) == -1
    lsum = torch.zeros(5, dtype=torch.float32, device=DEV)
    nxt = eng.sample_step(lg, noise, logprob_sum=lsum, embed_step=1, **kw)
    assert eng.lib.kmb_gen_embedded_step(eng.h) == 1
    assert torch.equal(nxt, eng.sample_step(lg.clone(), noise, **kw))          # the plain step's tokens
    _lib().check(eng.lib.kmb_gen_step(eng.h, None, 1, _p(eng._gen_logits), _stream()))
    assert eng.lib.kmb_gen_embedded_step(eng.h) == -1
    folded = eng._gen_logits[:, :Vm].clone()
    eng.gen_begin(*args)
    eng.gen_step(start, 0)
    plain_lg = eng.gen_step(nxt.clone(), 1)[:, :Vm].clone()
    assert torch.equal(folded, plain_lg)
    # the Python loop's form: gen_step on the very tensor sample_step returned asks for the pending rows
    eng.gen_begin(*args)
    nxt2 = eng.sample_step(eng.gen_step(start, 0), noise, embed_step=1, **kw)
    assert torch.equal(nxt2, nxt)
    assert torch.equal(eng.gen_step(nxt2, 1)[:, :Vm], plain_lg) and eng.lib.kmb_gen_embedded_step(eng.h) == -1
    # without embed_step nothing is pending, scored or not
    eng.gen_begin(*args)
    eng.sample_step(eng.gen_step(start, 0), noise, logprob_sum=lsum, **kw)
    assert eng.lib.kmb_gen_embedded_step(eng.h) == -1
    eng.sample_step(eng._gen_logits, noise, **kw)
    assert eng.lib.kmb_gen_embedded_step(eng.h) == -1
    assert eng.lib.kmb_gen_step(eng.h, None, 1, _p(eng._gen_logits), _stream()) != 0
    # edited logits take the stateless form: nothing is folded
    eng.gen_begin(*args)
    lg = eng.gen_step(start, 0)
    lg[:, 0] -= 1.0
    eng.sample_step(lg, noise, logprob_sum=lsum, embed_step=1, **kw)
    assert eng.lib.kmb_gen_embedded_step(eng.h) == -1
    # kmb_gen_last_hidden still returns the step's decoder states after a fold
    eng.gen_begin(*args)
    lg = eng.gen_step(start, 0)
    before = eng.gen_last_hidden().clone()
    eng.sample_step(lg, noise, embed_step=1, **kw)
    assert eng.lib.kmb_gen_embedded_step(eng.h) == 1 and torch.equal(eng.gen_last_hidden(), before)


# ------------------------------------------------------------------------------------------------ 7. generate
def _generate_both(model, kw, seed=17):
    torch.manual_seed(seed)
    a = model.generate(**kw)
    sa = torch.cuda.get_rng_state()
    model._device_sampling = False
    try:
        torch.manual_seed(seed)
        b = model.generate(**kw)
        sb = torch.cuda.get_rng_state()
    finally:
        del model._device_sampling
    return a, b, sa, sb


def _consistent(model, ids, lp, eos):
    from src.model import GenerationLogprobs
    assert isinstance(lp, GenerationLogprobs)
    n = ids.shape[0]
    assert lp.token_logprobs.shape == (n, ids.shape[1] - 1) and lp.sum_logprobs.shape == (n,)
    for t in lp:
        assert t.dtype == torch.float32 and t.device == ids.device and bool(torch.isfinite(t).all()) and bool((t <= 0).all())
    assert (lp.sum_logprobs - lp.token_logprobs.sum(1)).abs().max().item() <= ATOL
    is_eos = (ids[:, 1:] == eos).long()
    after = (torch.cumsum(is_eos, dim=1) - is_eos) > 0                     # strictly after the first EOS
    assert bool((lp.token_logprobs[after] == 0).all())


def _same_rows(a, b):
    """Rows whose ids agree on the two paths (padded to a common length the paths share by construction)."""
    assert a.shape == b.shape
    return (a == b).all(dim=1)


def _device_against_torch(model, kw):
    (a, la), (c, lc), sa, sc = _generate_both(model, kw)
    assert torch.equal(sa, sc)
    same = _same_rows(a, c)
    assert float(same.float().mean()) >= 0.95, (a[:4].tolist(), c[:4].tolist())
    dt = (la.token_logprobs - lc.token_logprobs)[same].abs().max().item()
    ds = (la.sum_logprobs - lc.sum_logprobs)[same].abs().max().item()
    print("device against torch path: %d of %d rows equal, token_logprobs %.3e, sum_logprobs %.3e" % (int(same.sum()), len(same), dt, ds))
    assert dt <= ATOL and ds <= ATOL, (dt, ds)
    return a, la, c, lc, same


def test_generate_tiny_logprobs_device_path_against_torch_path(tiny):
    eos = tiny.config.eos_token_id
    kw = dict(_batch(16), do_sample=True, top_k=50, top_p=1.0, max_length=12, return_logprobs=True)
    a, la, _, lc, _ = _device_against_torch(tiny, kw)
    _consistent(tiny, a, la, eos)
    torch.manual_seed(17)
    bare = tiny.generate(**dict(kw, return_logprobs=False))
    assert torch.is_tensor(bare) and torch.equal(bare, a)
    # top-p and min_length: shapes, finiteness, the EOS ban, internal consistency
    torch.manual_seed(18)
    m, lm = tiny.generate(**dict(kw, top_p=0.9, min_length=6))
    assert m.shape[0] == 16 and m.shape[1] <= 12 and not bool((m[:, 1:6] == eos).any())
    _consistent(tiny, m, lm, eos)
    tiny._device_sampling = False
    try:
        torch.manual_seed(18)
        m2, lm2 = tiny.generate(**dict(kw, top_p=0.9, min_length=6))
    finally:
        del tiny._device_sampling
    _consistent(tiny, m2, lm2, eos)


# ------------------------------------------------------------------------------------------------ 8. the oracle
def test_generate_tiny_sum_logprobs_against_the_oracle(tiny):
    """The oracle's teacher-forced fp32 log-probabilities of the sampled ids, summed up to and including the first EOS: the
    device path may be no further off than the torch path (which reads the same bf16 logits) + ATOL."""
    from oracle import goldenlib as G
    from oracle import kmbart_oracle as O
    cfg = tiny.config
    cpu = _batch(16, dev="cpu")
    kw = dict(_batch(16), do_sample=True, top_k=0, top_p=1.0, temperature=1.0, min_length=0, max_length=12, return_logprobs=True)
    a, la, c, lc, same = _device_against_torch(tiny, kw)
    out = a.cpu()
    with torch.no_grad():
        _, logits, _ = O.forward(G.trained_state_dict(), G.tiny_config(), cpu["input_ids"], cpu["image_features"],
                                 cpu["attention_mask"], out[:, :-1], torch.ones_like(out[:, :-1]))
    lp = torch.log_softmax(logits.double(), dim=-1).gather(2, out[:, 1:, None]).squeeze(2)
    is_eos = (out[:, 1:] == cfg.eos_token_id).long()
    live = (torch.cumsum(is_eos, dim=1) - is_eos) == 0
    want = (lp * live).sum(dim=1)
    same = same.cpu()
    gap_dev = (la.sum_logprobs.cpu().double() - want)[same].abs().max().item()
    gap_torch = (lc.sum_logprobs.cpu().double() - want)[same].abs().max().item()
    print("sampled sum_logprobs gap to the fp32 oracle: device path %.3e, torch path %.3e" % (gap_dev, gap_torch))
    assert gap_dev <= gap_torch + ATOL, (gap_dev, gap_torch)


# ------------------------------------------------------------------------------------------------ 9. sample_sentence
def test_sample_sentence_is_the_generate_call_it_stands_for(tiny):
    import types
    from src.model.utils import sample_sentence
    cfg = tiny.config
    tok = types.SimpleNamespace(bos_token_id=cfg.bos_token_id, pad_token_id=cfg.pad_token_id, eos_token_id=cfg.eos_token_id)
    b = _batch(8)
    torch.manual_seed(23)
    ids, sums = sample_sentence(tiny, b["input_ids"], b["image_features"], b["attention_mask"], tok, top_k=20, top_p=0.95, max_length=10)
    assert ids.shape[0] == 8 and 2 <= ids.shape[1] <= 10 and sums.shape == (8, 1) and sums.dtype == torch.float32
    assert bool((ids[:, 0] == cfg.bos_token_id).all())
    torch.manual_seed(23)
    want, lp = tiny.generate(**dict(b, do_sample=True, num_beams=1, return_logprobs=True, top_k=20, top_p=0.95, max_length=10,
                                    temperature=1.0, min_length=0, num_return_sequences=1, repetition_penalty=1.0,
                                    no_repeat_ngram_size=0, bad_words_ids=None, decoder_start_token_id=cfg.bos_token_id,
                                    pad_token_id=cfg.pad_token_id, eos_token_id=cfg.eos_token_id))
    assert torch.equal(ids, want) and torch.equal(sums, lp.sum_logprobs[:, None])


# ------------------------------------------------------------------------------------------------ 10. greedy
def test_greedy_return_logprobs(tiny):
    kw = dict(_batch(16), num_beams=1, max_length=12)
    bare = tiny.generate(**kw)
    ids, scores = tiny.generate(**dict(kw, return_scores=True))
    a, la = tiny.generate(**dict(kw, return_logprobs=True))
    assert torch.equal(a, bare) and torch.equal(ids, bare)
    _consistent(tiny, a, la, tiny.config.eos_token_id)
    assert (la.sum_logprobs - scores).abs().max().item() <= ATOL
    tiny._device_greedy = False
    try:
        c, lc = tiny.generate(**dict(kw, return_logprobs=True))
    finally:
        del tiny._device_greedy
    assert torch.equal(c, a)
    assert (la.token_logprobs - lc.token_logprobs).abs().max().item() <= ATOL
    assert (la.sum_logprobs - lc.sum_logprobs).abs().max().item() <= ATOL
    with pytest.raises(ValueError, match="num_beams == 1"):
        tiny.generate(**dict(kw, num_beams=2, return_logprobs=True))


# ------------------------------------------------------------------------------------------------ 11. full size
def test_generate_fullsize_logprobs_device_path_against_torch_path():
    import bench
    from src.data.synthetic import make_batch
    from src.model import MultiModalBartConfig, MultiModalBartForConditionalGeneration
    torch.manual_seed(0)
    model = MultiModalBartForConditionalGeneration(MultiModalBartConfig.from_dict(dict(bench.VCG_BASE, dropout=0.0)))
    model.to(DEV).eval()
    b = make_batch(16, seed=3)
    kw = dict(input_ids=b["input_ids"].to(DEV), image_features=[f.to(DEV) for f in b["image_features"]],
              attention_mask=b["attention_mask"].to(DEV), do_sample=True, top_k=50, num_return_sequences=5, max_length=8,
              return_logprobs=True)
    a, la, _, _, _ = _device_against_torch(model, kw)
    assert a.shape[0] == 80
    _consistent(model, a, la, model.config.eos_token_id)
