"""GPU: the device sampler of generate(do_sample=True, num_beams=1) (kmb_sample_step, csrc/sample.hip) against an fp64
torch reference of transformers 3.0.2 top_k_top_p_filtering + softmax + torch.multinomial's exponential race, its tie
rules, its distribution, the finished-row bookkeeping, and same-seed agreement with the torch path of generate()."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
R, V = 320, 50265
LD = 50432            # what kmb_gen_step pads 50 265 columns to (197 blocks of 256)
TIE = 1e-5            # near-tie of the draw: best and second-best p / q closer than this, relative
BORDER = 1e-6         # a top-p boundary token's exclusive mass this close to top_p: the fp32 masses may decide either way


def _lib():
    from kmbart import _lib
    return _lib


def sample(logits, noise, T=1.0, top_k=0, top_p=1.0, ban=-1, unfinished=None, pad=0, eos=-1, ids=None, t=0, flag=None,
           V_=V):
    """kmb_sample_step on [rows, ld] logits; returns (tokens, info [rows, 2])."""
    L = _lib()
    rows = logits.shape[0]
    tok = torch.empty(rows, dtype=torch.int64, device=DEV)
    info = torch.empty((rows, 2), dtype=torch.float32, device=DEV)
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())   # noqa: E731
    L.check(L.load().kmb_sample_step(p(logits), logits.stride(0), V_, rows, float(T), int(top_k), float(top_p), int(ban),
                                     p(noise), noise.stride(0), p(unfinished), int(pad), int(eos), p(tok), p(ids), int(t),
                                     ids.stride(0) if ids is not None else 0, p(flag), p(info),
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return tok, info


def padded(x):
    buf = torch.full((x.shape[0], LD), float("nan"), dtype=torch.float32, device=DEV)   # padding must never be read as a token
    buf[:, :x.shape[1]] = x
    return buf


def reference(x, noise, T, top_k, top_p, ban=-1):
    """fp64 reference on the same fp32 x / T: kept mask, kept count, smallest kept value, token, near-tie rows, rows with
    a boundary token whose exclusive mass lies within TIE of top_p."""
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
    xk = x.double().masked_fill(~keep, -float("inf"))
    pk = torch.softmax(xk, dim=-1)
    ratio = pk / noise[:, :n].double()
    top2 = torch.topk(ratio, 2, dim=-1)[0]
    near = (top2[:, 0] - top2[:, 1]) <= TIE * top2[:, 0]
    kept_min = x.masked_fill(~keep, float("inf")).min(dim=-1)[0]
    return keep, keep.sum(-1), kept_min, ratio.argmax(-1), near, border


def logits_for(scale, seed, rows=R):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn((rows, V), generator=g, device=DEV) * scale


def exp_noise(rows, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.empty((rows, LD), device=DEV).exponential_(1, generator=g)


CASES = [(1.0, 0, 1.0), (1.0, 0, 0.9), (0.7, 50, 0.9), (1.3, 8, 1.0), (1.0, 1, 1.0), (1.0, 0, 0.0), (1.0, V + 7, 0.5)]


@pytest.mark.parametrize("scale", [0.05, 5.0], ids=["flat", "peaked"])
@pytest.mark.parametrize("T,top_k,top_p", CASES)
def test_filter_and_draw_match_fp64_reference(scale, T, top_k, top_p):
    x = logits_for(scale, seed=11)
    q = exp_noise(R, seed=12)
    for ban in ([-1, 7] if (T, top_k, top_p) == (0.7, 50, 0.9) else [-1]):
        tok, info = sample(padded(x), q, T, top_k, top_p, ban)
        keep, cnt, kmin, rtok, near, border = reference(x, q, T, top_k, top_p, ban)
        ok = ~border
        # flat rows put a token every ~2e-5 of mass, so a few percent of them have one within BORDER of the cut
        assert int(border.sum()) <= (R // 100 if scale > 1 else R * 15 // 100), int(border.sum())
        assert torch.equal(info[ok, 0].long(), cnt[ok]), (info[ok, 0][:8], cnt[ok][:8])
        assert torch.equal(info[ok, 1], kmin[ok])
        sure = ok & ~near
        assert int(sure.sum()) >= R * 3 // 4   # flat rows without top-k hold ~45 000 candidates: near-ties are common
        assert torch.equal(tok[sure], rtok[sure])
        assert bool(keep.gather(1, tok.view(-1, 1)).all())           # every token drawn was kept
        if ban >= 0:
            assert not bool((tok == ban).any())
    if (T, top_k, top_p) == (1.0, 1, 1.0):
        assert torch.equal(tok, x.argmax(-1))   # distinct random values: the maximum alone survives
    if top_p == 0.0:
        assert bool((info[:, 0] == 1).all())


def test_ties_at_the_kth_place_and_at_the_top_p_cut():
    x = torch.full((R, V), -30.0, device=DEV)
    # rows: values 5, 4, then five tokens of 3 at scattered indices -> top_k = 3 keeps all seven
    spots = torch.tensor([40000, 3, 1025, 50264, 2047], device=DEV)
    x[:, 100] = 5.0
    x[:, 60000 % V] = 4.0
    x[:, spots] = 3.0
    q = torch.ones((R, LD), device=DEV)
    tok, info = sample(padded(x), q, top_k=3)
    assert bool((info[:, 0] == 7).all()) and bool((info[:, 1] == 3.0).all())
    # top-p cut inside ten equal values (the rest is negligible): masses 0.1 each, top_p = 0.35 keeps the four tokens of
    # the lowest indices; give the 5th-lowest (removed) the smallest noise and the 4th-lowest the next smallest
    ties = torch.tensor([50000, 17, 4096, 1, 33333, 2048, 999, 12345, 1024, 45678], device=DEV)
    x = torch.full((R, V), -1e4, device=DEV)
    x[:, ties] = 0.0
    order = ties.sort()[0]
    q = torch.ones((R, LD), device=DEV)
    q[:, order[4]] = 1e-6
    q[:, order[3]] = 1e-3
    tok, info = sample(padded(x), q, top_p=0.35)
    assert bool((info[:, 0] == 4).all())
    assert bool((tok == order[3]).all()), tok[:4]
    # the same through the reference
    keep, cnt, _, rtok, _, _ = reference(x, q, 1.0, 0, 0.35)
    assert bool((cnt == 4).all()) and torch.equal(rtok, tok)


@pytest.mark.parametrize("scale,T,top_k,top_p", [(0.3, 1.0, 20, 1.0), (3.0, 1.0, 0, 0.9)], ids=["flat", "peaked"])
def test_distribution_chi_square(scale, T, top_k, top_p):
    from scipy.stats import chi2
    n = 4096
    x = logits_for(scale, seed=5, rows=1)
    keep, _, _, _, _, _ = reference(x, torch.ones((1, LD), device=DEV), T, top_k, top_p)
    p = torch.softmax(x.double().masked_fill(~keep, -float("inf")), dim=-1)[0]
    tok, _ = sample(padded(x.expand(n, V).contiguous()), exp_noise(n, seed=6), T, top_k, top_p)
    assert bool(keep[0, tok].all())
    counts = torch.bincount(tok, minlength=V).double()
    exp = p * n
    big = exp >= 5
    obs = torch.cat([counts[big], counts[~big].sum().view(1)])
    ex = torch.cat([exp[big], exp[~big].sum().view(1)])
    obs, ex = obs[ex > 0], ex[ex > 0]
    stat = float(((obs - ex) ** 2 / ex).sum())
    dof = obs.numel() - 1
    assert dof >= 3
    pval = float(chi2.sf(stat, dof))
    assert pval > 1e-3, (stat, dof, pval)


def test_bookkeeping_flag_ban_degenerate_rows_and_determinism():
    x = logits_for(2.0, seed=21)
    eos, pad = 2, 1
    x[: R // 2, eos] = 50.0                      # the first half picks eos for sure
    unf = torch.ones(R, dtype=torch.int64, device=DEV)
    unf[R - 10:] = 0                             # already finished
    ids = torch.full((R, 9), -5, dtype=torch.int64, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    q = exp_noise(R, seed=22)
    tok, _ = sample(padded(x), q, top_k=50, top_p=0.9, unfinished=unf, pad=pad, eos=eos, ids=ids, t=4, flag=flag)
    assert bool((tok[R - 10:] == pad).all()) and bool((tok[: R // 2] == eos).all())
    assert torch.equal(ids[:, 4], tok) and bool((ids[:, :4] == -5).all()) and bool((ids[:, 5:] == -5).all())
    assert bool((unf[: R // 2] == 0).all()) and bool((unf[R - 10:] == 0).all())
    assert torch.equal(unf[R // 2: R - 10], (tok[R // 2: R - 10] != eos).long())
    assert int(flag) == 1
    # every row finished: the flag stays 0
    flag.zero_()
    sample(padded(x), q, unfinished=torch.zeros(R, dtype=torch.int64, device=DEV), pad=pad, eos=eos, flag=flag)
    assert int(flag) == 0
    # the min_length ban: eos is never drawn, even where it dominates
    tok, _ = sample(padded(x), q, top_k=50, top_p=0.9, ban=eos)
    assert not bool((tok == eos).any())
    # degenerate rows: all -inf, all NaN, +inf, mixed NaN
    y = logits_for(1.0, seed=23)
    y[0] = -float("inf")
    y[1] = float("nan")
    y[2, 77] = float("inf")
    y[3, ::3] = float("nan")
    for T, k, p in CASES:
        tok, _ = sample(padded(y), q, T, k, p)
        assert bool(((tok >= 0) & (tok < V)).all()), tok[:4]
    # bit-identical reruns
    a, ia = sample(padded(x), q, 0.7, 50, 0.9)
    b, ib = sample(padded(x), q, 0.7, 50, 0.9)
    assert torch.equal(a, b) and torch.equal(ia, ib)


def test_same_seed_same_tokens_as_torch_multinomial():
    from src.model.model import _top_k_top_p_filtering
    x = logits_for(1.0, seed=31)
    xp = padded(x)
    for T, k, p in [(1.0, 50, 0.9), (0.7, 0, 0.95), (1.0, 0, 1.0)]:
        torch.manual_seed(123)
        lg = xp[:, :V] / T if T != 1.0 else xp[:, :V]
        lg = _top_k_top_p_filtering(lg.clone(), top_k=k, top_p=p)
        want = torch.multinomial(torch.softmax(lg, dim=-1), num_samples=1).squeeze(1)
        st_torch = torch.cuda.get_rng_state()
        torch.manual_seed(123)
        q = torch.empty((R, V), device=DEV).exponential_(1)
        st_dev = torch.cuda.get_rng_state()
        tok, _ = sample(xp, q, T, k, p)
        assert torch.equal(st_torch, st_dev)
        diff = tok != want
        assert int(diff.sum()) <= R // 100, int(diff.sum())
        if bool(diff.any()):
            _, _, _, _, near, border = reference(x, q, T, k, p)
            assert bool((near | border)[diff].all())


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


def _agree(a, b):
    n = min(a.shape[1], b.shape[1])
    return sum(ra == rb for ra, rb in zip(a[:, :n].tolist(), b[:, :n].tolist())) / a.shape[0]


def test_generate_device_sampling_matches_torch_path_fullsize():
    import bench
    from src.data.synthetic import make_batch
    from src.model import MultiModalBartConfig, MultiModalBartForConditionalGeneration
    torch.manual_seed(0)
    model = MultiModalBartForConditionalGeneration(MultiModalBartConfig.from_dict(dict(bench.VCG_BASE, dropout=0.0)))
    model.to(DEV).eval()
    b = make_batch(16, seed=3)
    kw = dict(input_ids=b["input_ids"].to(DEV), image_features=[f.to(DEV) for f in b["image_features"]],
              attention_mask=b["attention_mask"].to(DEV), do_sample=True, top_k=50, top_p=0.9, num_return_sequences=5,
              max_length=12)
    a, c, sa, sc = _generate_both(model, kw)
    assert a.shape[0] == 80 and int(a[:, 0].min()) == int(a[:, 0].max())
    assert _agree(a, c) >= 0.95, (a[:4].tolist(), c[:4].tolist())
    assert a.shape == c.shape and torch.equal(sa, sc)


def test_generate_device_sampling_matches_torch_path_trained_tiny():
    from oracle import goldenlib as G
    from oracle.make_golden import copy_task_batch
    from src.model import MultiModalBartConfig, MultiModalBartForConditionalGeneration
    ocfg = G.tiny_config()
    keys = ("vocab_size", "d_model", "encoder_layers", "decoder_layers", "encoder_attention_heads",
            "decoder_attention_heads", "encoder_ffn_dim", "decoder_ffn_dim", "max_position_embeddings",
            "image_feature_size", "img_feat_id", "cls_token_id", "dropout", "attention_dropout", "activation_dropout")
    model = MultiModalBartForConditionalGeneration(MultiModalBartConfig.from_dict({k: getattr(ocfg, k) for k in keys}))
    model.load_state_dict(G.trained_state_dict(), strict=False)
    model.to(DEV).eval()
    gb = copy_task_batch(9, 16)
    kw = dict(input_ids=gb["input_ids"].to(DEV), image_features=[f.to(DEV) for f in gb["image_features"]],
              attention_mask=gb["attention_mask"].to(DEV), do_sample=True, top_k=50, top_p=0.9,
              num_return_sequences=5, max_length=12)
    a, c, sa, sc = _generate_both(model, kw)
    assert a.shape[0] == 80
    assert _agree(a, c) >= 0.95, (a[:4].tolist(), c[:4].tolist())
    assert a.shape == c.shape and torch.equal(sa, sc)
    # min_length bans eos on the device path as on the torch path
    eos = model.config.eos_token_id
    m = model.generate(**dict(kw, min_length=6))
    assert not bool((m[:, 1:6] == eos).any())


def test_sample_step_rejects_bad_arguments():
    x = padded(logits_for(1.0, seed=41, rows=4))
    q = exp_noise(4, seed=42)
    for bad in (dict(T=0.0), dict(top_p=1.5), dict(top_k=-1), dict(ban=V)):
        with pytest.raises(_lib().KmbError):
            sample(x, q, **bad)
