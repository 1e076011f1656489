"""GPU: beam sampling on the device (kmb_beam_sample_step / kmb_gen_beam_sample_step, csrc/beam_sample.hip) against an fp64
torch reference of transformers 3.0.2 _generate_beam_search's sampling branch, torch.multinomial's exponential race on the
device, determinism, argument checks, the gen-handle form, and generate()'s routing and same-seed agreement with the host loop."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
V = 50265
LD = 50432            # what kmb_gen_step pads 50 265 columns to
TIE = 1e-4            # race keys (log domain) of neighbouring draws closer than this: fp32 rounding may swap them
BORDER = 1e-5         # a top-k boundary within this, relative: the fp32 filter may decide either way
BORDER_P = 3e-7       # a top-p cut whose exclusive mass lies this close to top_p (fp32 token masses, summed)


def _lib():
    from kmbart import _lib
    return _lib


def _p(x):
    return None if x is None else C.c_void_p(x.data_ptr())


def step(logits, noise, nb, add=None, T=1.0, top_k=0, top_p=1.0, ban=-1, eos=-1, V_=V, k=None, outs=None, scratch_floats=None):
    """kmb_beam_sample_step; outs: (out, next_scores, next_tokens, next_beam_idx) to write into."""
    L = _lib()
    R = logits.shape[0]
    B = R // nb
    k = 2 * nb if k is None else k
    if outs is None:
        outs = (torch.empty((B, max(k, 1), 2), dtype=torch.int32, device=DEV), torch.empty(R, dtype=torch.float32, device=DEV),
                torch.empty(R, dtype=torch.int64, device=DEV), torch.empty(R, dtype=torch.int32, device=DEV))
    out, ns, nt, ni = outs
    nscr = int(L.load().kmb_beam_sample_scratch(R)) if scratch_floats is None else scratch_floats
    scr = torch.empty(max(nscr, 1), dtype=torch.float32, device=DEV)
    L.check(L.load().kmb_beam_sample_step(_p(logits), logits.stride(0), V_, B, nb, _p(add), float(T), int(top_k), float(top_p), int(ban),
                                          _p(noise), noise.stride(0), int(k), _p(out), int(eos), _p(ns), _p(nt), _p(ni), _p(scr), nscr,
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return out, ns, nt, ni


def padded(x, ld):
    buf = torch.full((x.shape[0], ld), float("nan"), dtype=torch.float32, device=DEV)   # padding is never read as a token
    buf[:, :x.shape[1]] = x
    return buf


def reference(x, noise, nb, add, T, top_k, top_p, ban):
    """fp64 steps 1-6 per batch item: (draws [B, k] flat indices in draw order, their scores, unsure [B]: a near-tie of the
    race or a filter boundary within rounding)."""
    R, n = x.shape
    B, k = R // nb, 2 * nb
    s = torch.log_softmax(x.double(), dim=-1)
    if ban >= 0:
        s[:, ban] = -float("inf")
    s = (s + add.double()[:, None]) / T
    unsure = torch.zeros(R, dtype=torch.bool, device=DEV)
    keep = torch.ones_like(s, dtype=torch.bool)
    if top_k > 0:
        kk = min(max(top_k, 2), n)
        tv = torch.topk(s, min(kk + 1, n))[0]
        keep &= ~(s < tv[:, kk - 1:kk])
        if kk < n:
            unsure |= (tv[:, kk - 1] - tv[:, kk]).abs() <= BORDER * tv[:, kk - 1].abs()
    if top_p < 1.0:
        sm = s.masked_fill(~keep, -float("inf"))
        sv, si = torch.sort(sm, dim=-1, descending=True, stable=True)
        pr = torch.softmax(sv, dim=-1)
        excl = torch.cumsum(pr, dim=-1) - pr
        rm = excl > top_p
        rm[:, :3] = False
        # the cut: the last kept and the first removed token's exclusive mass within rounding of top_p
        n_kept = (~rm).sum(dim=-1)
        for at in ((n_kept - 1).clamp(3, n - 1), n_kept.clamp(3, n - 1)):
            unsure |= (excl.gather(1, at[:, None])[:, 0] - top_p).abs() <= BORDER_P
        keep &= ~torch.zeros_like(rm).scatter(1, si, rm)
    sf = s.masked_fill(~keep, -float("inf"))
    key = sf - torch.log(noise[:, :nb * n].reshape(R, n).double())
    key = key.view(B, nb * n)
    top = torch.topk(key, k + 1, dim=-1)
    draws = top[1][:, :k]
    gaps = (top[0][:, :-1] - top[0][:, 1:]).abs()
    unsure_b = unsure.view(B, nb).any(dim=1) | (gaps <= TIE).any(dim=1)
    scores = torch.gather(sf.view(B, nb * n), 1, draws)
    return draws, scores, unsure_b


def check_step(x, noise, nb, add, T, top_k, top_p, ban, eos, ld, min_sure=0.8):
    R, n = x.shape
    B, k = R // nb, 2 * nb
    out, ns, nt, ni = step(padded(x, ld), noise, nb, add, T, top_k, top_p, ban, eos, V_=n)
    draws, scores, unsure = reference(x, noise, nb, add, T, top_k, top_p, ban)
    flat = out[:, :, 1].long()
    sc = out[:, :, 0].contiguous().view(torch.float32)
    # scores sorted descending, each the drawn entry's filtered score
    assert bool((sc[:, 1:] <= sc[:, :-1]).all())
    sure = ~unsure
    assert int(sure.sum()) >= min_sure * B, int(sure.sum())
    for b in torch.nonzero(sure).flatten().tolist():
        want = draws[b].tolist()
        got = flat[b].tolist()
        assert sorted(got) == sorted(want), (b, got, want)
        ref_sc = dict(zip(want, scores[b].tolist()))
        for f, v in zip(got, sc[b].tolist()):
            assert abs(v - ref_sc[f]) <= 1e-5 * abs(ref_sc[f]) + 1e-5, (b, f, v, ref_sc[f])
    # next beams: the first nb non-EOS draws, in order
    for b in range(B):
        sel = [f for f in flat[b].tolist() if f % n != eos][:nb]
        assert nt[b * nb:(b + 1) * nb].tolist() == [f % n for f in sel]
        assert ni[b * nb:(b + 1) * nb].tolist() == [b * nb + f // n for f in sel]
        assert torch.equal(ns[b * nb:(b + 1) * nb], torch.tensor([sc[b, flat[b].tolist().index(f)].item() for f in sel],
                                                                  device=DEV))
    return out, ns, nt, ni


def exp_noise(B, cols, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.empty((B, cols), device=DEV).exponential_(1, generator=g)


@pytest.mark.parametrize("T,top_k,top_p,ban", [(1.0, 50, 0.9, -1), (0.7, 0, 1.0, -1), (1.3, 1, 1.0, 2), (1.0, 0, 1e-6, -1),
                                               (1.0, 0, 0.95, 2)])
def test_kernel_matches_fp64_reference_64x5(T, top_k, top_p, ban):
    # top-p over a whole 50k row: the cut's neighbours are ~1e-5 of mass apart, so some items sit within rounding of it
    B, nb = 64, 5
    g = torch.Generator(device=DEV).manual_seed(7)
    x = torch.randn((B * nb, V), generator=g, device=DEV) * 3.0
    add = torch.randn(B * nb, generator=g, device=DEV) * 2.0
    x[:5] = x[0]                      # identical beam rows of one item (the first step)
    add[:5] = 0.0
    noise = exp_noise(B, nb * V, seed=8)
    check_step(x, noise, nb, add, T, top_k, top_p, ban, eos=2, ld=LD, min_sure=0.5 if top_k == 0 and 0.5 < top_p < 1.0 else 0.8)


def test_kernel_small_shape_and_eos_among_top():
    B, nb, n = 2, 3, 40
    g = torch.Generator(device=DEV).manual_seed(11)
    x = torch.randn((B * nb, n), generator=g, device=DEV)
    x[:, 2] = 6.0                     # EOS is the most likely token of every row
    add = torch.zeros(B * nb, device=DEV)
    for T, top_k, top_p in [(1.0, 0, 1.0), (1.0, 5, 0.8), (2.0, 0, 0.5)]:
        for seed in range(4):
            noise = exp_noise(B, nb * n, seed=100 + seed)
            check_step(x, noise, nb, add, T, top_k, top_p, -1, eos=2, ld=48, min_sure=0.5)


def test_multinomial_is_the_exponential_race_on_the_device():
    g = torch.Generator(device=DEV).manual_seed(5)
    p = torch.softmax(torch.randn((64, 5 * 1000), generator=g, device=DEV) * 2, dim=-1)
    torch.manual_seed(99)
    want = torch.multinomial(p, 10)
    torch.manual_seed(99)
    q = torch.empty_like(p).exponential_(1)
    got = torch.topk(p / q, 10, dim=-1)[1]
    assert torch.equal(want, got)


def test_bit_identical_across_launches():
    B, nb = 16, 4
    g = torch.Generator(device=DEV).manual_seed(3)
    x = padded(torch.randn((B * nb, V), generator=g, device=DEV), LD)
    add = torch.randn(B * nb, generator=g, device=DEV)
    noise = exp_noise(B, nb * V, seed=4)
    for kw in (dict(top_k=50, top_p=0.9), dict(top_k=0, top_p=0.9), dict(top_k=0, top_p=1.0)):
        a = step(x, noise, nb, add, **kw)
        b = step(x, noise, nb, add, **kw)
        assert all(torch.equal(u, v) for u, v in zip(a, b))


def test_rejects_bad_arguments_and_launches_nothing():
    B, nb = 2, 3
    x = padded(torch.randn((B * nb, 100), device=DEV), 128)
    noise = exp_noise(B, nb * 100, seed=1)
    outs = (torch.full((B, 2 * nb, 2), -7, dtype=torch.int32, device=DEV), torch.full((B * nb,), -7.0, device=DEV),
            torch.full((B * nb,), -7, dtype=torch.int64, device=DEV), torch.full((B * nb,), -7, dtype=torch.int32, device=DEV))
    cases = [(x, noise, nb, bad) for bad in (dict(T=0.0), dict(top_p=0.0), dict(top_p=1.5), dict(top_k=-1), dict(ban=100), dict(eos=100),
                                             dict(k=4), dict(scratch_floats=10))]
    cases.append((x, exp_noise(B, 250, seed=2), nb, {}))                                    # ld_noise < num_beams * V
    cases.append((padded(torch.randn((18, 100), device=DEV), 128), exp_noise(2, 900, 2), 9, {}))   # 2 * num_beams > 16
    for lg, q, n, bad in cases:
        with pytest.raises(_lib().KmbError) as e:
            step(lg, q, n, V_=100, outs=outs, **bad)
        assert "kmb_beam_sample_step:" in str(e.value)
        torch.cuda.synchronize()
        assert all(bool((o == -7).all()) for o in outs), bad       # nothing was launched


def test_first_draw_pairs_follow_the_filtered_softmax():
    """Chi-square: over many items with identical rows and independent noise, the unordered pair of draws (num_beams = 1,
    k = 2) follows sampling without replacement from softmax of the filtered scores: P({i, j}) = p_i p_j / (1 - p_i) +
    p_j p_i / (1 - p_j)."""
    n, B = 6, 20000
    g = torch.Generator(device=DEV).manual_seed(21)
    row = torch.randn(n, generator=g, device=DEV)
    for T, top_k, crit in ((1.5, 0, 36.12), (1.0, 4, 20.52)):   # chi-square 0.999 quantiles for 14 and 5 degrees of freedom
        x = padded(row.expand(B, n).contiguous(), 8)
        noise = exp_noise(B, n, seed=22 + top_k)
        out, _, _, _ = step(x, noise, 1, torch.zeros(B, device=DEV), T=T, top_k=top_k, V_=n)
        s = torch.log_softmax(row.double(), dim=-1) / T
        if top_k:
            s = s.masked_fill(s < torch.topk(s, top_k)[0][-1], -float("inf"))
        p = torch.softmax(s, dim=-1).tolist()
        pairs = [(i, j) for i in range(n) for j in range(i + 1, n) if p[i] > 0 and p[j] > 0]
        exp_p = [p[i] * p[j] / (1 - p[i]) + p[j] * p[i] / (1 - p[j]) for i, j in pairs]
        got = out[:, :, 1].sort(dim=1)[0].tolist()
        counts = {pr: 0 for pr in pairs}
        for a, b in got:
            assert (a, b) in counts, (a, b)                    # a filtered token is never drawn
            counts[(a, b)] += 1
        chi2 = sum((counts[pr] - B * e) ** 2 / (B * e) for pr, e in zip(pairs, exp_p))
        assert chi2 < crit, (T, top_k, chi2)


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


def _batch(n, seed=9):
    from oracle.make_golden import copy_task_batch
    gb = copy_task_batch(seed, n)
    return dict(input_ids=gb["input_ids"].to(DEV), image_features=[f.to(DEV) for f in gb["image_features"]],
                attention_mask=gb["attention_mask"].to(DEV))


def _both(model, kw, seed=17):
    torch.manual_seed(seed)
    a = model.generate(**kw)
    model._device_sampling = False
    try:
        torch.manual_seed(seed)
        b = model.generate(**kw)
    finally:
        del model._device_sampling
    return a, b


def _rows_agree(a, b):
    if isinstance(a, tuple):
        a, b = a[0], b[0]
    n = min(a.shape[1], b.shape[1])
    return sum(ra == rb for ra, rb in zip(a[:, :n].tolist(), b[:, :n].tolist())) / a.shape[0]


def test_generate_device_beam_sampling_matches_host_loop_tiny():
    model = _tiny_model()
    kw = dict(_batch(8), do_sample=True, num_beams=5, top_k=50, top_p=0.9, max_length=12, num_return_sequences=2,
              min_length=4, return_scores=True, temperature=3.0)
    a, b = _both(model, kw)
    assert a[0].shape[0] == 16
    assert _rows_agree(a, b) >= 0.9, (a[0][:4].tolist(), b[0][:4].tolist())
    same = [i for i, (x, y) in enumerate(zip(a[0].tolist(), b[0].tolist())) if x == y]
    assert torch.allclose(a[1][same], b[1][same], atol=1e-4)
    eos = model.config.eos_token_id
    assert not bool((a[0][:, 1:4] == eos).any())


def test_generate_device_beam_sampling_matches_host_loop_fullsize():
    import bench
    from src.data.synthetic import make_batch
    from src.model import MultiModalBartConfig, MultiModalBartForConditionalGeneration
    torch.manual_seed(0)
    model = MultiModalBartForConditionalGeneration(MultiModalBartConfig.from_dict(dict(bench.VCG_BASE, dropout=0.0)))
    model.to(DEV).eval()
    b = make_batch(64, seed=3)
    kw = dict(input_ids=b["input_ids"].to(DEV), image_features=[f.to(DEV) for f in b["image_features"]],
              attention_mask=b["attention_mask"].to(DEV), do_sample=True, num_beams=5, top_k=50, top_p=0.9, max_length=8)
    a, c = _both(model, kw)
    assert a.shape[0] == 64
    assert _rows_agree(a, c) >= 0.9, (a[:4].tolist(), c[:4].tolist())


def test_routing(monkeypatch):
    model = _tiny_model()
    kw = dict(_batch(3), do_sample=True, num_beams=3, top_k=8, top_p=0.9, max_length=8)

    def boom(*a, **k):
        raise AssertionError("torch.multinomial called")
    with monkeypatch.context() as m:
        m.setattr(torch, "multinomial", boom)
        out = model.generate(**kw)                 # the device path draws no multinomial
        assert out.shape[0] == 3
        for over in (dict(repetition_penalty=1.2), dict(no_repeat_ngram_size=2)):
            with pytest.raises(AssertionError, match="multinomial"):
                model.generate(**dict(kw, **over))
        for flag in (False, 0, None):              # falsy selects the host loop, as for one beam
            model._device_sampling = flag
            try:
                with pytest.raises(AssertionError, match="multinomial"):
                    model.generate(**kw)
            finally:
                del model._device_sampling
        model._engine.set_precision(True)          # the fp32 validation mode keeps the host loop
        try:
            with pytest.raises(AssertionError, match="multinomial"):
                model.generate(**kw)
        finally:
            model._engine.set_precision(False)
        calls = []
        model._sampler = lambda probs, n: calls.append(1) or torch.topk(probs, n, dim=-1)[1]   # an explicit sampler: host loop
        try:
            model.generate(**kw)
            assert calls
        finally:
            del model._sampler
    # an unsupported shape (2 * num_beams > 16) falls back to the host loop and still agrees with it
    kw9 = dict(kw, num_beams=9)
    a, b = _both(model, kw9)
    assert torch.equal(a, b)


def test_gen_handle_form_reorders_and_embeds_like_explicit_calls():
    """At a step where the beams have diverged, kmb_gen_beam_sample_step (history reorder and next embedding folded into its
    merge, kmb_gen_embedded_step) followed by gen_step(NULL) gives the candidates and next logits of the stateless
    kmb_beam_sample_step + kmb_gen_reorder + gen_step on explicit tokens."""
    import bench
    from src.data.synthetic import make_batch
    from src.model import MultiModalBartConfig, MultiModalBartForConditionalGeneration
    torch.manual_seed(0)
    model = MultiModalBartForConditionalGeneration(MultiModalBartConfig.from_dict(dict(bench.VCG_BASE, dropout=0.0,
                                                                                       decoder_layers=2, encoder_layers=1)))
    model.to(DEV).eval()
    eng = model._need_engine()
    b = make_batch(4, seed=5)
    nb, Vm = 3, model.config.vocab_size
    args = (b["input_ids"].to(DEV), [f.to(DEV) for f in b["image_features"]], b["attention_mask"].to(DEV), nb, 6)
    kw = dict(temperature=2.0, top_k=50, top_p=0.9)
    res = []
    for folded in (True, False):
        eng.gen_begin(*args)
        tok = torch.full((4 * nb,), model.config.decoder_start_token_id, dtype=torch.long, device=DEV)
        lg = eng.gen_step(tok, 0)
        _, sc0, nt0, _ = eng.beam_sample_step(lg, nb, exp_noise(4, nb * Vm, seed=3), add=torch.zeros(4 * nb, device=DEV),
                                              reorder_step=0, **kw)
        lg1 = eng.gen_step(nt0.clone(), 1)
        noise1 = exp_noise(4, nb * Vm, seed=4)
        if folded:
            cand, sc1, nt1, ni1 = eng.beam_sample_step(lg1, nb, noise1, add=sc0, reorder_step=1, **kw)
            assert eng.lib.kmb_gen_embedded_step(eng.h) == 2
            lg2 = eng.gen_step(nt1, 2)
        else:
            cand, sc1, nt1, ni1 = eng.beam_sample_step(lg1.clone(), nb, noise1, add=sc0, **kw)   # stateless, no reorder
            eng.gen_reorder(ni1, 1)
            lg2 = eng.gen_step(nt1.clone(), 2)
        res.append((cand.clone(), ni1.clone(), lg2[:, :Vm].clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert not torch.equal(res[0][1].cpu(), torch.arange(4 * nb, dtype=torch.int32))   # the beams were permuted
    assert torch.equal(res[0][2], res[1][2])
