"""Plain torch float64 reference of the decode-step attention (csrc/decode.hip kinds 1 and 2, csrc/attention.hip attn_decode_kernel).
No project code; importable without a GPU.

    [LayerNorm ->] projection x W^T + b -> q *= q_scale -> attention of ONE query per row over that row's keys / values

Inputs are what the kernels are given: bf16 activations and caches, fp32 parameters.  Caches are [rows, Tmax, H*64] VIEWS (a cache with a
wider row stride -- the engine's ldc = layers * 2 * d with a per-layer offset -- is passed as a slice of the wide tensor).

Contract, shared by all three kernels: a row whose keys are ALL masked gets zeros (the kernels' 1 / sum is replaced by 0).

  exact(...)           every operation in float64, nothing rounded in between
  rounding_model(...)  the same computation with the kernels' storage roundings and nothing else: LayerNorm output, q (after scaling), new
                       k / v and the output go through bf16.  weights="fp32": softmax weights unrounded (the vector kernels keep fp32);
                       weights="hi_lo": e = exp(s - max) enters the value product as bf16(e) + bf16(e - bf16(e)) (the KVLDS form's two
                       bf16 matrices, 16 significant bits) while the normaliser sums the unrounded e, as that kernel does
  reorder_by_copy(...) the semantics the history index replaces (HF _reorder_cache): gather the cache rows by beam_idx
"""
import torch

HD = 64


def bf16_round(x):
    return x.float().to(torch.bfloat16).double()


def ulp_bf16(x):
    """spacing of bf16 numbers at |x| (8 significant bits), float64; the smallest normal's spacing below it"""
    _, e = torch.frexp(x.double().abs().clamp_min(2.0 ** -126))     # |x| = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), e - 8)


def layer_norm(z, gamma, beta, eps):
    z = z.double()
    mu = z.mean(-1, keepdim=True)
    var = ((z - mu) ** 2).mean(-1, keepdim=True)
    return (z - mu) / torch.sqrt(var + eps) * gamma.double() + beta.double()


def gather_history(cache, hist, Tc):
    """[R, Tc, d]: position t of row r is cache[hist[r, t], t] (hist None: the row's own cache row)"""
    R = cache.shape[0] if hist is None else hist.shape[0]
    if Tc == 0:
        return cache.new_zeros((R, 0, cache.shape[2])).double()
    t = torch.arange(Tc, device=cache.device)
    rows = torch.arange(R, device=cache.device)[:, None].expand(R, Tc) if hist is None else hist[:, :Tc].long()
    return cache[rows, t[None, :].expand(R, Tc)].double()


def attention(q, keys, vals, mask=None, weights="fp32"):
    """q [R, H*64] (already scaled), keys / vals [R, T, H*64], mask [R, T] (0 = masked) or None -> [R, H*64] float64"""
    R, T, d = keys.shape
    H = d // HD
    qh = q.double().view(R, H, HD)
    kh, vh = keys.double().view(R, T, H, HD), vals.double().view(R, T, H, HD)
    s = torch.einsum("rhe,rthe->rht", qh, kh)
    if mask is not None:
        s = s.masked_fill((mask == 0)[:, None, :], float("-inf"))
    mx = s.max(-1, keepdim=True).values
    dead = torch.isinf(mx) & (mx < 0)                       # every key masked
    e = torch.exp(s - torch.where(dead, torch.zeros_like(mx), mx))
    e = torch.where(dead, torch.zeros_like(e), e)
    l = e.sum(-1, keepdim=True)
    if weights == "hi_lo":
        hi = bf16_round(e)
        e = hi + bf16_round(e - hi)
    else:
        assert weights == "fp32", weights
    o = torch.einsum("rht,rthe->rhe", e, vh) / torch.where(dead, torch.ones_like(l), l)
    return o.reshape(R, d)


def _run(rnd, weights, z, W, bias, H, q_scale, gamma, beta, eps, Kc, Vc, Tk, hist, kv_row, key_mask, mask_row, k_new, v_new, self_attn):
    """rnd: the storage rounding (identity for exact).  W None: z holds the projected, scaled q rows (attn_decode_kernel) and k_new / v_new
    the new key / value rows (or None: plain attention over the cache)."""
    res = {}
    d = H * HD
    if W is not None:
        x = z.double()
        if gamma is not None:
            res["ln"] = layer_norm(z, gamma, beta, eps)
            x = rnd(res["ln"])
        y = x @ W.double().t() + bias.double()
        res["x"] = x                                       # what the projection consumed
        res["y"] = y                                       # ... and produced, before q_scale and any rounding
        q = rnd(y[:, :d] * q_scale)
        if self_attn:
            k_new, v_new = y[:, d:2 * d], y[:, 2 * d:]
    else:
        q = z.double()
    R = q.shape[0]
    if self_attn:
        has_new = k_new is not None
        Tc = Tk - 1 if has_new else Tk
        keys, vals = gather_history(Kc, hist, Tc)[:R], gather_history(Vc, hist, Tc)[:R]
        if has_new:
            res["k_new"], res["v_new"] = rnd(k_new.double()), rnd(v_new.double())
            keys = torch.cat([keys, res["k_new"][:, None]], 1)
            vals = torch.cat([vals, res["v_new"][:, None]], 1)
        mask = None
    else:
        crow = torch.arange(R, device=q.device) if kv_row is None else kv_row.long()
        keys, vals = Kc[crow, :Tk].double(), Vc[crow, :Tk].double()
        mask = None
        if key_mask is not None:
            mrow = crow if mask_row is None else mask_row.long()
            mask = key_mask[mrow, :Tk]
    res["q"] = q
    res["out"] = rnd(attention(q, keys, vals, mask, weights))
    return res


def exact(z, H, *, W=None, bias=None, q_scale=1.0, gamma=None, beta=None, eps=1e-5, Kc, Vc, Tk, hist=None, kv_row=None, key_mask=None,
          mask_row=None, k_new=None, v_new=None, self_attn):
    """dict: out [R, H*64]; with a projection also ln (LayerNorm given), x, y, q; self-attention with a new row also k_new / v_new, the rows
    to be appended at cache position Tk - 1.  Self-attention: key / value t < Tk - 1 of row r is cache[hist[r][t], t], key / value Tk - 1
    the row's new projection.  Cross-attention: keys / values of cache row kv_row[r], masked by key_mask[mask_row[r]] (default kv_row)."""
    return _run(lambda t: t, "fp32", z, W, bias, H, q_scale, gamma, beta, eps, Kc, Vc, Tk, hist, kv_row, key_mask, mask_row, k_new, v_new,
                self_attn)


def rounding_model(z, H, *, weights="fp32", W=None, bias=None, q_scale=1.0, gamma=None, beta=None, eps=1e-5, Kc, Vc, Tk, hist=None,
                   kv_row=None, key_mask=None, mask_row=None, k_new=None, v_new=None, self_attn):
    return _run(bf16_round, weights, z, W, bias, H, q_scale, gamma, beta, eps, Kc, Vc, Tk, hist, kv_row, key_mask, mask_row, k_new, v_new,
                self_attn)


def reorder_by_copy(Kc, Vc, beam_idx):
    """HF _reorder_cache: row r of the new caches is row beam_idx[r] of the old ones"""
    return Kc[beam_idx.long()].clone(), Vc[beam_idx.long()].clone()


def head_rel_err(got, ref, H):
    """[R, H]: norm-wise error of every (row, head) against the reference head's norm; an all-zero reference head (fully masked item) must
    be matched exactly -- its entry is 0 then and inf otherwise"""
    R = ref.shape[0]
    g, r = got.double().view(R, H, HD), ref.double().view(R, H, HD)
    num, den = (g - r).norm(dim=-1), r.norm(dim=-1)
    return torch.where(den > 0, num / den.clamp_min(1e-300), torch.where(num > 0, torch.full_like(num, float("inf")), torch.zeros_like(num)))
