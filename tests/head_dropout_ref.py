"""One classification head under classif_dropout: float64 reference, the emulation of the engine's roundings, and the figures measured
between the two (a helper module of test_head_dropout_emulation_cpu.py and test_classif_dropout_ops_gpu.py; runs on whatever device its
inputs live on).

The head (HF 3.0.2 BartClassificationHead, reference src/model/model.py:133-158) is out_proj(m_h . tanh(dense(m_in . x))) with m_in [n, d_in]
and m_h [n, d] holding keep * scale or 0, scale = 1 / (1 - thr16 / 65536) computed in fp32 as kmb_handle::site_drop computes it.

* head_ref: float64 autograd of factor * loss(head(hdec[rows])) under GIVEN masks; the decoder-state gradient is the upstream one plus the head's.
* emu_head: the same float64 arithmetic with bf16 roundings where csrc/engine_train.cpp head_run rounds: the masked input hx, the unmasked
  tanh output hy, its masked copy hyd, the logits gradient, d_pre = m_h . (dlogits W_o) . (1 - hy^2), d_x = m_in . (d_pre W_d), and the
  decoder-state gradient after the fp32 scatter-add.

Two cases: "mrm" is loss_ref.HEAD (n = 203, d = 768, C = 1601, KL divergence); "rel" is relation-shaped (object | subject rows: d_in = 1536,
C = 129 padded to 136, cross-entropy).  EMU / EMU_WORST_ROW / EMU_LOSS are the emulation's errors against the reference under Bernoulli(0.1)
masks of a fixed generator (which mask is used does not matter for a rounding bound: the largest of four is recorded), rounded up;
test_head_dropout_emulation_cpu.py re-measures them and fails when one no longer holds or has grown slack.  The GPU test allows twice the
figure, for the loss too, under the masks the kernels drew (the project's margin for fp32 arithmetic and accumulation order, as
loss_ref.EMU_HEAD is used)."""
import torch

import loss_ref as R

P = 0.1
THR16 = 6554                                     # lrintf(0.1 * 65536)
SCALE = float(torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(1.0, dtype=torch.float32) - torch.tensor(float(THR16), dtype=torch.float32) / 65536.0))
MASK_SEED = 4711

REL = dict(n=203, d=768, din=1536, C=129, Cpad=136, rows_total=640, factor=0.5, seed=78)

MASK_SEEDS = tuple(range(MASK_SEED, MASK_SEED + 4))

# emulation against float64: relative norm of the whole tensor, the worst row of the decoder-state gradient, the loss (relative) -- each the LARGEST
# over the four masks of MASK_SEEDS (a single mask's figure moves by up to a third from mask to mask for the bias gradients and the loss, whose
# rounding errors partly cancel).  Measured: mrm 3.355e-3, 1.722e-3, 3.670e-3, 3.354e-3, 3.324e-3, worst row 4.829e-3, loss 2.72e-5;
# rel 3.411e-3, 1.627e-3, 4.176e-3, 3.568e-3, 4.442e-3, worst row 5.719e-3, loss 6.99e-5.
EMU = {
    "mrm": {"d_out_w": 3.4e-3, "d_out_b": 1.8e-3, "d_dense_w": 3.7e-3, "d_dense_b": 3.4e-3, "d_states": 3.4e-3},
    "rel": {"d_out_w": 3.5e-3, "d_out_b": 1.7e-3, "d_dense_w": 4.2e-3, "d_dense_b": 3.6e-3, "d_states": 4.5e-3},
}
EMU_WORST_ROW = {"mrm": 4.9e-3, "rel": 5.8e-3}
EMU_LOSS = {"mrm": 2.8e-5, "rel": 7.1e-5}        # hx, hy and hyd are rounded to bf16 before the logits: more than the plain head's 3.4e-6


def measure(name):
    """{quantity: the emulation's error against the float64 reference, largest over MASK_SEEDS} for case `name`; keys of EMU[name] plus
    worst_row and loss"""
    k = case(name)
    worst = {}
    for seed in MASK_SEEDS:
        m_in, m_h = bernoulli_masks(k, seed)
        ref, emu = head_ref(k, m_in, m_h), emu_head(k, m_in, m_h)
        got = {n: R.rel_norm(emu[n], ref[n]) for n in EMU[name]}
        got["worst_row"] = R.row_rel_norms(emu["d_states"], ref["d_states"])[0]
        got["loss"] = abs(float(emu["loss"] - ref["loss"])) / abs(float(ref["loss"]))
        for n, v in got.items():
            worst[n] = max(worst.get(n, 0.0), v)
    return worst


def case(name):
    """name -> dict(hdec, dhdec, rows: [idx] or [object idx, subject idx], Wd, bd, Wo, bo, tgt | labels, n, d, din, C, Cpad, rows_total, factor)"""
    if name == "mrm":
        k = R.head_case()
        k["rows"] = [k["rows"]]
        k.update(n=R.HEAD["n"], d=R.HEAD["d"], din=R.HEAD["d"], C=R.HEAD["C"], Cpad=R.HEAD["Cpad"], rows_total=R.HEAD["rows_total"],
                 factor=R.HEAD["factor"])
        return k
    c = REL
    g = torch.Generator(device="cpu").manual_seed(c["seed"])
    hdec = torch.randn(c["rows_total"], c["d"], generator=g).to(torch.bfloat16)
    dhdec = (torch.randn(c["rows_total"], c["d"], generator=g) * 1e-5).to(torch.bfloat16)
    obj = torch.randint(0, c["rows_total"], (c["n"],), generator=g).to(torch.int32)
    subj = torch.randint(0, c["rows_total"], (c["n"],), generator=g).to(torch.int32)
    obj[:6] = obj[6]                         # one state gathered seven times as an object ...
    subj[3] = obj[6]                         # ... and once as a subject
    Wd = (torch.randn(c["d"], c["din"], generator=g) * 0.03).to(torch.bfloat16)
    bd = torch.randn(c["d"], generator=g) * 0.02
    Wo = (torch.randn(c["C"], c["d"], generator=g) * 0.05).to(torch.bfloat16)
    bo = torch.randn(c["C"], generator=g) * 0.02
    labels = torch.randint(0, c["C"], (c["n"],), generator=g)
    labels[0], labels[1] = 0, c["C"] - 1
    out = dict(hdec=hdec, dhdec=dhdec, rows=[obj, subj], Wd=Wd, bd=bd, Wo=Wo, bo=bo, labels=labels)
    out.update({key: c[key] for key in ("n", "d", "din", "C", "Cpad", "rows_total", "factor")})
    return out


def bernoulli_masks(k, seed=MASK_SEED):
    """(m_in [n, din], m_h [n, d]) bool keep masks, P(drop) = 0.1, from a fixed CPU generator"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    m_in = torch.rand(k["n"], k["din"], generator=g) >= P
    m_h = torch.rand(k["n"], k["d"], generator=g) >= P
    return m_in, m_h


def _gather(hdec64, rows):
    return torch.cat([hdec64[r.long()] for r in rows], dim=1)


def _loss_and_grad(k, lg):
    """(loss, float64 gradient wrt the logits [n, C]) of factor * the head's loss on logits lg (any float type)"""
    n, C, f = k["n"], k["C"], k["factor"]
    if "tgt" in k:
        rows, g, _ = R.kl_ref(lg, k["tgt"], C, f)
        return f * rows.sum() / n, g
    rows, ok = R.ce_rows(lg, k["labels"], C)
    return f * rows.sum() / n, R.ce_grad(lg, k["labels"], C, f)


def head_ref(k, m_in, m_h):
    """float64 autograd of factor * loss(out_proj(m_h . tanh(dense(m_in . hdec[rows])))) on the same weights under the given keep masks"""
    import torch.nn.functional as F
    hdec = R.f64(k["hdec"]).requires_grad_(True)
    p = [R.f64(k[n]).requires_grad_(True) for n in ("Wd", "bd", "Wo", "bo")]
    x = _gather(hdec, k["rows"]) * (R.f64(m_in) * SCALE)
    y = torch.tanh(x @ p[0].t() + p[1]) * (R.f64(m_h) * SCALE)
    lg = y @ p[2].t() + p[3]
    if "tgt" in k:
        loss = k["factor"] * F.kl_div(torch.log_softmax(lg, dim=1), R.f64(k["tgt"]), reduction="batchmean")
    else:
        loss = k["factor"] * F.cross_entropy(lg, k["labels"])
    loss.backward()
    return dict(loss=loss.detach(), d_dense_w=p[0].grad, d_dense_b=p[1].grad, d_out_w=p[2].grad, d_out_b=p[3].grad,
                d_states=R.f64(k["dhdec"]) + hdec.grad, logits=lg.detach())


def emu_head(k, m_in, m_h):
    """head_run's roundings on float64 arithmetic: hx = bf16(m_in . x); hy = bf16(tanh); hyd = bf16(m_h . hy); logits fp32; dlogits = bf16;
    d_pre = bf16(m_h . (dlogits Wo)(1 - hy^2)); dx = bf16(m_in . (d_pre Wd)); scatter-add in fp32; states gradient = bf16(upstream + sum)"""
    d = k["d"]
    mi, mh = R.f64(m_in) * SCALE, R.f64(m_h) * SCALE
    hx = R.rb(_gather(R.f64(k["hdec"]), k["rows"]) * mi)
    hy = R.rb(torch.tanh(hx @ R.f64(k["Wd"]).t() + R.f64(k["bd"])))
    hyd = R.rb(hy * mh)
    lg = (hyd @ R.f64(k["Wo"]).t() + R.f64(k["bo"])).to(torch.float32)
    loss, g = _loss_and_grad(k, lg)
    g = R.rb(g)
    dpre = R.rb((g @ R.f64(k["Wo"])) * (1.0 - hy * hy) * mh)
    dx = R.rb((dpre @ R.f64(k["Wd"])) * mi)
    acc = torch.zeros_like(R.f64(k["hdec"]))
    for i, r in enumerate(k["rows"]):
        acc.index_add_(0, r.long(), dx[:, i * d:(i + 1) * d])
    return dict(loss=loss, d_out_w=g.t() @ hyd, d_out_b=g.sum(0), d_dense_w=dpre.t() @ hx, d_dense_b=dpre.sum(0),
                d_states=R.rb(R.f64(k["dhdec"]) + acc.to(torch.float32).to(torch.float64)))
