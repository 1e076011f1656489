"""CPU: the bounds of test_row_kernels_gpu.py have headroom.  At that module's shapes, seeds and edge rows, an fp32 emulation of each op
(torch fp32, strictly sequential sums: tests/row_ref.py) is held against the float64 reference in units of the same bounds.  The fp32
part of every bound must keep a factor 2 -- err / slack <= 0.5, measured on the fp32 values BEFORE any bf16 rounding; the total of a bf16
output (rounding included) may reach 1: round-to-nearest gives exactly 2^-8 at a binade edge.  The masks here are seeded Bernoulli draws
(the GPU module takes the kernels' own from kmb_op_dropout_mask); bit-exact statements (the slab reducers) have no fp32 part to measure.
The measured ratios are recorded in test_row_kernels_gpu.py's docstring; `pytest -s` prints them."""
import pytest
import torch

import row_ref as R

HEADROOM = 0.5
LN_FWD = [(M, D) for D in (8, 72, 512, 520, 768, 1024, 1032, 2048) for M in (1, 6)] + [(8197, 520), (8197, 1024)]


def _ln_fwd_ratios(ref, emu, what):
    R.assert_elementwise(emu["mean"], ref["mean"], ref["mean_bound"], what + " mean", HEADROOM)
    R.assert_elementwise(emu["rstd"], ref["rstd"], ref["rstd_bound"], what + " rstd", HEADROOM)
    R.assert_elementwise(emu["y32"], ref["y"], ref["y_slack"], what + " y fp32 part", HEADROOM)
    R.assert_elementwise(emu["y32"].to(torch.bfloat16), ref["y"], R.bf16_bound(ref["y"], ref["y_slack"]), what + " y total")


@pytest.mark.parametrize("M,D", LN_FWD)
def test_layernorm_forward_bounds_have_headroom(M, D):
    for kind in (("random", "const", "ramp") if M == 1 else ("mixed",)):
        c = R.ln_fwd_case(M, D, kind)
        emu = R.ln_fwd_emu(c["z"], c["gamma"], c["beta"])
        _ln_fwd_ratios(c["ref"], emu, "ln_fwd %dx%d %s" % (M, D, kind))
        for k, r in c["edges"].items():
            if k == "const":   # variance 0: rstd = eps^-1/2 and y = beta, whatever the order of the sums
                assert float(emu["mean"][r]) == R.CONST_ROW and torch.equal(emu["y32"][r], c["beta"])
                assert abs(float(c["ref"]["rstd"][r]) - R.EPS ** -0.5) <= 1e-9 * R.EPS ** -0.5


def test_one_pass_variance_on_the_large_mean_row():
    """what the large-mean row can and cannot see: a one-pass E[x^2] - mean^2 with sequential fp32 sums misses rstd's bound there from
    D = 768 on (measured 1.58, 1.63, 1.54 at D = 768, 1024, 2048); at the narrower widths the row's exact partial sums protect the
    one-pass form as well (0.08 at D = 8, 0.58 at D = 520), and the random rows have to catch it"""
    for D in (768, 1024, 2048):
        x = R.ramp_row(D)[None]
        ref = R.ln_fwd_ref(x, torch.ones(D), torch.zeros(D))
        mu = R.seq_sum(x, 1) / D
        rs = torch.rsqrt(R.seq_sum(x * x, 1) / D - mu * mu + R.EPS)
        r, _ = R.worst(rs, ref["rstd"], ref["rstd_bound"])
        print("one-pass variance, D = %d: rstd err / bound %.3g" % (D, r))
        assert r > 1.0, (D, r)


@pytest.mark.parametrize("M,D,form", R.LN_BWD_CASES)
def test_layernorm_backward_bounds_have_headroom(M, D, form):
    c = R.ln_bwd_inputs(M, D)
    d1, o2, d2 = R.form_flags(form)
    _, sc = R.drop_params(R.DROP_P)
    kw = dict(keep1=R.bernoulli_keep(M, D, R.SEED_DY) if d1 else None, scale1=sc, with_out2=o2,
              keep2=R.bernoulli_keep(M, D, R.SEED_OUT2) if d2 else None, scale2=sc)
    ref = R.ln_bwd_ref(c["dy"], c["z"], c["mean"], c["rstd"], c["gamma"], **kw)
    emu = R.ln_bwd_emu(c["dy"], c["z"], c["mean"], c["rstd"], c["gamma"], **kw)
    what = "ln_bwd %dx%d %s" % (M, D, form)
    R.assert_elementwise(emu["dz32"], ref["dz"], ref["dz_slack"], what + " dz fp32 part", HEADROOM)
    R.assert_elementwise(emu["dz32"].to(torch.bfloat16), ref["dz"], R.bf16_bound(ref["dz"], ref["dz_slack"]), what + " dz total")
    if o2:
        R.assert_elementwise(emu["out2_32"], ref["out2"], ref["out2_slack"], what + " out2 fp32 part", HEADROOM)
        R.assert_elementwise(emu["out2_32"].to(torch.bfloat16), ref["out2"], R.bf16_bound(ref["out2"], ref["out2_slack"]), what + " out2 total")
    for k in ("dgamma", "dbeta", "dsub"):
        R.assert_elementwise(emu[k], ref[k], ref[k + "_bound"], what + " " + k, HEADROOM)


@pytest.mark.parametrize("D", (72, 512, 520, 1024))
def test_slabs_layernorm_bounds_have_headroom(D):
    for nslabs in (1, 2, 5, 6):
        for with_bias in (False, True):
            c = R.ln_slabs_case(D, nslabs, with_bias)
            assert bool(torch.isfinite(c["pre"].float()).all())
            emu = R.ln_fwd_emu(c["pre"], c["gamma"], c["beta"])
            _ln_fwd_ratios(c["ref"], emu, "ln_fwd_slabs D=%d nslabs=%d bias=%d" % (D, nslabs, with_bias))


def test_column_sum_bounds_have_headroom():
    for M, N, ld in R.COLSUM_CASES:
        c = R.colsum_case(M, N, ld)
        R.assert_elementwise(R.seq_sum(c["X"][:, :N].float(), 0), c["ref"], c["bound"], "colsum %dx%d" % (M, N), HEADROOM)
    for B, S, D in R.POS_CASES:
        c = R.pos_case(B, S, D)
        R.assert_elementwise(R.seq_sum(c["dz"].float().view(B, S, D), 0), c["ref"], c["bound"], "pos_bwd %dx%dx%d" % (B, S, D), HEADROOM)


@pytest.mark.parametrize("D", (72, 520, 768, 2048))
def test_embedding_forward_bounds_have_headroom(D):
    _, sc = R.drop_params(R.DROP_P)
    for scaled in (False, True):
        c = R.embed_fwd_case(D, scaled)
        ref, emu = c["ref"], R.embed_fwd_emu(c)
        what = "embed_ln_fwd D=%d scale=%.4g" % (D, c["scale"])
        R.assert_elementwise(emu["z32"], ref["z"], ref["z_slack"], what + " z fp32 part", HEADROOM)
        R.assert_elementwise(emu["z32"].to(torch.bfloat16), ref["z"], R.bf16_bound(ref["z"], ref["z_slack"]), what + " z total")
        _ln_fwd_ratios(ref, emu, what)
        r = ref["y"] * sc
        R.assert_elementwise(emu["y32"] * torch.tensor(sc), r, ref["y_slack"] * sc + 2 * R.U * r.abs(), what + " dropped y fp32 part", HEADROOM)


@pytest.mark.parametrize("D", (72, 768))
def test_embedding_backward_bounds_have_headroom(D):
    for scaled in (False, True):
        c = R.embed_bwd_case(D, scaled)
        assert int(c["count"][R.EMBB_HOT]) == 40 and int(c["count"][R.EMBB_PAD]) == 0 and not bool(c["touched"][44:].any())
        what = "embed_bwd D=%d scale=%.4g" % (D, c["scale"])
        R.assert_elementwise(R.embed_bwd_emu(c), c["dE"], c["dE_bound"], what + " dE", HEADROOM)
        t32 = c["dz"].float()[c["sel"]] * torch.tensor(c["scale"])
        R.assert_elementwise(t32, c["dimg"], 2 * R.U * c["dimg"].abs(), what + " dimg fp32 part", HEADROOM)


def test_epilogue_reducer_dropout_slack_has_headroom():
    """kept elements of reduce_slabs_epi under dropout: fl(fl(w s) + res) or one fused multiply-add, against w s + res in float64"""
    _, sc = R.drop_params(R.DROP_P)
    c = R.epi_case(130, 768, 3)
    w = R.epi_pre_drop(c, True, 20)
    res = c["res"][:, :768].float()
    r = R.f64(w) * sc + R.f64(res)
    slack = 4 * R.U * ((R.f64(w) * sc).abs() + R.f64(res).abs())
    R.assert_elementwise(w * torch.tensor(sc) + res, r, slack, "reduce_slabs_epi kept value, two roundings", HEADROOM)
    R.assert_elementwise((R.f64(w) * sc + R.f64(res)).float(), r, slack, "reduce_slabs_epi kept value, fused", HEADROOM)
