"""CPU: the bounds of test_gemm_epilogue_gpu.py have headroom, and its reference can see slips.

* For every small case of the matrix (tests/gemm_epi_ref.py: groups S, E = K edges, F = few rows; group P is the same code at 2048 x 4096) the
  fp32 emulation stays at or under 0.5 of each bound, measured on the fp32 values BEFORE any bf16 rounding; a bf16 output's total (rounding
  included) may reach 1.  The masks are seeded Bernoulli draws (the GPU module takes the kernels' own from kmb_op_dropout_mask).
* Every mutation of gemm_epi_ref.MUTATIONS, applied to the emulation alone, is rejected by assert_elementwise(limit = 1.0) on the fp32 form of
  its case and on the bf16 form too -- except those listed in BF16_BLIND (shown here to be tens of bounds out in fp32 and at most a rounding tie in bf16:
  why every class also runs with an fp32 output) and NO_BF16_FORM.  The polynomial-constant slip moves GeLU by at most 1.8e-5: the accumulator slack (K + 1) u mag is 6e-4 at K = 256
  and 4e-5 at K = 64, so only the K = 8 GeLU case (slack 7e-7) can see it, on the GPU as here.
* The constants the GPU module's bounds use are re-derived or range-checked."""
import math

import pytest
import torch

import gemm_epi_ref as G
import row_ref as R

HEADROOM = 0.5
SMALL = G.names("S") + G.names("E") + G.names("F")


def judge(c, emu, ex, what, fp32_limit=HEADROOM, forms=("f32", "bf16")):
    """every output of a case; the fp32 parts at fp32_limit, the bf16 totals at 1.0"""
    M = c["M"]
    if "f32" in forms:
        G.assert_elementwise(emu["v32"], ex["v"], ex["v_slack"], what + " v fp32 part", fp32_limit)
        if c["f32"]:
            G.assert_elementwise(emu["f32"], ex["f32"], ex["f32_slack"], what + " out_f32", fp32_limit)
        if "pre32" in emu:
            G.assert_elementwise(emu["pre32"], ex["pre"], ex["pre_slack"], what + " preact fp32 part", fp32_limit)
        if c["cs"]:
            ref, bound = G.colsum_bands(ex, M)
            G.assert_elementwise(G.fold_bands(emu["colsum"], M), ref, bound, what + " colsum bands", fp32_limit)
    if "bf16" in forms:
        if c["bf16"]:
            G.assert_elementwise(emu["v32"].to(torch.bfloat16), ex["v"], G.bf16_bound(ex["v"], ex["v_slack"]), what + " out_bf16 total")
        if "pre32" in emu:
            G.assert_elementwise(emu["pre32"].to(torch.bfloat16), ex["pre"], G.bf16_bound(ex["pre"], ex["pre_slack"]), what + " preact total")


@pytest.mark.parametrize("name", SMALL)
def test_emulation_stays_under_half_of_every_bound(name):
    c = G.case(name)
    keep = G.bernoulli_keep(c) if c["drop"] else None
    judge(c, G.emulate(c, keep), G.exact(c, keep), name)


def test_gelu_cases_reach_both_tails_and_the_underflow_region():
    for name in [n for n in G.names("S") if "gelu" in n]:
        c = G.case(name)
        a, b = G.logical(c)
        t = (G.f64(a) @ G.f64(b).t() + G.f64(c["bias_t"])).abs()
        n_small, n_mid, n_big = int((t < 0.5).sum()), int(((t > 2) & (t < 4)).sum()), int((t > 9).sum())
        print("%-28s |t| < 0.5: %d   2 .. 4: %d   > 9: %d" % (name, n_small, n_mid, n_big))
        assert n_small > 0 and n_mid > 0 and n_big > 0, name


# (mutation, case, K or None for the case's own)
MUTATION_CASES = [
    ("bias_after_scale", "S200x132_c03_scale20", 64),
    ("scale_n_plus1", "S200x132_c03_scale20", 64),
    ("scale_n_minus1", "S200x132_c03_scale20", 64),
    ("bias_shift_last8", "S200x132_c02_bias_ld4", 64),
    ("poly_const", "E200x132k8_c04_gelu_pre", None),
    ("no_tphi", "S200x132_c04_gelu_pre", 64),
    ("drop_after_res", "S200x132_c06_drop_res", 64),
    ("res_row_plus1", "S200x132_c07_res", 64),
    ("act4_linear", "S200x132_c17_kt_act4", 64),
    ("beta_ignored", "S200x132_c18_tt_beta1", 64),
    ("beta_ignored", "S200x132_c18_tt_betah", 64),
    ("colsum_skip_row", "S200x132_c12_kt_cs", 64),
    ("skip_kstep", "S200x132_c02_bias_ld4", None),
    ("pad_nan", "S200x132_c07_res", 64),
    ("pad_nan", "S200x132_c18_tt_beta0", 64),
]


def test_every_listed_mutation_has_a_case():
    assert sorted(set(m for m, _, _ in MUTATION_CASES)) == sorted(G.MUTATIONS)
    assert set(G.BF16_BLIND) | set(G.NO_BF16_FORM) <= set(G.MUTATIONS)


@pytest.mark.parametrize("mut,name,K", MUTATION_CASES)
def test_the_reference_sees_the_mutation(mut, name, K):
    c = G.case(name, K)
    keep = G.bernoulli_keep(c) if c["drop"] else None
    ex = G.exact(c, keep)
    judge(c, G.emulate(c, keep), ex, name + " unmutated", fp32_limit=1.0)       # the case itself passes
    emu = G.emulate(c, keep, mut)
    with pytest.raises(AssertionError):
        judge(c, emu, ex, "%s %s" % (name, mut), fp32_limit=1.0, forms=("f32",))
    has_bf16 = c["bf16"] or "pre32" in emu
    if mut in G.NO_BF16_FORM or not has_bf16:
        return
    if mut in G.BF16_BLIND:
        # below bf16 resolution: all the bf16 form shows is an element at a rounding tie tipped the other way, a percent over its bound,
        # where the fp32 form is tens of bounds out
        r32, _ = R.worst(emu["v32"], ex["v"], ex["v_slack"])
        r16, _ = R.worst(emu["v32"].to(torch.bfloat16), ex["v"], G.bf16_bound(ex["v"], ex["v_slack"]))
        print("%s %s: fp32 form %.1f bounds, bf16 form %.3f" % (name, mut, r32, r16))
        assert r32 > 10.0 and r16 < 1.05
    else:
        with pytest.raises(AssertionError):
            judge(c, emu, ex, "%s %s bf16" % (name, mut), forms=("bf16",))


def test_the_polynomial_slip_hides_under_the_accumulator_slack_of_a_long_reduction():
    """why the K = 8 GeLU case exists: at K = 64 the same slip passes even in fp32"""
    c = G.case("S200x132_c04_gelu_nopre", 64)
    judge(c, G.emulate(c, None, "poly_const"), G.exact(c), "poly_const at K = 64", fp32_limit=1.0, forms=("f32",))


def test_recorded_constants():
    x = torch.linspace(-12.0, 12.0, 240001, dtype=torch.float64)
    phi = torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    g1 = G.gelu_grad64(x)
    g2 = phi * (2.0 - x * x)
    g3 = phi * (x ** 3 - 4.0 * x)
    assert G.LIP1 - 0.01 < float(g1.abs().max()) <= G.LIP1
    assert G.LIP2 - 0.01 < float(g2.abs().max()) <= G.LIP2
    assert float(g2.abs().max()) / 2 <= 1.0 and float(g3.abs().max()) / 2 <= 1.0        # the s_t^2 terms
    assert float((1.0 - torch.tanh(x) ** 2).max()) <= G.LIP_TANH
    # Abramowitz-Stegun 7.1.26 with exact operations: 1.5e-7 on erf, half of that on Phi
    z = x.abs() / math.sqrt(2.0)
    t = 1.0 / (1.0 + 0.3275911 * z)
    poly = (((1.061405429 * t - 1.453152027) * t + 1.421413741) * t - 0.284496736) * t + 0.254829592
    erf_as = 1.0 - poly * t * torch.exp(-z * z)
    assert float((erf_as - torch.erf(z)).abs().max()) <= 1.5e-7
    assert G.AS_PHI == 0.75e-7
    # the pieces of the 24 u: poly >= 0.23, |t poly'(t) / poly(t)| <= 2.5 on (0, 1], |arg| 2^-|arg| <= 0.53
    tt = torch.linspace(1e-3, 1.0, 100001, dtype=torch.float64)
    pl = (((1.061405429 * tt - 1.453152027) * tt + 1.421413741) * tt - 0.284496736) * tt + 0.254829592
    dpl = ((4 * 1.061405429 * tt - 3 * 1.453152027) * tt + 2 * 1.421413741) * tt - 0.284496736
    assert float(pl.min()) >= 0.23 and float((tt * dpl / pl).abs().max()) <= 2.5
    hz = (((1.061405429 * tt - 1.453152027).abs() * tt ** 3 + ((1.061405429 * tt - 1.453152027) * tt + 1.421413741).abs() * tt ** 2
           + (pl - 0.254829592).abs() + pl) / pl)        # the four fmas' roundings, relative to poly
    assert float(hz.max()) <= 4.2
    ar = torch.linspace(0.0, 200.0, 200001, dtype=torch.float64)
    assert float((ar * torch.exp2(-ar)).max()) <= 0.5308
    assert 4 + 10 + 4.2 + 2 + 3 <= 24
    # tanhf: no accuracy table ships with the toolchain; 8 ulp is an assumption that nothing on a CPU can check
    assert G.TANH_ULP == 8
    # dropout's parameters as KmbDrop carries them
    thr, sc = G.drop_params(G.DROP_P)
    assert thr == 6554 and abs(sc - 1.0 / (1.0 - 6554 / 65536.0)) <= 2 * G.U * sc


def test_the_matrix_names_every_class():
    """21 classes at each of the three S shapes, the K edges under classes 2, 4, 10, 18, the few-row and persistent extras"""
    for M, N in G.S_SHAPES:
        got = G.names("S%dx%d_" % (M, N))
        assert sorted(set(n.split("_")[1] for n in got)) == ["c%02d" % k for k in range(1, 22)], got
    assert len(G.names("E")) == 4 * len(G.K_EDGES) and len(G.names("F")) == 5 * len(G.FEW_ROWS) + 1 + 2
    assert len(G.names("PW_")) == 9 and len(G.names("PE_")) == 5 and G.names("PG_") == ["PG_gelu_drop"]
