"""GPU: activation dropout at operator level -- KmbGemm act 1 with drop_thr16 != 0 stores keep ? GeLU(v) * scale : 0 and, in
preact, keep ? GeLU'(v) * scale : 0 (the derivative of what was stored), through kmb_op_gemm.

The launch variant is a per-process choice (KMB_GEMM_VARIANT), so every variant runs in a child process of its own: this file
behind KMB_GELU_DROP_CHILD.  The parent tests only start children, one at a time, each under its own timeout, and compare what
they report.  In every child, for every shape:

1. exactness without a tolerance: with p = 0.5 the threshold is 32768 and the scale exactly 2, so the dropped launch's out / pre
   must equal where(keep, 2 * plain, 0) of the same launch without dropout, keep = kmb_op_dropout_mask(seed, 0.5, M, N); doubling a
   bf16 is exact and the inputs are far from overflow.  The padding columns of the outputs stay untouched, the launch without the
   side output stores the same GeLU, and a relaunch into cleared outputs reproduces the bits.
2. against torch at p = 0.1: out against where(keep, gelu(base) * scale, 0), pre against where(keep, gelu'(base) * scale, 0) with
   gelu' from autograd, within tests/test_ops_gpu.py's F32_TOL / BF_TOL (the same quantities without the mask).
3. the backward contract: an act 2 launch with aux = the dropped pre equals (A B^T) * pre within F32_TOL.

Across children: every variant's out and pre of the p = 0.5 case have the bits of variant 7's.

Shapes (all pass kmb_gemm_check: K is a multiple of 8 in the forward layout, output rows are padded to a multiple of 8):
192 x 256 x 128 (the existing epilogue test's); 300 x 264 x 128 (edge rows, N a multiple of 8 but not of the tile); 77 x 100 x 72 (K % 64
!= 0: variant 1; N not a multiple of 8: four valid columns in the last group); 512 x 768 x 256 (the one shape here that variant 5
keeps); 2048 x 4096 x 384 (whole tiles: the four-wave persistent variants, 6 and 9 run it themselves; 8, 14 and 15 hand the class to 7); 4096 x 3072 x 768 (the fc1 launch at batch 64).
The kept fraction is asserted (0.5 +- 0.01) at every shape: the mask is a fixed function of seed 1234 and the shape (0.5022 on the
7700 elements of the smallest one, where 0.01 is 1.75 sigma of a fair mask).

Variant "0" is the unforced route: in one process every shape is launched first without dropout and then with it, so the two
whole-tile shapes reach the tuner twice -- the launch with dropout must be tuned on its own (the tuner's key separates the class)
among the variants that carry it, and the fp32-output launch of the same shape, which finds that cached choice, must leave a
persistent kernel's lean class for a variant that masks the derivative in its general path.  The activation-panel prefetch has no
switch in the product library (it is compiled into the diagnostic build only), so prefetch-off is not covered here."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(192, 256, 128), (300, 264, 128), (77, 100, 72), (512, 768, 256), (2048, 4096, 384), (4096, 3072, 768)]
SEED = 1234
# KMB_GEMM_VARIANT, then o1: per-XCD tile ranges (tile_order bit 0), s: shared-device mode (every tile of a persistent kernel from the
# counter).  (The activation-panel prefetch has no switch in the product library: it is on in every one of these runs.)
VARIANTS = ("7", "0", "8", "5", "11", "12", "13", "14", "15", "6", "9", "11o1", "14o1", "12s")
# the variant that must really have run the two whole-tile shapes (2048 x 4096 x 384 and 4096 x 3072 x 768): itself -- but 8, 14 and
# 15, which do not carry the class and fall back to 7 (csrc/gemm.hip gelu_drop_ok)
RUNS_ITSELF = ("7", "11", "12", "13", "6", "9")
FALLS_BACK_TO_7 = ("8", "14", "15", "14o1")


def _md5(t):
    return hashlib.md5(t.cpu().view(__import__("torch").uint8).numpy().tobytes()).hexdigest()


def child():
    import torch
    import torch.nn.functional as F
    sys.path[:0] = [ROOT, os.path.join(ROOT, "km-bart_amd"), os.path.join(ROOT, "tests")]
    from kmbart import _lib
    from kmbart._lib import KmbGemm, ptr
    from gpu_util import DEV, bf, dropout_mask, gemm, rel_err
    from test_ops_gpu import BF_TOL, F32_TOL
    lib = _lib.load()
    lib.kmb_gemm_shared_device(int(os.environ.get("KMB_GELU_DROP_SHARED", "0")))
    forced = int(os.environ.get("KMB_GEMM_VARIANT", "0"))
    report, fails = {}, []

    def check(ok, what):
        if not ok:
            fails.append(what)

    for si, (M, N, K) in enumerate(SHAPES):
        tag = "%dx%dx%d" % (M, N, K)
        g = torch.Generator(device="cpu").manual_seed(50 + si)
        A = bf((torch.randn(M, K, generator=g) * 0.5).to(DEV))
        # pre-activations of standard deviation ~1.5 at every K (|a| < 9): GeLU(a) and GeLU'(a) then stay in the NORMAL range of
        # bf16, where doubling is exact; from a ~ -13 on GeLU(a) is subnormal, and a rounded subnormal doubled is not the doubled one rounded
        B = bf((torch.randn(N, K, generator=g) * 0.2 * min(1.0, (128.0 / K) ** 0.5)).to(DEV))
        bias = torch.randn(N, generator=g).to(DEV)
        base = A.float() @ B.float().t() + bias
        Np = (N + 7) & ~7
        new = lambda dt: torch.zeros((M, Np), dtype=dt, device=DEV)
        kw = dict(N=N, bias=bias, act=1)
        # what runs it: the route of the launch as the library decides it for this process
        p = KmbGemm()
        p.A, p.B, p.lda, p.ldb, p.a_kc, p.b_kc, p.M, p.N, p.K = ptr(A), ptr(B), K, K, 1, 1, M, N, K
        p.bias, p.act, p.drop_thr16, p.drop_scale = ptr(bias), 1, 32768, 2.0
        o_, p_ = new(torch.bfloat16), new(torch.bfloat16)
        p.out_bf16, p.ld_out_bf16, p.preact, p.ld_preact = ptr(o_), Np, ptr(p_), Np
        p.tile_order = int(os.environ.get("KMB_TILE_ORDER", "0"), 0)
        route = (C.c_int32 * 128)()
        n = lib.kmb_debug_gemm_route(C.byref(p), forced, route, len(route))
        ran = int(route[2]) if n >= 4 and route[0] == 0 else -1
        timed = sorted({int(c) & 15 for c in route[1:n:3]}) if n >= 4 and route[0] == 1 else []   # unforced: the variants the tuner times for it

        # ---- 1. p = 0.5: exact
        out0, pre0, out1, pre1, out2 = (new(torch.bfloat16) for _ in range(5))
        gemm(A, B, preact=pre0, out_bf16=out0, **kw)
        gemm(A, B, preact=pre1, out_bf16=out1, drop_p=0.5, drop_seed=SEED, **kw)
        gemm(A, B, out_bf16=out2, drop_p=0.5, drop_seed=SEED, **kw)
        keep = dropout_mask(SEED, 0.5, M, N)
        zero = torch.zeros((), dtype=torch.bfloat16, device=DEV)
        check(torch.equal(out1[:, :N], torch.where(keep, (out0[:, :N].float() * 2).to(torch.bfloat16), zero)), tag + ": out != where(keep, 2 out, 0)")
        check(torch.equal(pre1[:, :N], torch.where(keep, (pre0[:, :N].float() * 2).to(torch.bfloat16), zero)), tag + ": pre != where(keep, 2 pre, 0)")
        check(bool((out1[:, N:] == 0).all()) and bool((pre1[:, N:] == 0).all()), tag + ": padding columns written")
        check(torch.equal(out1, out2), tag + ": the launch without preact stores another output")
        check(float(pre0.float().abs().max()) > 0.5 and float(out0.float().abs().max()) > 0.5, tag + ": degenerate inputs")
        check(float(base.abs().max()) < 10.0, tag + ": pre-activations outside the range the exactness argument covers")
        frac = float(keep.float().mean())
        check(abs(frac - 0.5) < 0.01, tag + ": kept fraction %.4f" % frac)
        h_out, h_pre = _md5(out1), _md5(pre1)
        out1.zero_(); pre1.zero_()
        gemm(A, B, preact=pre1, out_bf16=out1, drop_p=0.5, drop_seed=SEED, **kw)
        check((_md5(out1), _md5(pre1)) == (h_out, h_pre), tag + ": a relaunch differs")

        # ---- 2. p = 0.1 against torch
        thr = int(round(0.1 * 65536))
        scale = 1.0 / (1.0 - thr / 65536.0)
        keep1 = dropout_mask(SEED + 1, 0.1, M, N)
        bb = base.clone().requires_grad_(True)
        F.gelu(bb).sum().backward()
        z32 = torch.zeros((), device=DEV)
        ref_out = torch.where(keep1, F.gelu(base) * scale, z32)
        ref_pre = torch.where(keep1, bb.grad * scale, z32)
        outb, preb, out32, pre32 = new(torch.bfloat16), new(torch.bfloat16), new(torch.float32), new(torch.bfloat16)
        gemm(A, B, preact=preb, out_bf16=outb, drop_p=0.1, drop_seed=SEED + 1, **kw)
        gemm(A, B, preact=pre32, out_f32=out32, drop_p=0.1, drop_seed=SEED + 1, **kw)
        errs = dict(out_bf16=rel_err(outb[:, :N], ref_out), pre=rel_err(preb[:, :N], ref_pre), out_f32=rel_err(out32[:, :N], ref_out),
                    pre_f32launch=rel_err(pre32[:, :N], ref_pre))
        check(errs["out_bf16"] < BF_TOL and errs["pre"] < BF_TOL and errs["out_f32"] < F32_TOL and errs["pre_f32launch"] < BF_TOL,
              tag + ": against torch %s" % errs)
        check(torch.equal(preb, pre32), tag + ": pre differs between the bf16- and the fp32-output launch")

        # ---- 3. backward contract: act 2 on the dropped derivative
        dx = new(torch.float32)
        gemm(A, B, N=N, act=2, aux=preb, out_f32=dx)
        errs["act2"] = rel_err(dx[:, :N], (A.float() @ B.float().t()) * preb[:, :N].float())
        check(errs["act2"] < F32_TOL, tag + ": act 2 on the dropped derivative %.3e" % errs["act2"])
        torch.cuda.synchronize()
        report[tag] = dict(ran=ran, timed=timed, out=h_out, pre=h_pre, kept=frac, errs=errs)
    print("JSON" + json.dumps(dict(report=report, fails=fails)))


_results = {}


def run_child(v):
    if v not in _results:
        core = v.rstrip("s")
        env = dict(os.environ, KMB_GELU_DROP_CHILD="1", KMB_GEMM_VARIANT=core.split("o")[0],
                   KMB_TILE_ORDER=core.split("o")[1] if "o" in core else "0", KMB_GELU_DROP_SHARED="1" if v.endswith("s") else "0")
        r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("JSON")]
        assert r.returncode == 0 and line, (v, r.returncode, r.stdout[-2000:], r.stderr[-3000:])
        _results[v] = json.loads(line[0][4:])
    return _results[v]


@pytest.mark.parametrize("v", VARIANTS)
def test_gelu_dropout_masks_output_and_derivative(v):
    got = run_child(v)
    for tag, rec in got["report"].items():
        print(v, tag, "ran variant", rec["ran"], "kept %.4f" % rec["kept"], {k: "%.2e" % e for k, e in rec["errs"].items()})
    assert not got["fails"], got["fails"]
    ref = run_child("7")["report"]
    assert not run_child("7")["fails"]
    wrong = [tag for tag, rec in got["report"].items() if (rec["out"], rec["pre"]) != (ref[tag]["out"], ref[tag]["pre"])]
    assert not wrong, "bits differ from variant 7's: %s" % wrong
    if v in RUNS_ITSELF:
        for tag in ("2048x4096x384", "4096x3072x768"):
            if v == "13" and tag == "2048x4096x384":   # 4096 columns are no whole number of 192-column tiles
                continue
            assert got["report"][tag]["ran"] == int(v), (tag, got["report"][tag]["ran"])
    if v in FALLS_BACK_TO_7:
        for tag in ("2048x4096x384", "4096x3072x768"):
            assert got["report"][tag]["ran"] == 7, (tag, got["report"][tag]["ran"])
    if v == "0":
        for tag in ("2048x4096x384", "4096x3072x768"):
            timed = set(got["report"][tag]["timed"])
            assert timed and timed >= {7, 11, 12, 6, 9} and not timed & {8, 14, 15}, (tag, timed)
    if v == "5":
        assert got["report"]["512x768x256"]["ran"] == 5
    if v == "7":
        assert got["report"]["77x100x72"]["ran"] == 1   # K % 64 != 0: the register-staged kernel, whatever is forced


if __name__ == "__main__" and os.environ.get("KMB_GELU_DROP_CHILD"):
    child()
