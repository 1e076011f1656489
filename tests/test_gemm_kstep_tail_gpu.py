"""GPU: the K-step tail of the pipelined 128x128 tile body (csrc/gemm.hip tile128: variant 7 with two LDS stages, variant 5 with four).

Both variants are one template, so comparing them with each other cannot see a slip in the shared K loop -- a tail rung that is
skipped or run twice, a wrong stage buffer, a wrong slice range.  What can: variant 1, the register-staged kernel, whose K loop is
independent and accumulates in the same order (all variants are bit-identical), and a float64 product.

The launch variant is a per-process choice (KMB_GEMM_VARIANT), so each of 1, 7 and 5 runs in a child process of its own: this file
behind KMB_KSTEP_TAIL_CHILD.  The parent tests only start children, one at a time, each under its own timeout, and compare what they
report.  Operands are 0.5 * randn rounded to bf16 from a seeded CPU generator (the same in every child), outputs fp32.

Cases: M x N = 256 x 256 (four whole tiles) and 200 x 136 (edge rows and columns), in the three operand layouts (both K-contiguous,
only A, both token-major with lda / ldb rounded up to 8), with
  * K / 64 = 1 .. 7 steps without split-K -- every rung of either tail ladder, its steady-state loop entered zero, one and more times;
  * split-K into raw slabs: K = 192 in 2 slices (1 and 2 steps), K = 448 in 3 (2, 2 and 3), K = 576 in 2 (4 and 5).
Variants 1 and 7 run all of them, variant 5 those with at least four steps per slice (what it is eligible for).

Asserted: every child's launches really ran the forced variant (kmb_debug_gemm_route: a fallback is an error, not a skip); variant 7's
bits equal variant 1's on every case and variant 5's equal variant 7's on every case variant 5 runs; and variant 7's result c
(a split launch's slabs summed in float64) against the float64 product c64 of the same bf16 operands, elementwise
  |c - c64| <= (K + 1) * 2^-24 * sum_k |a_k b_k|     (sum in float64)
-- the standard bound for an fp32 sum of K exactly representable products, and an upper bound for the slices' bounds added up."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((256, 256), (200, 136))
LAYOUTS = ((True, True), (True, False), (False, False))   # (a_kc, b_kc)
KSPLIT = [(64 * s, 0) for s in range(1, 8)] + [(192, 2), (448, 3), (576, 2)]   # (K, split_k)
VARIANTS = (1, 7, 5)


def min_steps(K, split):
    return K // 64 // max(split, 1)


def cases(variant):
    """[(name, M, N, K, a_kc, b_kc, split_k)]: the seed of a case is its position in variant 7's list"""
    out = []
    for M, N in SHAPES:
        for a_kc, b_kc in LAYOUTS:
            for K, split in KSPLIT:
                name = "%dx%dx%d_%s%s_split%d" % (M, N, K, "k" if a_kc else "t", "k" if b_kc else "t", split)
                out.append((name, M, N, K, a_kc, b_kc, split))
    return [(i, c) for i, c in enumerate(out) if variant != 5 or min_steps(c[3], c[6]) >= 4]


def child():
    import torch
    sys.path[:0] = [ROOT, os.path.join(ROOT, "km-bart_amd"), os.path.join(ROOT, "tests")]
    from kmbart import _lib
    from kmbart._lib import KmbGemm, ptr
    from gpu_util import DEV, bf, gemm
    lib = _lib.load()
    forced = int(os.environ["KMB_GEMM_VARIANT"])
    up8 = lambda v: (v + 7) & ~7
    report = {}
    for seed, (name, M, N, K, a_kc, b_kc, split) in cases(forced):
        g = torch.Generator(device="cpu").manual_seed(7000 + seed)
        A = bf(0.5 * torch.randn((M, K) if a_kc else (K, up8(M)), generator=g))
        B = bf(0.5 * torch.randn((N, K) if b_kc else (K, up8(N)), generator=g))
        Ad, Bd = A.to(DEV), B.to(DEV)
        out = torch.zeros((max(split, 1), M, N), dtype=torch.float32, device=DEV)
        kw = dict(a_kc=a_kc, b_kc=b_kc, M=M, N=N, K=K)
        kw.update(dict(split_k=split, slab=out) if split else dict(out_f32=out[0]))
        # what runs it: the route of this launch as the library decides it for this process
        p = KmbGemm()
        p.A, p.B, p.lda, p.ldb, p.a_kc, p.b_kc, p.M, p.N, p.K = ptr(Ad), ptr(Bd), Ad.stride(0), Bd.stride(0), int(a_kc), int(b_kc), M, N, K
        p.split_k = split
        if split:
            p.slab = ptr(out)
        else:
            p.out_f32, p.ld_out_f32 = ptr(out), N
        route = (C.c_int32 * 128)()
        n = lib.kmb_debug_gemm_route(C.byref(p), forced, route, len(route))
        rec = dict(ran=int(route[2]) if n >= 4 and route[0] == 0 else -1)
        gemm(Ad, Bd, **kw)
        torch.cuda.synchronize()
        c = out.cpu()
        rec["md5"] = hashlib.md5(c.numpy().tobytes()).hexdigest()
        if forced == 7:
            a64 = (A if a_kc else A[:, :M].t()).double()
            b64 = (B if b_kc else B[:, :N].t()).double()
            bound = (K + 1) * 2.0 ** -24 * (a64.abs() @ b64.abs().t())
            err = (c.double().sum(0) - a64 @ b64.t()).abs()
            rec["over"] = int((err > bound).sum())
            rec["worst"] = float((err / bound).max())
        report[name] = rec
    print("JSON" + json.dumps(report))


_results = {}


def run_child(v):
    if v not in _results:
        env = dict(os.environ, KMB_KSTEP_TAIL_CHILD="1", KMB_GEMM_VARIANT=str(v), KMB_TILE_ORDER="0")
        r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=120)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("JSON")]
        assert r.returncode == 0 and line, (v, r.returncode, r.stdout[-2000:], r.stderr[-3000:])
        _results[v] = json.loads(line[0][4:])
    return _results[v]


@pytest.mark.parametrize("v", VARIANTS)
def test_every_case_runs_the_forced_variant(v):
    got = run_child(v)
    assert sorted(got) == sorted(c[0] for _, c in cases(v))
    assert len(got) == (len(SHAPES) * len(LAYOUTS) * (5 if v == 5 else len(KSPLIT)))
    fell_back = {name: rec["ran"] for name, rec in got.items() if rec["ran"] != v}
    assert not fell_back, fell_back


def test_variant_7_has_the_bits_of_the_register_staged_kernel():
    v1, v7 = run_child(1), run_child(7)
    assert sorted(v1) == sorted(v7)
    wrong = [name for name in v7 if v7[name]["md5"] != v1[name]["md5"]]
    assert not wrong, wrong


def test_variant_5_has_the_bits_of_variant_7():
    v5, v7 = run_child(5), run_child(7)
    assert v5 and set(v5) <= set(v7)
    wrong = [name for name in v5 if v5[name]["md5"] != v7[name]["md5"]]
    assert not wrong, wrong


def test_variant_7_against_float64():
    v7 = run_child(7)
    for name, rec in sorted(v7.items()):
        print("%-28s worst |c - c64| / bound %.3f" % (name, rec["worst"]))
    over = {name: (rec["over"], rec["worst"]) for name, rec in v7.items() if rec["over"] or not rec["worst"] <= 1.0}
    assert not over, over


if __name__ == "__main__" and os.environ.get("KMB_KSTEP_TAIL_CHILD"):
    child()
