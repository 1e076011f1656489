"""What activation dropout costs the fc1 forward launch (bias + GeLU + stored GeLU', bf16 output) at the benchmark's two shapes,
65536 x 3072 x 768 (encoder rows of b = 1024) and 32768 x 3072 x 768 (decoder rows): p = 0 against p = 0.1 (P from the environment)
alternating in one process in rounds of 20 launches, the median round of each, per launch variant the tuner may pick for the shape.
The variant is a per-process choice (KMB_GEMM_VARIANT), so the tool re-runs itself once per variant, one child at a time.

    python tools/gelu_dropout_time.py > profiles/gelu_dropout_time.txt
"""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "km-bart_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = ((65536, 3072, 768), (32768, 3072, 768))
# the tuner's candidates for these shapes with dropout (kmb_debug_gemm_route) -- the variants that carry the class -- then 8, 14, 15,
# which do not: for them only the launch without dropout is timed (what the shape runs on when activation_dropout = 0)
VARIANTS = (7, 11, 12, 13, 9, 6, 8, 14, 15)
NO_CLASS = (8, 14, 15)
P = float(os.environ.get("P", "0.1"))
ROUNDS, REPS = 7, 20


def child():
    import torch
    from gpu_util import DEV, bf, gemm

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / REPS

    v = os.environ["KMB_GEMM_VARIANT"]
    for M, N, K in SHAPES:
        g = torch.Generator(device=DEV).manual_seed(1)
        A = bf(torch.randn(M, K, device=DEV, generator=g) * 0.5)
        B = bf(torch.randn(N, K, device=DEV, generator=g) * 0.05)
        bias = torch.randn(N, device=DEV, generator=g) * 0.1
        out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
        pre = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
        runs = [lambda p=p: gemm(A, B, bias=bias, act=1, preact=pre, out_bf16=out, drop_p=p, drop_seed=12345, tile_order=1)
                for p in ((0.0,) if int(v) in NO_CLASS else (0.0, P))]
        for fn in runs:
            for _ in range(3):
                fn()
        t = ([], [])
        for _ in range(ROUNDS):
            for i, fn in enumerate(runs):
                t[i].append(timed(fn))
        if len(runs) == 1:
            print(f"v{v:>2s} {M} x {N} x {K}: p=0 {statistics.median(t[0]):7.1f} us   (does not carry the class; rounds: {min(t[0]):.1f}-{max(t[0]):.1f})",
                  flush=True)
            del A, B, out, pre
            continue
        t0, t1 = statistics.median(t[0]), statistics.median(t[1])
        print(f"v{v:>2s} {M} x {N} x {K}: p=0 {t0:7.1f} us   p={P} {t1:7.1f} us   +{(t1 / t0 - 1) * 100:5.1f} %"
              f"   (rounds: {min(t[0]):.1f}-{max(t[0]):.1f} / {min(t[1]):.1f}-{max(t[1]):.1f})", flush=True)
        del A, B, out, pre


def main():
    if os.environ.get("KMB_GELU_DROP_TIME_CHILD"):
        return child()
    for v in VARIANTS:
        env = dict(os.environ, KMB_GELU_DROP_TIME_CHILD="1", KMB_GEMM_VARIANT=str(v))
        r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:
            print("variant", v, "failed:\n", r.stderr[-3000:])
            sys.exit(1)


if __name__ == "__main__":
    main()
