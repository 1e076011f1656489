"""What attention dropout costs: attention forward and backward at the three training shapes (encoder self 64 x 64, decoder self
32 x 32 causal -- two heads per tile --, cross 32 x 64; B from the environment, default 1024: the benchmark batch), p = 0 against
p = 0.1 (P from the environment) in the same process on the product library.  The two settings alternate in rounds of 20 launches;
the median round of each is printed."""
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "km-bart_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
from gpu_util import DEV, attn_struct, stream  # noqa: E402
from kmbart import _lib  # noqa: E402
from kmbart._lib import check, ptr  # noqa: E402

lib = _lib.load()
B, H, d = int(os.environ.get("B", "1024")), 12, 768
P = float(os.environ.get("P", "0.1"))
THR = min(int(round(P * 65536)), 65535)
ROUNDS, REPS = 7, 20


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / REPS


for name, Tq, Tk, causal in (("enc self", 64, 64, 0), ("dec self", 32, 32, 1), ("cross", 32, 64, 0)):
    g = torch.Generator(device=DEV).manual_seed(1)
    qkv = (torch.randn(B * Tq, 3 * d, device=DEV, generator=g) * 0.5).bfloat16()
    kv = (torch.randn(B * Tk, 3 * d, device=DEV, generator=g) * 0.5).bfloat16() if Tk != Tq else qkv
    O = torch.empty(B * Tq, d, dtype=torch.bfloat16, device=DEV)
    lse = torch.empty(B * H * Tq, dtype=torch.float32, device=DEV)
    mask = torch.ones(B, Tk, dtype=torch.int64, device=DEV)   # the training step always passes a padding mask
    dO = (torch.randn(B * Tq, d, device=DEV, generator=g) * 0.1).bfloat16()
    dqkv = torch.empty(B * Tq, 3 * d, dtype=torch.bfloat16, device=DEV)
    dkv = torch.empty(B * Tk, 3 * d, dtype=torch.bfloat16, device=DEV) if Tk != Tq else dqkv
    cs = torch.empty(B, 3 * d, dtype=torch.float32, device=DEV)
    structs = []
    for thr in (0, THR):
        a = attn_struct(qkv[:, :d], kv[:, d:2 * d], kv[:, 2 * d:], B, H, Tq, Tk, mask, causal, O, lse)
        a.dO, a.lddo = ptr(dO), d
        a.dQ, a.dK, a.dV = ptr(dqkv[:, :d]), ptr(dkv[:, d:2 * d]), ptr(dkv[:, 2 * d:])
        a.lddq, a.lddk, a.lddv = 3 * d, 3 * d, 3 * d
        a.dq_scale = 0.125
        a.dq_colsum, a.dk_colsum, a.dv_colsum, a.ld_colsum = ptr(cs[:, :d]), ptr(cs[:, d:2 * d]), ptr(cs[:, 2 * d:]), 3 * d
        if thr:
            a.drop_thr16, a.drop_seed, a.drop_scale = thr, 12345, 1.0 / (1.0 - thr / 65536.0)
        structs.append(a)
    for what, op in (("fwd", lib.kmb_op_attn_fwd), ("bwd", lib.kmb_op_attn_bwd)):
        for a in structs:   # warm-up (the forward also leaves the log-sum-exps the backward reads)
            for _ in range(3):
                check(op(C.byref(a), stream()))
        t = ([], [])
        for _ in range(ROUNDS):
            for i, a in enumerate(structs):
                t[i].append(timed(lambda: check(op(C.byref(a), stream()))))
        t0, t1 = statistics.median(t[0]), statistics.median(t[1])
        print(f"{name:9s} {what} B={B} Tq={Tq} Tk={Tk}: p=0 {t0:7.1f} us   p={P} {t1:7.1f} us   +{(t1 / t0 - 1) * 100:5.1f} %"
              f"   (rounds: {min(t[0]):.1f}-{max(t[0]):.1f} / {min(t[1]):.1f}-{max(t[1]):.1f})")
