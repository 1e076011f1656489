"""Several targets per input: what the query-streaming attention kernels and the grouped training step cost.

    timeout 900 python tools/grouped_targets_time.py [--out profiles/grouped_targets_time.txt]

1. Kernels.  kmb_op_attn_fwd / kmb_op_attn_bwd at the training step's cross-attention shape with G = 5 targets of T = 32 tokens per input
   (B = 204, H = 12, Tq = 160, Tk = 64, the cross layout: Q rows of width d, K | V rows of width 2 d, key mask with padding), with and without
   dropout: the query-streaming kernels (the product library) against the general kernels on the same inputs (the DIAGNOSTIC library with
   KMB_ATTN_QSTREAM=0: `python km-bart_amd/build.py --variant diag KMB_DIAG` first).  Each library runs in a child process of its own; the
   route kmb_debug_attn_route reports is printed with every line.  Time per launch over windows of 3000 back-to-back launches between one
   event pair (tools/cider_reward_time.py; 0.1 - 0.8 s per window, the first window of every setting dropped), achieved algorithmic bytes / s,
   the median shader clock held in the windows and the board power over them.
2. Step.  vcg_base, 204 inputs x G = 5 = 1020 targets: forward + backward + AdamW as bench.py times its step, `targets_per_input=5` against
   today's path on the same 1020 targets with the inputs replicated (unchanged code: the parent commit's step), alternating windows in one
   process on one card; both times, their ratio, the workspace bytes of each.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "km-bart_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

HD = 64


def med(v):
    v = sorted(x for x in v if x is not None)
    return v[len(v) // 2] if v else None


# ------------------------------------------------------------------------------------------------ 1. kernels (child process)
def kernels(args):
    import bench
    from kmbart import _lib
    from kmbart._lib import check
    from gpu_util import DEV, attn_bwd_fields, attn_struct, stream
    lib = _lib.load()
    B, H, Tq, Tk = args.B, 12, args.G * args.T, args.S
    d = H * HD
    g = torch.Generator().manual_seed(7)
    Q = (torch.randn(B * Tq, d, generator=g) * 0.7).to(torch.bfloat16).to(DEV)
    kv = (torch.randn(B * Tk, 2 * d, generator=g) * 0.7).to(torch.bfloat16).to(DEV)
    dO = torch.randn(B * Tq, d, generator=g).to(torch.bfloat16).to(DEV)
    mask = torch.ones((B, Tk), dtype=torch.int64)
    for b in range(B):
        mask[b, Tk - b % 24:] = 0
    mask = mask.to(DEV)
    O = torch.empty((B * Tq, d), dtype=torch.bfloat16, device=DEV)
    lse = torch.empty((B, H, Tq), dtype=torch.float32, device=DEV)
    dq = torch.empty((B * Tq, d), dtype=torch.bfloat16, device=DEV)
    dkv = torch.empty((B * Tk, 2 * d), dtype=torch.bfloat16, device=DEV)
    cs = torch.empty((B, 3 * d), dtype=torch.float32, device=DEV)
    probe = bench.ClockProbe(lib, torch.device(DEV))
    fwd_bytes = 2 * B * Tq * d * 2 + 2 * B * Tk * d * 2 + B * H * Tq * 4
    bwd_bytes = 3 * B * Tq * d * 2 + 4 * B * Tk * d * 2 + B * H * Tq * 4
    for p in (0.0, 0.1):
        a = attn_struct(Q, kv[:, :d], kv[:, d:], B, H, Tq, Tk, mask, False, O, lse)
        attn_bwd_fields(a, dO, dq, dkv[:, :d], dkv[:, d:], (cs[:, :d], cs[:, d:2 * d], cs[:, 2 * d:]), 0.125)
        if p > 0:
            thr = int(round(p * 65536))
            a.drop_thr16, a.drop_seed, a.drop_scale = thr, 0x1234abcd, 1.0 / (1.0 - thr / 65536.0)
        routes = (lib.kmb_debug_attn_route(C.byref(a), 0), lib.kmb_debug_attn_route(C.byref(a), 1))
        for name, op, nbytes, route in (("fwd", lib.kmb_op_attn_fwd, fwd_bytes, routes[0]), ("bwd", lib.kmb_op_attn_bwd, bwd_bytes, routes[1])):
            for _ in range(10):
                check(op(C.byref(a), stream()))
            torch.cuda.synchronize()
            times, clocks = [], []
            pw = None
            for w in range(args.windows + 1):   # the first window is dropped: clock and power settle in it
                if w == 1:
                    pw = bench.PowerProbe(torch.device(DEV))
                    pw.start()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                probe.stamp(0)
                e0.record()
                for _ in range(args.launches):
                    check(op(C.byref(a), stream()))
                e1.record()
                probe.stamp(1)
                e1.synchronize()
                if w == 0:
                    continue
                times.append(e0.elapsed_time(e1) * 1e3 / args.launches)
                clocks.append(probe.mhz())
            rep = pw.report()
            us = med(times)
            print("KERNEL " + json.dumps(dict(lib=args.tag, op=name, dropout=p, route=route, B=B, H=H, Tq=Tq, Tk=Tk, us=round(us, 2),
                                              us_windows=[round(t, 2) for t in sorted(times)], tb_per_s=round(nbytes / us / 1e6, 3),
                                              clock_mhz=med(clocks), power_w=rep["median_w"] if rep else None)), flush=True)


# ------------------------------------------------------------------------------------------------ 2. step
def step(args, out):
    import bench
    from kmbart import _lib
    from kmbart.data import PackedFeatures
    from kmbart.optim import AdamW
    from src.data.synthetic import make_batch
    from src.model import MultiModalBartConfig, MultiModalBartForConditionalGeneration
    dev = torch.device("cuda", 0)
    B, G = args.B, args.G
    model = MultiModalBartForConditionalGeneration(MultiModalBartConfig.from_dict(bench.VCG_BASE)).to(dev).train()
    opt = AdamW(model.parameters(), lr=1e-5)
    opt.allow_overlap(True)
    src = make_batch(B, seed=1)
    tgt = make_batch(B * G, seed=2, num_regions=0, enc_len=8)
    grouped = {k: src[k].to(dev) for k in ("input_ids", "attention_mask")}
    grouped.update({k: tgt[k].to(dev) for k in ("decoder_input_ids", "decoder_attention_mask", "labels")})
    grouped["image_features"] = PackedFeatures.from_list(src["image_features"], 2052).to(dev)
    rep = dict(grouped, input_ids=grouped["input_ids"].repeat_interleave(G, 0), attention_mask=grouped["attention_mask"].repeat_interleave(G, 0))
    rep["image_features"] = PackedFeatures.from_list([src["image_features"][i // G] for i in range(B * G)], 2052).to(dev)
    eng = model._engine
    S, T = src["input_ids"].shape[1], tgt["labels"].shape[1]
    nf = sum(int(f.shape[0]) for f in src["image_features"])
    ws = dict(grouped=int(eng.lib.kmb_workspace_bytes_grouped(eng.h, B, S, T, nf, G)), replicated=int(eng.lib.kmb_workspace_bytes(eng.h, B * G, S, T, nf * G)))
    probe = bench.ClockProbe(_lib.load(), dev)

    def window(which, n):
        torch.cuda.synchronize()
        probe.stamp(0)
        t0 = time.perf_counter()
        for _ in range(n):
            if which == "grouped":
                model.train_step_fwd_bwd(grouped, targets_per_input=G)
            else:
                model.train_step_fwd_bwd(rep)
            opt.step()
        probe.stamp(1)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3, probe.mhz()

    for which in ("replicated", "grouped"):
        window(which, args.warmup)
    res, power = {"grouped": [], "replicated": []}, {}
    for r in range(args.rounds):
        for which in ("replicated", "grouped"):
            pw = bench.PowerProbe(dev)
            pw.start()
            ms, mhz = window(which, args.steps)
            rp = pw.report()
            res[which].append(ms)
            power.setdefault(which, []).append(rp["median_w"] if rp else None)
            line = "STEP round %d %-10s %.3f ms/step  shader clock %s MHz  power %s W" % (r, which, ms, mhz, rp["median_w"] if rp else None)
            print(line, flush=True)
            out.append(line)
    g_ms, r_ms = med(res["grouped"]), med(res["replicated"])
    line = "STEP_SUMMARY " + json.dumps(dict(inputs=B, targets_per_input=G, targets=B * G, S=S, T=T, grouped_ms=round(g_ms, 3), replicated_ms=round(r_ms, 3),
                                             ratio=round(g_ms / r_ms, 4), workspace_bytes=ws, power_w={k: med(v) for k, v in power.items()}))
    print(line, flush=True)
    out.append(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=204)
    ap.add_argument("--G", type=int, default=5)
    ap.add_argument("--T", type=int, default=32)
    ap.add_argument("--S", type=int, default=64)
    ap.add_argument("--launches", type=int, default=3000, help="back-to-back launches of a timed window (0.1 - 0.8 s per window)")
    ap.add_argument("--windows", type=int, default=5, help="timed windows per kernel and setting, behind one that is dropped")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernels-child", dest="tag", default=None, help="internal: time the kernels with the library this process loads")
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grouped_targets_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("grouped_targets_time.py measures on an MI355X; there is no GPU here")
    if args.tag:
        return kernels(args)
    out = ["tools/grouped_targets_time.py: B = %d inputs, G = %d targets of T = %d per input, S = %d" % (args.B, args.G, args.T, args.S)]
    diag = os.path.join(ROOT, "km-bart_amd", "lib", "libkmbart_hip_diag.so")
    runs = [("product", {})]
    if os.path.exists(diag):
        runs.append(("diag_qstream_off", {"KMB_LIB_PATH": diag, "KMB_ATTN_QSTREAM": "0"}))
    else:
        out.append("(no diagnostic library at %s: the general kernels were not timed)" % diag)
    for tag, env in runs:   # one child at a time: each loads its own library
        cmd = [sys.executable, os.path.abspath(__file__), "--kernels-child", tag] + [x for k in ("B", "G", "T", "S", "launches", "windows")
                                                                                    for x in ("--" + k, str(getattr(args, k)))]
        r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, **env), timeout=420)
        if r.returncode != 0:
            sys.exit("kernel timing child %s failed (%d):\n%s" % (tag, r.returncode, r.stderr[-3000:]))
        for line in r.stdout.splitlines():
            if line.startswith("KERNEL "):
                print(line, flush=True)
                out.append(line)
    if not args.skip_step:
        step(args, out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
