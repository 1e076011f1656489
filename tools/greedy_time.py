"""Greedy generate(num_beams=1) on the device (kmb_gen_greedy_step) against the torch loop
(model._device_greedy = False, the code path before the device loop existed): wall time per generate() and per decode step
at 64 rows, max_length 20, vcg_base dimensions, random weights.

    python tools/greedy_time.py [--batch 64] [--max-length 20] [--reps 20] [--windows 3] [--out FILE]
    python tools/greedy_time.py --trace-path device --reps 3      # one path alone, for a kernel trace

Both paths alternate inside every timed window; a window's figure is the mean over its generates, the reported one the
median of the windows.  The time per decode step is (generate at max_length - generate at max_length 2) / (max_length - 2):
the encoder and the first step cancel.  The two paths must return the same ids."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "km-bart_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import bench  # noqa: E402
from src.data.synthetic import make_batch  # noqa: E402
from src.model import MultiModalBartConfig, MultiModalBartForConditionalGeneration  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--max-length", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20, help="generates per path, length and window")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--trace-path", choices=("device", "torch"), help="run only this path, --reps times, and print nothing else")
    ap.add_argument("--out", help="also write the report to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "greedy_time.py measures on the GPU"
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = MultiModalBartForConditionalGeneration(MultiModalBartConfig.from_dict(dict(bench.VCG_BASE, dropout=0.0))).to(dev).eval()
    b = make_batch(args.batch, seed=4321)
    kw = dict(input_ids=b["input_ids"].to(dev), image_features=[f.to(dev) for f in b["image_features"]],
              attention_mask=b["attention_mask"].to(dev), num_beams=1, eos_token_id=None)   # no EOS: every generate runs every step

    def run(path, max_length, n):
        model._device_greedy = path == "device"
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            out = model.generate(max_length=max_length, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n, out

    if args.trace_path:
        run(args.trace_path, args.max_length, 2)
        dt, out = run(args.trace_path, args.max_length, args.reps)
        print("%s path: %d generates of %d decode steps, %.3f ms each" % (args.trace_path, args.reps, out.shape[1] - 1, dt * 1e3))
        return
    paths, lengths = ("device", "torch"), (args.max_length, 2)
    outs = {p: run(p, args.max_length, 3)[1] for p in paths}      # warm-up of every shape, and the ids
    for p in paths:
        run(p, 2, 3)
    same = torch.equal(outs["device"], outs["torch"])
    wins = {(p, n): [] for p in paths for n in lengths}
    for _ in range(args.windows):
        for n in lengths:
            for p in paths:
                wins[(p, n)].append(run(p, n, args.reps)[0])
    med = {k: sorted(v)[len(v) // 2] for k, v in wins.items()}
    steps = args.max_length - 2
    lines = ["greedy generate(num_beams=1), %d rows, max_length %d, vcg_base, random weights, no EOS; %d windows x %d generates per "
             "path and length, paths alternated; median window (all windows in brackets)" % (args.batch, args.max_length, args.windows,
                                                                                              args.reps)]
    for p in paths:
        full, short = med[(p, args.max_length)], med[(p, 2)]
        lines.append("%-6s path: %.3f ms per generate [%s]; max_length 2: %.3f ms; %.1f us per decode step ((%.3f - %.3f) / %d)" % (
            p, full * 1e3, ", ".join("%.3f" % (w * 1e3) for w in wins[(p, args.max_length)]), short * 1e3,
            (full - short) / steps * 1e6, full * 1e3, short * 1e3, steps))
    d = (med[("device", args.max_length)] - med[("device", 2)]) / steps
    t = (med[("torch", args.max_length)] - med[("torch", 2)]) / steps
    lines.append("device / torch: %.3f per generate, %.3f per decode step (%.1f us shorter); ids identical: %s" % (
        med[("device", args.max_length)] / med[("torch", args.max_length)], d / t, (t - d) * 1e6, same))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    assert same, "the device path and the torch path chose different tokens"


if __name__ == "__main__":
    main()
