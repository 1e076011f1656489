"""What the clipped / guarded optimizer step costs: the training step's time (forward + backward + optimizer, no host synchronisation
inside the timed window) with max_grad_norm / skip_nonfinite OFF and ON, alternated in one process on one card, with the shader clock the
chip held in each window (kmb_clock_stamp).  ON adds one 4 B/param read of the gradient arena beside backward, one finish launch, and
moves the AdamW launches behind the last gradient (the norm needs all of them), so they no longer hide under backward.

    timeout 600 python tools/clip_step_time.py [--batch 1024] [--steps 20] [--warmup 6] [--rounds 3]

Prints one line per window and one JSON summary line (medians)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "km-bart_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import bench  # noqa: E402
from kmbart import _lib  # noqa: E402
from kmbart.data import PackedFeatures  # noqa: E402
from kmbart.optim import AdamW  # noqa: E402
from src.data.synthetic import make_batch  # noqa: E402
from src.model import MultiModalBartConfig, MultiModalBartForConditionalGeneration  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max_grad_norm", type=float, default=1.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("clip_step_time.py measures on an MI355X; there is no GPU here")
    dev = torch.device("cuda", 0)
    model = MultiModalBartForConditionalGeneration(MultiModalBartConfig.from_dict(bench.VCG_BASE)).to(dev).train()
    opts = {"off": AdamW(model.parameters(), lr=1e-5),
            "on": AdamW(model.parameters(), lr=1e-5, max_grad_norm=args.max_grad_norm, skip_nonfinite=True)}
    for o in opts.values():
        o.allow_overlap(True)
    b = make_batch(args.batch, seed=1)
    batch = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in b.items()}
    batch["image_features"] = PackedFeatures.from_list(b["image_features"], 2052).to(dev)
    probe = bench.ClockProbe(_lib.load(), dev)

    def window(opt, n):
        torch.cuda.synchronize()
        probe.stamp(0)
        t0 = time.perf_counter()
        for _ in range(n):
            model.train_step_fwd_bwd(batch)
            opt.step()
        probe.stamp(1)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3, probe.mhz()

    for name in ("off", "on"):
        window(opts[name], args.warmup)
    res = {"off": [], "on": []}
    for r in range(args.rounds):
        for name in ("off", "on"):
            ms, mhz = window(opts[name], args.steps)
            res[name].append((ms, mhz))
            print("round %d  %-3s  %.3f ms/step  shader clock %s MHz" % (r, name, ms, mhz), flush=True)
    st = opts["on"].step_state()

    def med(v):
        v = sorted(v)
        return v[len(v) // 2]

    out = {"batch": args.batch, "steps": args.steps, "rounds": args.rounds,
           "off_ms": round(med([m for m, _ in res["off"]]), 3), "on_ms": round(med([m for m, _ in res["on"]]), 3),
           "off_ms_all": [round(m, 3) for m, _ in res["off"]], "on_ms_all": [round(m, 3) for m, _ in res["on"]],
           "off_mhz": med([c for _, c in res["off"] if c] or [None]), "on_mhz": med([c for _, c in res["on"] if c] or [None]),
           "grad_norm": st["norm"], "coef": st["coef"], "applied_steps": st["steps"], "skipped": st["skipped"]}
    out["delta_ms"] = round(out["on_ms"] - out["off_ms"], 3)
    print("CLIP_STEP_TIME " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
