"""What label smoothing costs: the training step's time (forward + backward + optimizer, no host synchronisation inside the timed window)
with label_smoothing 0 and eps, alternated in one process on one card, with the shader clock the chip held in each window
(kmb_clock_stamp) and the board power over all windows of a setting (hwmon PPT).  bench.py's vcg_base step on make_batch.

eps > 0 adds, in the fused head: one read of the tied matrix's bf16 mirror (2 V d bytes) for wsum | bsum and its finishing launch, a
finishing launch for u, and a few d-wide operands in row kernels that run anyway (csrc/loss.hip "Label smoothing as rank-one terms").

    timeout 600 python tools/label_smoothing_time.py [--batch 64 1024] [--eps 0.1] [--steps 20] [--warmup 6] [--rounds 3]

Prints one line per window and one JSON summary line per batch (medians)."""
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


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def run(model, opt, dev, bsz, eps, steps, warmup, rounds):
    b = make_batch(bsz, seed=1)
    batch = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in b.items()}
    batch["image_features"] = PackedFeatures.from_list(b["image_features"], 2052).to(dev)
    probe = bench.ClockProbe(_lib.load(), dev)

    def window(e, n):
        model.label_smoothing = e
        torch.cuda.synchronize()
        probe.stamp(0)
        t0 = time.perf_counter()
        for _ in range(n):
            model.train_step_fwd_bwd(batch)
            opt.step()
        probe.stamp(1)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3, probe.mhz()

    settings = (("off", 0.0), ("on", eps))
    for _, e in settings:
        window(e, warmup)
    res = {"off": [], "on": []}
    power = {}
    for r in range(rounds):
        for name, e in settings:
            pw = bench.PowerProbe(dev)
            pw.start()
            ms, mhz = window(e, steps)
            rep = pw.report()
            res[name].append((ms, mhz))
            if rep:
                power.setdefault(name, []).append(rep["median_w"])
            print("b=%d round %d  %-3s (eps %.2f)  %.3f ms/step  shader clock %s MHz  power %s W  head form %d"
                  % (bsz, r, name, e, ms, mhz, rep["median_w"] if rep else None, model._engine.last_head_form()), flush=True)
    out = {"batch": bsz, "eps": eps, "steps": steps, "rounds": rounds,
           "off_ms": round(med([m for m, _ in res["off"]]), 3), "on_ms": round(med([m for m, _ in res["on"]]), 3),
           "off_ms_all": [round(m, 3) for m, _ in res["off"]], "on_ms_all": [round(m, 3) for m, _ in res["on"]],
           "off_mhz": med([c for _, c in res["off"] if c] or [None]), "on_mhz": med([c for _, c in res["on"] if c] or [None]),
           "off_power_w": med(power.get("off") or [None]), "on_power_w": med(power.get("on") or [None])}
    out["delta_ms"] = round(out["on_ms"] - out["off_ms"], 3)
    out["delta_pct"] = round(100.0 * out["delta_ms"] / out["off_ms"], 2)
    print("LABEL_SMOOTHING_TIME " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--eps", type=float, default=0.1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("label_smoothing_time.py measures on an MI355X; there is no GPU here")
    dev = torch.device("cuda", 0)
    model = MultiModalBartForConditionalGeneration(MultiModalBartConfig.from_dict(bench.VCG_BASE)).to(dev).train()
    opt = AdamW(model.parameters(), lr=1e-5)
    opt.allow_overlap(True)
    for bsz in args.batch:
        run(model, opt, dev, bsz, args.eps, args.steps, args.warmup, args.rounds)


if __name__ == "__main__":
    main()
