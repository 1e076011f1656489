"""What gradient accumulation costs and saves per micro-step: bench.py's training step (vcg_base, dropout 0.1,
synthetic batch resident in HBM, overlapped AdamW) timed in windows as bench.py does, in ONE mode per process:

  --mode plain            forward + backward + optimizer step (what bench.py times)
  --mode accum --n N      groups of N micro-steps: zero_grad, N x (forward + backward at scale 1/N, folded), one optimizer step;
                          a "step" below is one MICRO-step

--root DIR takes the package and the library from another checkout of this repository (a build of the parent commit, for the
comparison `accumulation off == parent`); the plain mode uses nothing the parent lacks.  tools/grad_accum_ab.sh alternates the
processes.  Besides the wall time per step of each window, the device time from each micro-step's start to the next one's is taken
with events and reported by position in the group (the last position carries the optimizer)."""
import argparse
import json
import os
import sys
import time

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--mode", choices=("plain", "accum"), default="plain")
ap.add_argument("--n", type=int, default=4)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--steps", type=int, default=48, help="timed (micro-)steps, split over three windows; a multiple of 3 * n")
ap.add_argument("--warmup", type=int, default=12)
args = ap.parse_args()
root = os.path.abspath(args.root)
for p in (os.path.join(root, "km-bart_amd"), root):
    sys.path.insert(0, p)

import bench  # noqa: E402  (the checkout's own: workload constants and the clock / power probes)
from kmbart import _lib  # noqa: E402
from kmbart.data import PackedFeatures  # noqa: E402
from kmbart.optim import AdamW  # noqa: E402
from src.data.synthetic import make_batch  # noqa: E402
from src.model import MultiModalBartConfig, MultiModalBartForConditionalGeneration  # noqa: E402

n = args.n if args.mode == "accum" else 1
assert args.steps % (3 * n) == 0 and args.warmup % n == 0
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
torch.manual_seed(0)
model = MultiModalBartForConditionalGeneration(MultiModalBartConfig.from_dict(bench.VCG_BASE))
model.to(dev).train()
model._engine.set_seed(1234)
opt = AdamW(model.parameters(), lr=1e-5)
opt.allow_overlap(True)
b = make_batch(args.batch, enc_len=bench.S_ENC, dec_len=bench.T_DEC, num_regions=bench.REGIONS, seed=1234)
batch = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in b.items()}
batch["image_features"] = PackedFeatures.from_list(b["image_features"], 2052).to(dev)
if args.mode == "accum":
    model.accumulate_gradients(True)

stamps = []   # (position in the group, event at the micro-step's start)


def micro(i, record):
    pos = i % n
    if record:
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        stamps.append((pos, ev))
    if pos == 0:
        opt.zero_grad()
    model.train_step_fwd_bwd(batch, loss_scale=1.0 / n)
    if pos == n - 1:
        opt.step()


for i in range(args.warmup):
    micro(i, False)
probe = bench.ClockProbe(_lib.load(), dev)
power = bench.PowerProbe(dev)
power.start()
windows = []
per = args.steps // 3
for w in range(3):
    torch.cuda.synchronize()
    probe.stamp(0)
    t0 = time.perf_counter()
    for i in range(per):
        micro(i, True)
    ev = torch.cuda.Event(enable_timing=True)
    ev.record()
    stamps.append((-1, ev))
    probe.stamp(1)
    torch.cuda.synchronize()
    windows.append((round((time.perf_counter() - t0) / per * 1e3, 3), probe.mhz()))
by_pos = {}
for (pos, a), (_, z) in zip(stamps, stamps[1:]):
    if pos >= 0:
        by_pos.setdefault(pos, []).append(a.elapsed_time(z))
out = {"root": os.path.basename(root), "mode": args.mode, "n": n, "batch": args.batch,
       "ms_per_step_windows": [w[0] for w in windows], "clock_mhz_windows": [w[1] for w in windows],
       "device_ms_by_position": {str(k): round(sorted(v)[len(v) // 2], 3) for k, v in sorted(by_pos.items())},
       "board_power": power.report()}
print(json.dumps(out))
