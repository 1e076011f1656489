"""Scoring a given target sequence three ways, alternated in one process on vcg_base (b = 64 and b = 1024, 32 decoder rows):
  (a) model.score                      -- store-free head (per-block softmax statistics only)
  (b) the workaround without it        -- eval forward(use_cache=False) without labels (fp32 [B, T, V] logits), log_softmax + gather in torch
  (c) eval forward(labels=...)         -- the scalar loss (act 5: writes the bf16 exp matrix)
Every path runs `--warmup` untimed rounds, then `--windows` windows of `--iters` calls each between two events, the three paths
interleaved window by window so that clock drift hits them alike; reported: median and min .. max of the per-call window means, the
ratios a / c and b / a, and the shader clock the chip held over the run (kmb_clock_stamp).  One JSON line per batch size.

    python tools/score_bench.py [--batches 64,1024] [--windows 7] [--iters 10] [--warmup 3] [--only a,c]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "km-bart_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import bench  # noqa: E402
from kmbart import _lib  # noqa: E402
from src.data.synthetic import make_batch  # noqa: E402
from src.model import MultiModalBartConfig, MultiModalBartForConditionalGeneration  # noqa: E402

DEV = "cuda:0"


def clock_stamp():
    out = torch.zeros(16, dtype=torch.int64, device=DEV)
    _lib.check(_lib.load().kmb_clock_stamp(_lib.ptr(out), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,1024")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="a,b,c")
    args = ap.parse_args()
    only = args.only.split(",")
    model = MultiModalBartForConditionalGeneration(MultiModalBartConfig.from_dict(dict(bench.VCG_BASE, dropout=0.0)))
    model.to(DEV).eval()
    for bsz in [int(x) for x in args.batches.split(",")]:
        b = make_batch(bsz, seed=1234)
        d = {k: v.to(DEV) for k, v in b.items() if torch.is_tensor(v)}
        feats = [f.to(DEV) for f in b["image_features"]]
        kw = dict(input_ids=d["input_ids"], image_features=feats, attention_mask=d["attention_mask"],
                  decoder_input_ids=d["decoder_input_ids"], decoder_attention_mask=d["decoder_attention_mask"])
        lab = d["labels"]

        def path_a():
            return model.score(labels=lab, **kw).nll

        def path_b():
            logits = model(use_cache=False, **kw)[0]
            lp = torch.log_softmax(logits, -1).gather(-1, lab.clamp(min=0).unsqueeze(-1)).squeeze(-1)
            return -(lp * (lab >= 0)).sum(1)

        def path_c():
            return model(labels=lab, **kw)[0]

        paths = {k: f for k, f in (("a", path_a), ("b", path_b), ("c", path_c)) if k in only}
        times = {k: [] for k in paths}
        with torch.no_grad():
            for f in paths.values():
                for _ in range(args.warmup):
                    f()
            torch.cuda.synchronize()
            c0 = clock_stamp()
            for _ in range(args.windows):
                for k, f in paths.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.iters):
                        f()
                    e1.record()
                    e1.synchronize()
                    times[k].append(e0.elapsed_time(e1) / args.iters)
            c1 = clock_stamp()
            torch.cuda.synchronize()
        dt = (c1 - c0).cpu().view(8, 2).double()
        mhz = float((dt[:, 0] / dt[:, 1].clamp(min=1)).median() * 100.0)
        res = {"batch": bsz, "decoder_rows": int(lab.numel()), "score_path": getattr(model._engine, "last_score_path", None),
               "windows": args.windows, "iters": args.iters, "clock_mhz": round(mhz, 1)}
        for k, v in times.items():
            res[k + "_ms"] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
        if "a" in times and "c" in times:
            res["a_over_c"] = round(statistics.median(times["a"]) / statistics.median(times["c"]), 4)
            res["c_spread"] = round((max(times["c"]) - min(times["c"])) / statistics.median(times["c"]), 4)
        if "a" in times and "b" in times:
            res["b_over_a"] = round(statistics.median(times["b"]) / statistics.median(times["a"]), 3)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
