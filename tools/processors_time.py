"""Generation with score processors (one beam, or --num-beams N greedy beam search), timed as tools/gen_bench.py times it (its model and batch, one warm-up generate,
--reps timed ones, each to a device synchronise; "rep_ms" = their own times), on the built checkout named by --root: the parent
commit's tool has no processor flags, and tools/processors_ab.sh alternates parent / default / --device_processors processes with
it (profiles/processors_on_device_time.txt; with --num-beams and --device_beam_processors
profiles/beam_processors_on_device_time.txt, section 6n).  Prints one JSON line.

    python tools/processors_time.py --root . --repetition-penalty 1.2 --no-repeat-ngram 3 [--device_processors] [--do-sample ...]
    python tools/processors_time.py --root . --num-beams 5 --repetition-penalty 1.2 --no-repeat-ngram 3 [--device_beam_processors]
"""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", required=True)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--max-length", type=int, default=20)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--do-sample", action="store_true")
ap.add_argument("--top-p", type=float, default=1.0)
ap.add_argument("--top-k", type=int, default=0)
ap.add_argument("--num-gen", type=int, default=1)
ap.add_argument("--repetition-penalty", type=float, default=1.0)
ap.add_argument("--no-repeat-ngram", type=int, default=0)
ap.add_argument("--device_processors", action="store_true")
ap.add_argument("--num-beams", type=int, default=1)
ap.add_argument("--device_beam_processors", action="store_true")
ap.add_argument("--tag", default="")
args = ap.parse_args()
root = os.path.abspath(args.root)
sys.path.insert(0, os.path.join(root, "km-bart_amd"))
sys.path.insert(0, root)
import torch  # noqa: E402
import bench  # noqa: E402
from src.data.synthetic import make_batch  # noqa: E402
from src.model import MultiModalBartConfig, MultiModalBartForConditionalGeneration  # noqa: E402
import kmbart._lib as L  # noqa: E402
assert os.path.abspath(L.LIB_PATH).startswith(root), L.LIB_PATH

dev = torch.device("cuda", 0)
torch.manual_seed(0)
model = MultiModalBartForConditionalGeneration(MultiModalBartConfig.from_dict(bench.VCG_BASE)).to(dev).eval()
if args.device_processors:
    model._device_processors = True
if args.device_beam_processors:
    model._device_beam_processors = True
b = make_batch(args.batch, seed=4321)
ids, am = b["input_ids"].to(dev), b["attention_mask"].to(dev)
feats = [f.to(dev) for f in b["image_features"]]
proc = {}
if args.repetition_penalty != 1.0:
    proc["repetition_penalty"] = args.repetition_penalty
if args.no_repeat_ngram != 0:
    proc["no_repeat_ngram_size"] = args.no_repeat_ngram
if args.do_sample:
    kw = dict(num_beams=args.num_beams, do_sample=True, top_p=args.top_p, top_k=args.top_k, num_return_sequences=args.num_gen,
              max_length=args.max_length, **proc)
else:
    kw = dict(num_beams=args.num_beams, num_return_sequences=1, max_length=args.max_length, early_stopping=True, **proc)
rep_ms, steps = [], 0
for rep in range(args.reps + 1):
    torch.manual_seed(rep)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = model.generate(input_ids=ids, image_features=feats, attention_mask=am, **kw)
    torch.cuda.synchronize()
    if rep:
        rep_ms.append(round((time.perf_counter() - t0) * 1e3, 2))
        steps += out.shape[1] - 1
mean = sum(rep_ms) / len(rep_ms)
print(json.dumps({"tree": args.tag, "device_processors": bool(args.device_processors),
                  "device_beam_processors": bool(args.device_beam_processors), "metric": "generate_ms", "value": round(mean, 2), "unit": "ms/generate",
                  "ms_per_decode_step": round(sum(rep_ms) / max(steps, 1), 3), "rep_ms": rep_ms,
                  "config": dict(kw, batch=args.batch, rows=args.batch * args.num_gen * args.num_beams, decoder_steps=steps / args.reps)}))
