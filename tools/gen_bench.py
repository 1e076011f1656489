"""Generation throughput (BASELINE.json config 5): vcg_base, beam search with num_beams=5, KV-cached decoder steps,
cross-attention K/V computed once per batch item.  Prints one JSON line.

    python tools/gen_bench.py [--batch 64] [--beams 5] [--max-length 20] [--reps 5]

--do-sample times sampled generation (batch x --num-gen rows): with --beams 1 the reference's nucleus sampling on the device
sampler (kmb_sample_step), with --beams N > 1 beam sampling on kmb_beam_sample_step; unless --no-host, the torch host loop
(model._device_sampling = False) is alternated with it in one process, each generate timed to a device synchronise; one JSON
line per path, the first row of each seeded output shared between them.  --host-sampling times the torch path alone.
--logprobs (with --beams 1) asks generate for return_logprobs=True: the sampler then also writes every token's log-probability.
--repetition-penalty / --no-repeat-ngram hand generate() its score processors: by default that selects the torch loops;
--device_processors (with --beams 1) sets model._device_processors, and the pipelined one-beam loops apply them on the device
(kmb_logits_process).
Each line carries the repetitions' own times ("rep_ms"): their spread is the noise a difference between two runs is read against.
"""
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
from src.data.synthetic import make_batch  # noqa: E402
from src.model import MultiModalBartConfig, MultiModalBartForConditionalGeneration  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--beams", type=int, default=5)
ap.add_argument("--max-length", type=int, default=20)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--do-sample", action="store_true")
ap.add_argument("--top-p", type=float, default=1.0)
ap.add_argument("--top-k", type=int, default=0)
ap.add_argument("--temperature", type=float, default=1.0)
ap.add_argument("--num-gen", type=int, default=1)
ap.add_argument("--host-sampling", action="store_true", help="time the torch sampling path only")
ap.add_argument("--no-host", action="store_true", help="time the device sampler only")
ap.add_argument("--logprobs", action="store_true", help="generate(return_logprobs=True): one-beam sampling with token log-probabilities")
ap.add_argument("--repetition-penalty", type=float, default=1.0, help="generate(repetition_penalty=...)")
ap.add_argument("--no-repeat-ngram", type=int, default=0, help="generate(no_repeat_ngram_size=...)")
ap.add_argument("--device_processors", "--device-processors", action="store_true",
                help="model._device_processors = True: one-beam generation applies the score processors on the device")
args = ap.parse_args()
proc = {}
if args.repetition_penalty != 1.0:
    proc["repetition_penalty"] = args.repetition_penalty
if args.no_repeat_ngram != 0:
    proc["no_repeat_ngram_size"] = args.no_repeat_ngram
dev = torch.device("cuda", 0)
torch.manual_seed(0)
model = MultiModalBartForConditionalGeneration(MultiModalBartConfig.from_dict(bench.VCG_BASE)).to(dev).eval()
b = make_batch(args.batch, seed=4321)
if args.device_processors:
    model._device_processors = True
ids, am = b["input_ids"].to(dev), b["attention_mask"].to(dev)
feats = [f.to(dev) for f in b["image_features"]]
if args.do_sample:
    kw = dict(num_beams=args.beams, do_sample=True, top_p=args.top_p, top_k=args.top_k, temperature=args.temperature,
              num_return_sequences=args.num_gen, max_length=args.max_length, **proc)
    if args.logprobs:
        kw["return_logprobs"] = True
    paths = ["host"] if args.host_sampling else (["device"] if args.no_host else ["device", "host"])
    tot = {p: 0.0 for p in paths}
    steps = {p: 0 for p in paths}
    rep_ms = {p: [] for p in paths}
    for rep in range(args.reps + 1):          # rep 0 warms both paths up
        for p in paths:
            model._device_sampling = p == "device"
            torch.manual_seed(rep)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = model.generate(input_ids=ids, image_features=feats, attention_mask=am, **kw)
            torch.cuda.synchronize()
            if args.logprobs:
                out = out[0]
            if rep:
                dt = time.perf_counter() - t0
                tot[p] += dt
                rep_ms[p].append(round(dt * 1e3, 2))
                steps[p] += out.shape[1] - 1
    for p in paths:
        dt = tot[p] / args.reps
        print(json.dumps({"metric": "sampled_generate_ms", "path": p, "value": round(dt * 1e3, 2), "unit": "ms/generate",
                          "ms_per_decode_step": round(tot[p] / max(steps[p], 1) * 1e3, 3),
                          "sequences_per_sec": round(args.batch * args.num_gen / dt, 1), "rep_ms": rep_ms[p],
                          "logprobs": bool(args.logprobs),
                          "config": {"workload": "vcg_base generate, sampling", "batch": args.batch, "num_gen": args.num_gen,
                                     "rows": args.batch * args.num_gen, "top_k": args.top_k, "top_p": args.top_p,
                                     "temperature": args.temperature, "max_length": args.max_length,
                                     "decoder_steps": steps[p] / args.reps, **proc,
                                     "device_processors": bool(args.device_processors)},
                          "dtype": "bf16", "data": "synthetic", "n_gpus": 1}))
    sys.exit(0)
kw = dict(num_beams=args.beams, num_return_sequences=1, max_length=args.max_length, early_stopping=True, **proc)
out = model.generate(input_ids=ids, image_features=feats, attention_mask=am, **kw)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(args.reps):
    out = model.generate(input_ids=ids, image_features=feats, attention_mask=am, **kw)
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / args.reps
steps = out.shape[1] - 1
print(json.dumps({"metric": "generate_sequences_per_sec", "value": round(args.batch / dt, 1), "unit": "sequences/s",
                  "decoder_steps_per_sec": round(steps / dt, 1), "ms_per_generate": round(dt * 1e3, 2),
                  "config": {"workload": "vcg_base generate, beam search", "batch": args.batch, "num_beams": args.beams,
                             "max_length": args.max_length, "decoder_steps": steps, **proc,
                             "device_processors": bool(args.device_processors)}, "dtype": "bf16",
                  "data": "synthetic", "n_gpus": 1}))
