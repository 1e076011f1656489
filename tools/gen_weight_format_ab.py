"""A/B of the decoder weight formats (model.set_decoder_weight_format: "bf16" | "fp8_e4m3") at the benchmark's generation setting:
vcg_base, batch 64, beam search with 5 beams and max_length 20, and the greedy leg (64 rows).  DESIGN.md section 6u.

    python tools/gen_weight_format_ab.py [--windows 7] [--reps 20] [--no-quality] [--out profiles/fp8_decoder_weights.md]

One process, the two formats alternated window by window (a window = --reps generates up to a device synchronise) after two
warm-up generates per format and leg; the MEDIAN window per format is the result, its spread the noise.  Beside each number: the
shader clock and board power sampled from hwmon (read only) while that format's windows ran.  bf16 is the parent commit's code path
(the format switch selects other kernel instances, nothing else), so "FP8 against bf16 in this run" is the comparison that counts.

Per block kind: the six fused blocks of one decoder layer at 320 rows (and at 64) through kmb_op_decode_block on random weights,
2000 launches per window between device events, formats alternated.

Quality (REPORTED, not asserted; --no-quality skips it): on the full-size golden model (oracle.goldenlib weights re-scaled as
tests/test_decode_fused_gpu.py does, so that searches move) the relative error of the FP8 decode's teacher-forced logits against
the bf16 decode's, the share of identical beam-5 rows and the largest length-normalised score gap.  Random-init logits are
near-ties: row agreement there measures rounding, not quality; a checkpoint-quality statement needs trained weights."""
import argparse
import ctypes as C
import glob
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "km-bart_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import bench  # noqa: E402
from kmbart import _lib  # noqa: E402
from kmbart._lib import KmbDecodeBlock, check, ptr  # noqa: E402
from src.data.synthetic import make_batch  # noqa: E402
from src.model import MultiModalBartConfig, MultiModalBartForConditionalGeneration  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=7)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--no-quality", action="store_true")
ap.add_argument("--out", default=None, help="also write the report to this file")
args = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU: there is nothing to fall back to"
dev = torch.device("cuda", 0)
FORMATS = ("bf16", "fp8_e4m3")
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


class Hwmon:
    """shader clock (MHz) and board power (W) of device 0, sampled every 5 ms while `on`"""

    def __init__(self):
        p = torch.cuda.get_device_properties(0)
        bus = "%04x:%02x:%02x" % (getattr(p, "pci_domain_id", 0), p.pci_bus_id, p.pci_device_id)
        card = [c for c in glob.glob("/sys/class/drm/card*/device") if bus in os.path.realpath(c)]
        self.pw = glob.glob(card[0] + "/hwmon/hwmon*/power1_input") if card else []
        self.fq = glob.glob(card[0] + "/hwmon/hwmon*/freq1_input") if card else []
        self.samples = {}
        self.key = None
        self.stop = False
        self.t = threading.Thread(target=self.run, daemon=True)
        self.t.start()

    def run(self):
        while not self.stop:
            k = self.key
            if k is not None and self.pw and self.fq:
                try:
                    self.samples.setdefault(k, []).append((int(open(self.fq[0]).read()) / 1e6, int(open(self.pw[0]).read()) / 1e6))
                except Exception:
                    pass
            time.sleep(0.005)

    def text(self, k):
        s = self.samples.get(k)
        if not s:
            return "clock / power: not readable on this machine"
        return "clock median %.0f MHz, power median %.0f W (%d samples)" % (statistics.median(x[0] for x in s),
                                                                             statistics.median(x[1] for x in s), len(s))


hw = Hwmon()


def spread(v):
    return "median %.3f, min %.3f, max %.3f" % (statistics.median(v), min(v), max(v))


# ------------------------------------------------------------------ generate(), both legs
torch.manual_seed(0)
model = MultiModalBartForConditionalGeneration(MultiModalBartConfig.from_dict(bench.VCG_BASE)).to(dev).eval()
b = make_batch(args.batch, seed=4321)
ids, am = b["input_ids"].to(dev), b["attention_mask"].to(dev)
feats = [f.to(dev) for f in b["image_features"]]
say("# FP8 (e4m3) decoder weights against bf16: vcg_base generate, batch %d, max_length 20" % args.batch)
say("windows %d x %d generates per format, alternated in one process; times in ms" % (args.windows, args.reps))
for leg, kw in (("beam search, 5 beams (320 rows)", dict(num_beams=5, num_return_sequences=1, max_length=20, early_stopping=True)),
                ("greedy (%d rows)" % args.batch, dict(num_beams=1, max_length=20))):
    ms = {f: [] for f in FORMATS}
    steps = 0
    for f in FORMATS:
        model.set_decoder_weight_format(f)
        for _ in range(2):
            out = model.generate(input_ids=ids, image_features=feats, attention_mask=am, **kw)
        torch.cuda.synchronize()
        steps = out.shape[1] - 1
    for w in range(args.windows):
        for f in (FORMATS if w % 2 == 0 else FORMATS[::-1]):
            model.set_decoder_weight_format(f)
            model.generate(input_ids=ids, image_features=feats, attention_mask=am, **kw)   # (repacks: not in the window)
            torch.cuda.synchronize()
            hw.key = (leg, f)
            t0 = time.perf_counter()
            for _ in range(args.reps):
                model.generate(input_ids=ids, image_features=feats, attention_mask=am, **kw)
            torch.cuda.synchronize()
            ms[f].append((time.perf_counter() - t0) / args.reps * 1e3)
            hw.key = None
    say()
    say("## %s, %d decode steps" % (leg, steps))
    for f in FORMATS:
        m = statistics.median(ms[f])
        say("- %-8s ms per generate: %s; per decode step %.3f; %.0f sequences/s; %s" % (f, spread(ms[f]), m / max(steps, 1),
                                                                                       args.batch / m * 1e3, hw.text((leg, f))))
    say("- FP8 / bf16 (medians): %.3f" % (statistics.median(ms["fp8_e4m3"]) / statistics.median(ms["bf16"])))
model.set_decoder_weight_format("bf16")
del model
torch.cuda.empty_cache()

# ------------------------------------------------------------------ the six blocks of a layer, one by one
lib = _lib.load()
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)   # noqa: E731
d, F, H, S, Tmax, Tk = 768, 3072, 12, 64, 20, 10


def blocks(R, nb):
    """[(name, {format: KmbDecodeBlock}, keep)] of one decoder layer at R rows (nb beams per item), random weights"""
    g = lambda *s: (torch.randn(*s, device=dev) * 0.04).to(torch.bfloat16)   # noqa: E731
    x, z, o, hh = g(R, d), g(R, d), g(R, d), g(R, F)
    kc, vc = g(R, Tmax, d), g(R, Tmax, d)
    ckv = g(R // nb, S, 2 * d)
    mask = torch.ones(R // nb, S, dtype=torch.int64, device=dev)
    kv_row = (torch.arange(R, device=dev) // nb).to(torch.int32)
    gam, bet = torch.ones(d, device=dev), torch.zeros(d, device=dev)
    spec = [("self-attention (kind 1)", 3 * d, d, dict(kind=1, in_=z, ld_in=d, gamma=gam, beta=bet, eps=1e-5, ln_out=x, out=o, ld_out=d, H=H,
                                                      q_scale=0.125, Kc=kc, Vc=vc, Tmax=Tmax, ldc=d, Tk=Tk)),
            ("self out projection (kind 0)", d, d, dict(kind=0, in_=o, ld_in=d, residual=x, ld_res=d, out=z, ld_out=d)),
            ("cross-attention (kind 2)", d, d, dict(kind=2, in_=z, ld_in=d, gamma=gam, beta=bet, eps=1e-5, ln_out=x, out=o, ld_out=d, H=H,
                                                   q_scale=0.125, Kc=ckv, Vc=ckv.view(-1)[d:], Tmax=S, ldc=2 * d, Tk=S, kv_row=kv_row,
                                                   key_mask=mask, mask_ld=S, kv_group=nb)),
            ("cross out projection (kind 0)", d, d, dict(kind=0, in_=o, ld_in=d, residual=x, ld_res=d, out=z, ld_out=d)),
            ("fc1 + GeLU (kind 0, wide)", F, d, dict(kind=0, in_=z, ld_in=d, gamma=gam, beta=bet, eps=1e-5, ln_out=x, act=1, out=hh, ld_out=F)),
            ("fc2 (kind 0, K = 3072)", d, F, dict(kind=0, in_=hh, ld_in=F, residual=x, ld_res=d, out=z, ld_out=d))]
    out = []
    for name, N, K, kw in spec:
        W = g(N, K)
        bias = torch.zeros(N, device=dev)
        packed = torch.empty_like(W)
        check(lib.kmb_op_decode_pack(ptr(W), K, N, K, ptr(packed), stream()))
        codes = torch.empty(N * K, dtype=torch.uint8, device=dev)
        exps = torch.empty(N, dtype=torch.int8, device=dev)
        check(lib.kmb_op_decode_pack_fp8(ptr(W), K, N, K, ptr(codes), ptr(exps), stream()))
        per = {}
        for f in FORMATS:
            blk = KmbDecodeBlock(R=R, K=K, N=N, bias=ptr(bias))
            for k, v in kw.items():
                setattr(blk, k, ptr(v) if torch.is_tensor(v) else v)
            blk.W = ptr(packed if f == "bf16" else codes)
            if f != "bf16":
                blk.w_format, blk.w_exp = 1, ptr(exps)
            per[f] = blk
        out.append((name, per, (W, bias, packed, codes, exps, kw)))
    return out


for R, nb in ((320, 5), (64, 1)):
    say()
    say("## the six blocks of one decoder layer at %d rows (%d per item), us per launch, 2000 launches per window" % (R, nb))
    total = {f: 0.0 for f in FORMATS}
    for name, per, keep in blocks(R, nb):
        us = {f: [] for f in FORMATS}
        for f in FORMATS:
            for _ in range(20):
                check(lib.kmb_op_decode_block(C.byref(per[f]), stream()))
        torch.cuda.synchronize()
        for w in range(args.windows):
            for f in (FORMATS if w % 2 == 0 else FORMATS[::-1]):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(2000):
                    check(lib.kmb_op_decode_block(C.byref(per[f]), stream()))
                e1.record()
                torch.cuda.synchronize()
                us[f].append(e0.elapsed_time(e1) * 1e3 / 2000)
        mb, mf = statistics.median(us["bf16"]), statistics.median(us["fp8_e4m3"])
        total["bf16"] += mb
        total["fp8_e4m3"] += mf
        say("- %-30s bf16 %6.2f (min %.2f max %.2f)   fp8 %6.2f (min %.2f max %.2f)   fp8 / bf16 %.3f" % (
            name, mb, min(us["bf16"]), max(us["bf16"]), mf, min(us["fp8_e4m3"]), max(us["fp8_e4m3"]), mf / mb))
    say("- %-30s bf16 %6.2f   fp8 %6.2f   fp8 / bf16 %.3f   (back to back launches of ONE block re-read a warm L2: in a decode step "
        "the six layers' weights alternate)" % ("sum of the six", total["bf16"], total["fp8_e4m3"], total["fp8_e4m3"] / total["bf16"]))

# ------------------------------------------------------------------ quality evidence: reported, not asserted
if not args.no_quality:
    from oracle import goldenlib as G
    from oracle import kmbart_oracle as O
    cfg = {k: bench.VCG_BASE[k] for k in ("activation_dropout", "attention_dropout", "d_model", "decoder_attention_heads", "decoder_ffn_dim",
                                          "decoder_layers", "encoder_attention_heads", "encoder_ffn_dim", "encoder_layers", "init_std",
                                          "max_position_embeddings", "vocab_size", "cls_token_id", "img_feat_id")}
    cfg["dropout"] = 0.0
    ocfg = O.OracleConfig.from_dict(cfg)
    sd = G.golden_state_dict(ocfg, seed=11)
    sd["model.shared.weight"] = sd["model.shared.weight"] * 8.0
    sd["model.decoder.embed_positions.weight"] = sd["model.decoder.embed_positions.weight"] * 40.0
    for k_ in list(sd):
        if k_.endswith("out_proj.weight") or k_.endswith("fc2.weight"):
            sd[k_] = sd[k_] * 3.0
    model = MultiModalBartForConditionalGeneration(MultiModalBartConfig.from_dict(cfg))
    model.load_state_dict(sd, strict=False)
    model.to(dev).eval()
    qb = make_batch(32, seed=99)
    qi, qm, qf = qb["input_ids"].to(dev), qb["attention_mask"].to(dev), [f.to(dev) for f in qb["image_features"]]
    res = {}
    for f in FORMATS:
        model.set_decoder_weight_format(f)
        eng = model._engine
        eng.gen_begin(qi, qf, qm, 1, 9)
        lg = []
        for t in range(8):
            lg.append(eng.gen_step(qb["decoder_input_ids"][:, t].to(dev), t)[:, : cfg["vocab_size"]].float().clone())
        torch.cuda.synchronize()
        out, sc = model.generate(input_ids=qi, image_features=qf, attention_mask=qm, num_beams=5, max_length=10, early_stopping=True,
                                 return_scores=True)
        res[f] = (torch.stack(lg, 1), out.cpu(), sc.float().cpu())
    model.set_decoder_weight_format("bf16")
    la, lb = res["bf16"][0], res["fp8_e4m3"][0]
    ia, ib = res["bf16"][1], res["fp8_e4m3"][1]
    n = max(ia.shape[1], ib.shape[1])
    pad = lambda t: torch.nn.functional.pad(t, (0, n - t.shape[1]), value=1)   # noqa: E731
    same = (pad(ia) == pad(ib)).all(dim=1)
    say()
    say("## quality evidence on the golden full-size model (random weights re-scaled so that searches move): reported, not asserted")
    say("- teacher-forced logits, 32 items x 8 steps: norm-wise relative error of FP8 against bf16 weights %.3e; top-1 token agrees at %.1f%% "
        "of the positions" % (float((lb - la).norm() / la.norm()), 100.0 * float((la.argmax(-1) == lb.argmax(-1)).float().mean())))
    say("- beam 5, max_length 10: %d of %d rows identical; largest length-normalised score gap %.3e (over all rows), %.3e (identical rows)" % (
        int(same.sum()), same.numel(), float((res["bf16"][2] - res["fp8_e4m3"][2]).abs().max()),
        float((res["bf16"][2] - res["fp8_e4m3"][2])[same].abs().max()) if bool(same.any()) else float("nan")))
    say("- random-init logits are near-ties, so row agreement measures rounding, not quality; trained weights were not available")

hw.stop = True
if args.out:
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
