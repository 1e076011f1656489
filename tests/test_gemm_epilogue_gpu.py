"""GPU: every GEMM epilogue class, under every launch variant, against float64 -- element by element, with sentinels around every output.

The reference, the bounds (derived in its docstring) and the seeded cases are tests/gemm_epi_ref.py's; test_gemm_epilogue_cpu.py shows that
an fp32 emulation keeps to half of each bound and that the reference sees a list of deliberate slips.  The limit here is 1.0.

The launch variant is a per-process choice, so each (group, variant) runs in a child of its own: this file behind KMB_GEMM_EPI_CHILD, with
KMB_GEMM_VARIANT = v, KMB_TILE_ORDER = 0, KMB_GEMM_AUTOTUNE = 0; the "0" children force nothing (the route to the narrow kernel).  Children
run one at a time, each under its own timeout, and print one JSON line that the parent caches.  A child that faults, aborts or times out
ends the run: no further child is started.

  group S (256 x 256, 200 x 132, 300 x 268, K = 256; variants 1, 7, 5, 8 and unforced): the 21 classes of gemm_epi_ref._classes;
          under variant 1 also the K edges 8, 72, 136, 200 (classes 2, 4, 10, 18), one of them under forced 7 (variant 1 runs it whatever
          is forced); under 1, 7 and unforced also M = 1, 5 at N = 268 and a split-K launch at 5 x 136.
  group P (2048 x 4096 x 384 whole tiles, 2040 x 4092 x 384 edges; variants 7, 11 .. 15, 6, 9): the persistent kernels' lean-epilogue classes
          on the whole-tile shape, their general wave path on the edge shape; 6 and 9 on the whole-tile shape.  GeLU with dropout also at
          2304 x 3840 x 384, whole tiles for bn = 128, 192 and 256: there 13 runs it too (4096 is no multiple of 192: 13 -> 8 -> 7).
  The narrow kernel's fp32 store with beta = 0.5: two K-contiguous bias cases (5 x 268, 200 x 132) under unforced, 1 and 7.

Per case the child
  * asks kmb_debug_gemm_route which kernel variant runs the launch (EXPECT below is written by hand from gemm.hip's rules: a mismatch fails);
  * allocates every output with two extra rows and ld = roundup8(N) + 16 (the fp32 output once with ld = N + 1), filled with NaN; after the
    launch rows >= M and columns >= N still hold the NaN bits and no NaN is left inside (so beta == 0 never read the old output);
  * judges every element of every output against exact() with row_ref.assert_elementwise; the column sums per 256-row band (four 64-row
    partial rows folded in float64);
  * checks dropped elements: the residual's bits exactly (or zero), kept ones different from the residual wherever the reference is more
    than two bounds away from it; the mask is kmb_op_dropout_mask's;
  * launches again into re-poisoned outputs: the same bits; GeLU without the stored derivative: the same GeLU bits.
Across children a case's output bits equal variant 7's (not the K edges, which only variant 1 runs; column sums are judged per band); a
difference is reported with the rows and columns that hold it (one hash per row and per column travels with each md5).

Measured on an MI355X (worst err / bound per class group, child wall times): DESIGN.md section 6v."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests")]
import gemm_epi_ref as G  # noqa: E402

CHILD_TIMEOUT = 60        # seconds: the slowest child took 5.1 s of wall time on an MI355X; ten times that, but never below 60

S_KK_NARROW = ("c01_plain", "c02_bias_ld4", "c02_bias_ldodd", "c03_scale64", "c03_scale20", "c03_scaleN", "c04_gelu_nopre", "c07_res",
               "c09_gelu_res")
K_EDGE_UNDER_7 = "E200x132k72_c02_bias_ld4"


def child_cases(key):
    S, E, F = G.names("S"), G.names("E"), G.names("F")
    PW, PE = G.names("PW_") + G.names("PG_"), G.names("PE_")
    return {
        "S1": S + E + F,
        "S7": S + F + [K_EDGE_UNDER_7],
        "S5": [n for n in S if "split" not in n],                                # at least 4 K steps per slice
        "S8": S,
        "S0": [n for n in S if n.split("_", 1)[1] in S_KK_NARROW] + F,        # what narrow_ok admits
        "P7": PW + PE, "P11": PW + PE, "P12": PW + PE, "P13": PW + PE, "P14": PW + PE, "P15": PW + PE,
        "P6": PW, "P9": PW,
    }[key]


KEYS = ("S1", "S7", "S5", "S8", "S0", "P7", "P11", "P12", "P13", "P14", "P15", "P6", "P9")

# The kernel variant each (child, case) is expected to run: (the child's default, [(part of the case's name, variant)]), by hand from gemm.hip:
#   K % 64 != 0 -> 1 whatever is forced (gemm_route);  unforced + narrow_ok (kk, M <= 512, < 128 tiles, act <= 1, no preact / colsum /
#   dropout, split-K only with N % 8 == 0) -> 0;  v7d_ok: <= 256 workgroups, >= 4 K steps per slice (K = 256 unsplit: 4; the split cases are
#   not in S5's list);  v8_ok: M > 128 and N > 128 (every S shape, 129 columns of class 19 included), but gelu_drop_ok(p, 0) is false for
#   GeLU with dropout: 8 -> 7;  v11_ok: no split, K >= 128, >= 128 tiles of 256 x bn (both P shapes, bn = 128, 192, 256);  gelu_drop_ok(p, bn)
#   wants M % 256 == 0 and N % bn == 0: 4096 % 192 = 64, so 13 -> 8 -> 7 like the eight-wave 14 and 15 (bn = 0);  kmb_gemm_lean_ok: A
#   K-contiguous, >= 5 K steps (384 / 64 = 6), whole 256 x 256 tiles, bf16 output only, col_scale_n % 64 == 0, a class of ln_class -- all nine
#   PW cases;  kmb_gemm_pair_ok: both operands K-contiguous, K % 192 == 0: the two kt cases fall back 9 -> 11.  PG (2304 x 3840): 9 x 15 = 135
#   tiles of 256 x 256, 9 x 20 of 256 x 192, 9 x 30 of 256 x 128, all whole: 11, 12, 13, 6 and 9 run GeLU with dropout themselves.
EXPECT = {
    "S1": (1, []),
    "S7": (7, [("E200x132k", 1)]),
    "S5": (5, []),
    "S8": (8, [("c05_gelu_drop", 7)]),
    "S0": (0, []),
    "P7": (7, []),
    "P11": (11, []),
    "P12": (12, []),
    "P13": (13, [("PW_gelu_drop", 7)]),          # PG_gelu_drop (N = 3840 = 20 x 192) stays on 13
    "P14": (14, [("_gelu_drop", 7)]),
    "P15": (15, [("_gelu_drop", 7)]),
    "P6": (6, []),
    "P9": (9, [("PW_kt_", 11)]),
}
# how many cases each child must have run on its own variant (87 = 3 shapes x 29 cases, 16 K edges, 13 few-row / narrow-kernel cases)
OWN_VARIANT_COUNT = {"S1": 87 + 16 + 13, "S7": 87 + 13, "S5": 87 - 3, "S8": 87 - 3, "S0": 27 + 13, "P7": 15, "P11": 15, "P12": 15, "P13": 14,
                     "P14": 13, "P15": 13, "P6": 10, "P9": 8}


def expected_variant(key, name):
    default, rules = EXPECT[key]
    for part, v in rules:
        if part in name:
            return v
    return default


def class_group(name):
    if name.startswith("PW_") or name.startswith("PG_"):
        return "lean"
    if name.startswith("PE_"):
        return "wave"
    if name.startswith("E"):
        return "k_edge"
    if name.startswith("F"):
        return "few_rows"
    c = int(name.split("_")[1][1:])
    return {1: "plain_bias_scale", 2: "plain_bias_scale", 3: "plain_bias_scale", 4: "gelu", 5: "gelu", 9: "gelu", 6: "dropout_residual",
            7: "dropout_residual", 21: "dropout_residual", 8: "tanh", 10: "kt", 11: "kt", 12: "kt", 13: "kt", 14: "act2", 15: "act2",
            16: "act2", 17: "act4", 18: "tt_f32", 19: "tt_f32", 20: "split_k"}[c]


KEY_GROUPS = [(k, g) for k in KEYS for g in sorted(set(class_group(n) for n in child_cases(k)))]


# ------------------------------------------------------------------------------------------------ the child
def child(key):
    import torch
    sys.path[:0] = [ROOT, os.path.join(ROOT, "km-bart_amd")]
    from kmbart import _lib
    from kmbart._lib import KmbGemm, check, ptr
    from gpu_util import DEV, dropout_mask, stream
    lib = _lib.load()
    forced = int(os.environ.get("KMB_GEMM_VARIANT", "0"))
    bf, f32 = torch.bfloat16, torch.float32
    report = {}

    def bits(t):
        return t.view(torch.int16 if t.dtype == bf else torch.int32)

    def md5(t):
        """the bits' md5 and one hash per row and per column, so that the parent can name where two children differ"""
        b = bits(t.reshape(-1, t.shape[-1]).contiguous())
        w = lambda n: ((torch.arange(n, device=DEV, dtype=torch.int64) * 2654435761 + 12345) | 1)
        b64 = b.to(torch.int64)
        return dict(md5=hashlib.md5(b.cpu().numpy().tobytes()).hexdigest(),
                    rows=((b64 * w(b.shape[1])).sum(1) & 0x7FFFFFFF).tolist(), cols=((b64 * w(b.shape[0])[:, None]).sum(0) & 0x7FFFFFFF).tolist())

    def alloc(c):
        M, N = c["M"], c["N"]
        ld = G.up8(N) + 16
        o = {}
        if c["split"] > 1:
            o["slab"] = torch.full((c["split"] * M + 2, N), G.NAN, dtype=f32, device=DEV)
            return o
        if c["bf16"]:
            o["out_bf16"] = torch.full((M + 2, ld), G.NAN, dtype=bf, device=DEV)
        if c["f32"]:
            o["out_f32"] = torch.full((M + 2, ld if c["ldf32"] == "pad" else N + 1), G.NAN, dtype=f32, device=DEV)
            if c["beta"] != 0.0:
                o["out_f32"][:M, :N] = c["old"]
        if c["preact"]:
            o["preact"] = torch.full((M + 2, ld), G.NAN, dtype=bf, device=DEV)
        if c["cs"]:
            o["colsum"] = torch.full(((M + 63) // 64 + 2, N), G.NAN, dtype=f32, device=DEV)
        return o

    def struct(c, o, with_preact=True):
        p = KmbGemm()
        A, B = c["A"], c["B"]
        p.A, p.B, p.lda, p.ldb, p.a_kc, p.b_kc = ptr(A), ptr(B), A.stride(0), B.stride(0), int(c["a_kc"]), int(c["b_kc"])
        p.M, p.N, p.K = c["M"], c["N"], c["K"]
        p.bias = ptr(c["bias_t"])
        p.col_scale, p.col_scale_n, p.act = c["col_scale"], c["csn"], c["act"]
        if c["preact"] and with_preact:
            p.preact, p.ld_preact = ptr(o["preact"]), o["preact"].stride(0)
        if c["aux"] is not None:
            p.aux, p.ld_aux = ptr(c["aux"]), c["aux"].stride(0)
        p.drop_thr16, p.drop_seed, p.drop_scale = c["drop_thr"], c["drop_seed"], c["drop_scale"]
        if c["res"]:
            p.residual, p.ld_res = ptr(c["residual"]), c["residual"].stride(0)
        if "out_bf16" in o:
            p.out_bf16, p.ld_out_bf16 = ptr(o["out_bf16"]), o["out_bf16"].stride(0)
        if "out_f32" in o:
            p.out_f32, p.ld_out_f32 = ptr(o["out_f32"]), o["out_f32"].stride(0)
        p.beta = c["beta"]
        p.split_k = c["split"]
        p.slab = ptr(o.get("slab"))
        p.colsum = ptr(o.get("colsum"))
        p.tile_order = int(os.environ.get("KMB_TILE_ORDER", "0"), 0)
        return p

    def launch(c, with_preact=True):
        o = alloc(c)
        check(lib.kmb_op_gemm(C.byref(struct(c, o, with_preact)), stream()))
        torch.cuda.synchronize()
        return o

    for name in child_cases(key):
        t0 = time.time()
        c = G.to_device(G.case(name), DEV)
        M, N = c["M"], c["N"]
        fails, ratios, sums = [], {}, {}
        route = (C.c_int32 * 128)()
        n = lib.kmb_debug_gemm_route(C.byref(struct(c, alloc(c))), forced, route, len(route))
        rec = dict(ran=int(route[2]) if n >= 4 and route[0] == 0 else -1, fails=fails, ratios=ratios, md5=sums)
        report[name] = rec
        o = launch(c)
        keep = dropout_mask(c["drop_seed"], c["drop"], M, N) if c["drop"] else None
        ex = G.exact(c, keep)

        def judge(got, ref, bound, what):
            try:
                ratios[what] = G.assert_elementwise(got, ref, bound, name + " " + what)
            except AssertionError as e:
                ratios[what] = float("inf")
                fails.append(str(e))

        def sentinels(what, rows, cols):
            full, fresh = o[what], alloc(c)[what]
            if not (torch.equal(bits(full)[rows:], bits(fresh)[rows:]) and torch.equal(bits(full)[:rows, cols:], bits(fresh)[:rows, cols:])):
                fails.append("%s %s: a sentinel beyond row %d / column %d was overwritten" % (name, what, rows, cols))
            if bool(torch.isnan(full[:rows, :cols]).any()):
                fails.append("%s %s: NaN left inside the %d x %d region" % (name, what, rows, cols))

        if c["split"] > 1:
            sentinels("slab", c["split"] * M, N)
            slabs = o["slab"][:c["split"] * M].view(c["split"], M, N)
            judge(G.f64(slabs).sum(0), ex["v"], ex["v_slack"], "slab sum")
            sums["slab"] = md5(slabs)
        if "out_bf16" in o:
            sentinels("out_bf16", M, N)
            judge(o["out_bf16"][:M, :N], ex["v"], G.bf16_bound(ex["v"], ex["v_slack"]), "out_bf16")
            sums["out_bf16"] = md5(o["out_bf16"][:M, :N])
        if "out_f32" in o:
            sentinels("out_f32", M, N)
            judge(o["out_f32"][:M, :N], ex["f32"], ex["f32_slack"], "out_f32")
            sums["out_f32"] = md5(o["out_f32"][:M, :N])
        if "preact" in o:
            sentinels("preact", M, N)
            judge(o["preact"][:M, :N], ex["pre"], G.bf16_bound(ex["pre"], ex["pre_slack"]), "preact")
            sums["preact"] = md5(o["preact"][:M, :N])
        if "colsum" in o:
            rows = (M + 63) // 64
            sentinels("colsum", rows, N)
            ref, bound = G.colsum_bands(ex, M)
            judge(G.fold_bands(o["colsum"], M), ref, bound, "colsum bands")
        if c["drop"]:
            res = c["residual"][:M, :N] if c["res"] else None
            res64 = G.f64(res) if c["res"] else torch.zeros_like(ex["v"])
            outs = [(k, o[k][:M, :N], ex["f32"] if k == "out_f32" else ex["v"],
                     ex["f32_slack"] if k == "out_f32" else G.bf16_bound(ex["v"], ex["v_slack"])) for k in ("out_bf16", "out_f32") if k in o]
            for k, got, ref, bound in outs:
                want = (res.to(got.dtype) if c["res"] else torch.zeros_like(got))
                if not torch.equal(bits(got)[~keep], bits(want)[~keep]):
                    fails.append("%s %s: a dropped element is not the residual's bits (or zero)" % (name, k))
                far = keep & ((ref - res64).abs() > 2 * bound)
                if bool((G.f64(got)[far] == res64[far]).any()):
                    fails.append("%s %s: a kept element equals the residual" % (name, k))
            if "preact" in o and bool((o["preact"][:M, :N][~keep] != 0).any()):
                fails.append("%s preact: a dropped element's derivative is not zero" % name)
        again = launch(c)
        for k in o:
            if not torch.equal(bits(o[k]), bits(again[k])):
                fails.append("%s %s: a second launch gave other bits" % (name, k))
        if c["act"] == 1 and c["preact"] and not c["drop"]:
            bare = launch(c, with_preact=False)
            for k in ("out_bf16", "out_f32"):
                if k in o and not torch.equal(bits(o[k][:M, :N]), bits(bare[k][:M, :N])):
                    fails.append("%s %s: GeLU without the stored derivative gave other bits" % (name, k))
            if not bool(torch.isnan(bare["preact"]).all()):
                fails.append("%s: preact written without being passed" % name)
        rec["seconds"] = round(time.time() - t0, 3)
    print("JSON" + json.dumps(report))


# ------------------------------------------------------------------------------------------------ the parent
_results = {}
_dead = []


def run_child(key):
    if key not in _results:
        assert not _dead, "an earlier child did not end cleanly, no further child is started: %s" % _dead[0]
        env = dict(os.environ, KMB_GEMM_EPI_CHILD=key, KMB_TILE_ORDER="0", KMB_GEMM_AUTOTUNE="0")
        env.pop("KMB_GEMM_VARIANT", None)
        env.pop("KMB_GEMM_TUNE_FILE", None)
        if key[1:] != "0":
            env["KMB_GEMM_VARIANT"] = key[1:]
        t0 = time.time()
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired as e:
            _dead.append("child %s ran into its %d s limit: %s" % (key, CHILD_TIMEOUT, str(e.stderr)[-2000:]))
            raise AssertionError(_dead[0])
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("JSON")]
        if r.returncode != 0 or not line:
            _dead.append("child %s exit %d: %s %s" % (key, r.returncode, r.stdout[-2000:], r.stderr[-3000:]))
            raise AssertionError(_dead[0])
        _results[key] = json.loads(line[0][4:])
        print("child %s: %d cases, %.1f s wall, %.1f s in the cases" % (key, len(_results[key]), time.time() - t0,
                                                                       sum(rec["seconds"] for rec in _results[key].values())))
    return _results[key]


@pytest.mark.parametrize("key", KEYS)
def test_every_launch_ran_the_expected_kernel_variant(key):
    got = run_child(key)
    assert sorted(got) == sorted(child_cases(key))
    wrong = {name: (rec["ran"], expected_variant(key, name)) for name, rec in got.items() if rec["ran"] != expected_variant(key, name)}
    assert not wrong, wrong
    own = int(key[1:])
    assert sum(1 for rec in got.values() if rec["ran"] == own) == OWN_VARIANT_COUNT[key]


def test_every_variant_runs_its_classes():
    """group S: the 21 classes under 1, 7 and 8 (8 hands GeLU with dropout to 7), all but split-K under 5, the narrow kernel's nine plus the
    few-row cases under 0; group P: the lean and the wave classes under 11 .. 15, the lean classes under 6 and 9"""
    ran = {}
    for key in KEYS:
        for name in child_cases(key):
            ran.setdefault(expected_variant(key, name), set()).add(name)
    classes = lambda v, prefix: set(n.split("_")[1] for n in ran[v] if n.startswith(prefix))
    allc = set("c%02d" % k for k in range(1, 22))
    assert classes(1, "S") == allc and classes(7, "S") == allc
    assert classes(5, "S") == allc - {"c20"} and classes(8, "S") == allc - {"c05"}
    assert classes(0, "S") == {"c01", "c02", "c03", "c04", "c07", "c09"} and len([n for n in ran[0] if n.startswith("F")]) == 13
    assert len([n for n in ran[1] if n.startswith("E")]) == 16
    for v in (11, 12):
        assert len([n for n in ran[v] if n.startswith("PW_")]) >= 9 and len([n for n in ran[v] if n.startswith("PE_")]) == 5
    for v in (13, 14, 15):
        assert len([n for n in ran[v] if n.startswith("PW_")]) == 8 and len([n for n in ran[v] if n.startswith("PE_")]) == 5
    assert len(ran[6]) == 10 and len(ran[9]) == 8
    for v in (11, 12, 13, 6, 9):          # GeLU with dropout, the masked derivative: every variant that carries the class runs it against float64
        assert "PG_gelu_drop" in ran[v], v
    assert "PW_gelu_drop" in ran[11] and "PW_gelu_drop" in ran[12] and "PW_gelu_drop" in ran[6] and "PW_gelu_drop" in ran[9]
    for n in ("F5x268_kk_bias_betah", "F200x132_kk_bias_betah"):          # the narrow kernel's fp32 store with beta != 0
        assert n in ran[0] and n in ran[7]


@pytest.mark.parametrize("key,group", KEY_GROUPS)
def test_every_element_within_its_bound_and_every_sentinel_intact(key, group):
    got = run_child(key)
    fails, worst = [], {}
    for name, rec in sorted(got.items()):
        if class_group(name) != group:
            continue
        fails += rec["fails"]
        for what, r in rec["ratios"].items():
            worst[what] = max(worst.get(what, 0.0), r)
    print("%s %-18s worst err / bound: %s" % (key, group, "  ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    assert worst and not fails, "\n".join(fails[:20])
    assert all(r <= 1.0 for r in worst.values()), worst


@pytest.mark.parametrize("key", [k for k in KEYS if k not in ("S7", "P7")])
def test_bits_equal_variant_7(key):
    ref, got = run_child(key[0] + "7"), run_child(key)
    shared = [n for n in got if n in ref and not n.startswith("E")]
    assert shared and (key != "S1" or len(shared) == 87 + 13)
    wrong = []
    for n in shared:
        assert sorted(got[n]["md5"]) == sorted(ref[n]["md5"]), n
        for k, g in got[n]["md5"].items():
            r = ref[n]["md5"][k]
            if g["md5"] != r["md5"]:
                rows = [i for i, (a, b) in enumerate(zip(g["rows"], r["rows"])) if a != b]
                cols = [i for i, (a, b) in enumerate(zip(g["cols"], r["cols"])) if a != b]
                wrong.append("%s %s: %d rows x %d columns hold other bits than under variant 7 (at least %d elements), the first at (%s, %s); rows %s columns %s"
                             % (n, k, len(rows), len(cols), max(len(rows), len(cols)), rows[:1], cols[:1], rows[:8], cols[:8]))
    assert not wrong, "\n".join(wrong[:20])


if __name__ == "__main__" and os.environ.get("KMB_GEMM_EPI_CHILD"):
    child(os.environ["KMB_GEMM_EPI_CHILD"])
