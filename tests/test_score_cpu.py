"""CPU: the scoring call (kmb_score, model.score, src.scoring.perplexity_filter, filter_reason.py) exists at every layer, the filter
loop keeps what the reference's contract keeps, and the gfx950 build of the new kernels has no scratch and no spills."""
import inspect
import math
import os
import re
import subprocess
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "km-bart_amd")
for p in (ROOT, PKG, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

NEW_SYMBOLS = ("kmb_score", "kmb_op_gemm_score", "kmb_op_gemm_score_stats_floats", "kmb_op_score_rows_finish")


def test_symbols_declared_exported_and_prototyped():
    import ctypes
    from kmbart import _lib
    header = open(os.path.join(ROOT, "include", "kmbart.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), "%s is not declared in include/kmbart.h" % name
        assert name in _lib.PROTOTYPES, "%s has no ctypes prototype" % name
        getattr(lib, name)   # AttributeError: not exported
    # the declared contract names its outputs and the tail rows
    decl = header[header.index("int kmb_score(") - 3000:header.index("int kmb_score(") + 400]
    for word in ("token_logprob", "sample_nll", "sample_count", "path_out", "TAIL ROWS"):
        assert word in decl, word
    assert lib.kmb_op_gemm_score_stats_floats.restype is not None
    lib.kmb_op_gemm_score_stats_floats.restype = ctypes.c_int64
    assert lib.kmb_op_gemm_score_stats_floats(512, 50432) == 512 * (50432 // 64) * 2


def test_score_without_labels_or_handle_fails_with_a_message():
    import ctypes
    from kmbart import _lib
    lib = _lib.load()
    b = _lib.KmbBatch(B=1, S=1, T=1)
    assert lib.kmb_score(None, ctypes.byref(b), None, None, None, None, None) != 0
    assert b"kmb_score" in lib.kmb_last_error()


def test_python_surface():
    from src.model import MultiModalBartForConditionalGeneration, MultiModalBartForPreTraining, SequenceScore
    from kmbart.engine import Engine
    want = ["self", "input_ids", "image_features", "attention_mask", "decoder_input_ids", "decoder_attention_mask", "labels"]
    for cls in (MultiModalBartForConditionalGeneration, MultiModalBartForPreTraining):
        sig = inspect.signature(cls.score)
        assert list(sig.parameters) == want
        assert all(sig.parameters[k].default is None for k in want[3:])
    assert list(inspect.signature(Engine.score).parameters) == want
    assert SequenceScore._fields == ("token_logprobs", "nll", "count")
    s = SequenceScore(torch.zeros(2, 3), torch.tensor([3.0, 0.0]), torch.tensor([2, 0], dtype=torch.int32))
    pp = s.perplexity
    assert abs(float(pp[0]) - math.exp(1.5)) < 1e-6 and math.isnan(float(pp[1]))
    from src.scoring import perplexity_filter
    assert list(inspect.signature(perplexity_filter).parameters) == ["model", "loader", "device", "args", "logger"]


def test_filter_cli_help_lists_the_reference_flags():
    r = subprocess.run([sys.executable, os.path.join(PKG, "filter_reason.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in ("--data_dir", "--output_dir", "--checkpoint", "--log_dir", "--split", "--pp_threshold", "--cpu", "--amp", "--batch_size",
                 "--num_workers", "--synthetic"):
        assert flag in r.stdout, flag


class _StubModel:
    """model.score with fixed per-sample sums / counts; records what the loop does with it"""

    def __init__(self, per_batch):
        self.per_batch, self.calls, self.eval_called = per_batch, 0, False

    def eval(self):
        self.eval_called = True
        return self

    def score(self, input_ids, image_features, attention_mask=None, decoder_input_ids=None, decoder_attention_mask=None, labels=None):
        from src.model import SequenceScore
        assert self.eval_called and labels is not None
        nll, count = self.per_batch[self.calls]
        self.calls += 1
        return SequenceScore(torch.zeros(len(nll), 2), torch.tensor(nll, dtype=torch.float32), torch.tensor(count, dtype=torch.int32))


class _Log:
    def __init__(self):
        self.lines = []

    def info(self, msg, pad=False):
        self.lines.append(msg)


def test_perplexity_filter_contract():
    from src.scoring import perplexity_filter
    # batch 0: mean 1.0 (kept), exactly the threshold 2.0 (`<`, not `<=`: dropped), 2.5 (dropped); batch 1: no valid label (NaN: dropped),
    # mean 1.999 (kept)
    model = _StubModel([([4.0, 8.0, 5.0], [4, 4, 2]), ([0.0, 3.998], [0, 2])])
    loader = []
    for idx in ([10, 11, 12], [20, 21]):
        n = len(idx)
        loader.append({"input_ids": torch.zeros(n, 2, dtype=torch.long), "image_features": [torch.zeros(0) for _ in range(n)],
                       "attention_mask": torch.ones(n, 2, dtype=torch.long), "decoder_input_ids": torch.zeros(n, 2, dtype=torch.long),
                       "decoder_attention_mask": torch.ones(n, 2, dtype=torch.long), "labels": torch.zeros(n, 2, dtype=torch.long),
                       "dataset_index": idx})
    log = _Log()
    kept = perplexity_filter(model, loader, "cpu", types.SimpleNamespace(pp_threshold=2.0, amp=False), log)
    assert kept == [10, 21]
    assert model.calls == 2   # one score per batch
    assert len(log.lines) == 2
    assert log.lines[0].startswith("Filtering, Step [1/2], ETA: ") and log.lines[1].startswith("Filtering, Step [2/2], ETA: ")


def _isa(src, tmp_path):
    from build import CSRC, FLAGS
    out = str(tmp_path / (src + ".s"))
    subprocess.check_call(["hipcc", "-x", "hip"] + FLAGS + ["-I" + os.path.join(ROOT, "include"), "-S", "--cuda-device-only", "-o", out,
                           os.path.join(CSRC, src)], stderr=subprocess.DEVNULL)
    return out


def _kernel_meta(asm, pattern):
    """{kernel: metadata text} of the .amdhsa metadata entries whose .name matches"""
    out = {}
    for m in re.finditer(r"- \.agpr_count:.*?(?=\n  - \.agpr_count:|\namdhsa\.target|\Z)", asm, re.S):
        blk = m.group(0)
        nm = re.search(r"\.name:\s+(\S+)", blk)
        if nm and re.search(pattern, nm.group(1)):
            out[nm.group(1)] = blk
    return out


def test_new_kernels_have_no_scratch_and_no_spills(tmp_path):
    lean = open(_isa("gemm_lean.hip", tmp_path)).read()
    loss = open(_isa("loss.hip", tmp_path)).read()
    gemm = _kernel_meta(lean, r"gemm_kernel_leanILb1ELi6E")      # gemm_kernel_lean<true, LN_SCORE>
    fin = _kernel_meta(loss, r"score_rows_finish_kernel|score_segments_kernel")
    assert len(gemm) == 1 and len(fin) == 2, (list(gemm), list(fin))
    for name, blk in list(gemm.items()) + list(fin.items()):
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", blk), name
        assert re.search(r"\.vgpr_spill_count:\s+0\b", blk), name
    for name, blk in fin.items():
        assert re.search(r"\.sgpr_spill_count:\s+0\b", blk), name
    # the persistent kernel body parks scalars of its tile schedule in VGPR lanes (v_writelane: registers, not memory) in EVERY instance; the
    # scoring epilogue must not add to what the cross-entropy instance (act 5) already carries
    ce = _kernel_meta(lean, r"gemm_kernel_leanILb1ELi5E")
    spills = lambda blk: int(re.search(r"\.sgpr_spill_count:\s+(\d+)", blk).group(1))   # noqa: E731
    assert spills(next(iter(gemm.values()))) <= spills(next(iter(ce.values()))), (spills(next(iter(gemm.values()))), spills(next(iter(ce.values()))))
    # the scoring class stores statistics only: no 16-byte global store (an output tile) anywhere in it, and its body has no scratch access
    name = next(iter(gemm))
    body = lean[lean.index(name + ":"):]
    body = body[:body.index(".Lfunc_end")]
    assert "scratch_" not in body
    # eight statistic stores (one (maximum, sum-exp) pair per 16-row chunk) and no output tile: the only wider stores left are the
    # two that zero the tile counters where a launch retires (two retire sites)
    assert body.count("global_store_dwordx2") == 8, body.count("global_store_dwordx2")
    assert body.count("global_store_dwordx4") <= 4 and not re.search(r"global_store_\w+ .* nt\b", body)
    assert "global_load_lds_dword " in body   # the L2 touch of every lean instance


def test_gemm_audits_hold_with_the_scoring_instance(tmp_path):
    """tools/gemm_tr_asm_hazards.py and the K-loop audit (tools/gemm_kloop_audit.py), as tests/test_cabi_cpu.py runs them, with the new
    instance compiled in -- and the instance itself is among the audited K loops."""
    from gemm_kloop_audit import audit_file
    out = _isa("gemm_lean.hip", tmp_path)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gemm_tr_asm_hazards.py"), out], capture_output=True, text=True)
    assert r.returncode == 0 and "total violations 0" in r.stdout, r.stdout[-3000:]
    rows = audit_file(out, "gemm_lean.hip")
    assert len(rows) >= 13, len(rows)
    mine = [row for row in rows if row[0].startswith("gemm_kernel_lean<true, 6>")]
    assert len(mine) == 1, [row[0] for row in rows]
    for row in rows:
        assert row[6] == 0, "%s: v_accvgpr moves inside its K step" % row[0]
        assert row[8] == 0, "%s: scratch accesses inside its K step" % row[0]
    ref = [row for row in rows if row[0].startswith("gemm_kernel_lean<true, 5>")][0]
    assert mine[0][2:6] == ref[2:6] and mine[0][9] == ref[9], (mine[0], ref)   # same K step as act 5's instance: MFMAs, pieces, reads, waits
