"""CPU: the beam-sampling step's C-ABI is exported and prototyped, and its gfx950 kernel uses no scratch (no spills)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "km-bart_amd", "csrc")


def test_symbols_exported_and_prototyped():
    from kmbart import _lib
    header = open(os.path.join(ROOT, "include", "kmbart.h")).read()
    for name in ("kmb_beam_sample_step", "kmb_gen_beam_sample_step"):
        assert name in _lib.PROTOTYPES, name
        assert re.search(r"\bint %s\(" % name, header), name
    lib = _lib.load()
    assert lib.kmb_beam_sample_step is not None and lib.kmb_gen_beam_sample_step is not None


def test_kernel_has_no_scratch_and_no_spills(tmp_path):
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    out = tmp_path / "beam_sample.s"
    r = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O3", "-fno-slp-vectorize", "-std=c++17", "-ffp-contract=off",
                        "--cuda-device-only", "-S", os.path.join(CSRC, "beam_sample.hip"), "-o", str(out)],
                       capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail(r.stderr[-2000:])
    asm = out.read_text()
    kernels = re.findall(r"\.name:\s+(\S*beam_sample_(?:row|merge)_kernel\S*)", asm)
    assert len(kernels) == 2, "the row and merge kernels are not both in the code object"
    assert re.findall(r"\.private_segment_fixed_size:\s+(\d+)", asm) == ["0"] * len(re.findall(r"\.private_segment_fixed_size:", asm))
    assert set(re.findall(r"\.vgpr_spill_count:\s+(\d+)", asm)) == {"0"}
