"""CPU: which kernel, which tile_order and which tuner candidates every GEMM shape gets, pinned to a table recorded from the
commit BEFORE the launch path became table-driven (tests/golden/gemm_route.json).

kmb_debug_gemm_route decides exactly as kmb_gemm_launch does and launches nothing, so this runs in milliseconds without a
GPU.  The golden table was not written by the code under test: the same probe was added to a copy of the previous commit
as a recording hook in front of its untouched launch_variant / launch_config / kmb_gemm_launch, that copy was built, and
`KMB_LIB_PATH=<that library> python tests/test_gemm_route_cpu.py --dump tests/golden/gemm_route.json` wrote the file.
A route is out[0] (0: the launch itself, 1: the tuner's candidate list) followed by triples
(configuration, kernel variant, tile_order); see include/kmbart.h."""
import ctypes as C
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "km-bart_amd"))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_route.json")
FORCED = list(range(0, 17))   # 0: the library's own choice; 1..16: KMB_GEMM_VARIANT (16: a number without a kernel)
LAYOUTS = {"fwd": (1, 1), "dgrad": (1, 0), "wgrad": (0, 0)}   # (a_kc, b_kc): X W^T, dY W, dY^T X

# fake operands: aligned, non-null, never dereferenced
A, B, BIAS, OUT, OUT32, AUX, RES, PRE, SLAB, COLSUM, SHIFT, SUMS = (0x10000000 * (i + 1) for i in range(12))


def _up8(v):
    return (v + 7) & ~7


def problem(M, N, K, layout="fwd", act=0, split_k=0, bias=True, out="bf16", **extra):
    from kmbart._lib import KmbGemm
    a_kc, b_kc = LAYOUTS[layout]
    p = KmbGemm()
    p.A, p.B, p.a_kc, p.b_kc, p.M, p.N, p.K = A, B, a_kc, b_kc, M, N, K
    p.lda = _up8(K) if a_kc else _up8(M)
    p.ldb = _up8(K) if b_kc else _up8(N)
    p.act, p.split_k = act, split_k
    if split_k > 1:
        p.slab = SLAB
        bias = False
    if bias:
        p.bias = BIAS
    if out == "bf16":
        p.out_bf16, p.ld_out_bf16 = OUT, _up8(N)
    else:
        p.out_f32, p.ld_out_f32 = OUT32, _up8(N)
    if act == 2:
        p.aux, p.ld_aux = AUX, _up8(N)
    if act == 5:
        p.row_shift, p.row_sums, p.row_sums_ld = SHIFT, SUMS, N // 64
    for k, v in extra.items():
        setattr(p, k, v)
    return p


def cases():
    """name -> KmbGemm: the smallest shapes on each side of every launch rule"""
    c = {}
    # K steps: 320 = five (variant 6's minimum), 256 = four, 192 = three (variant 9), 128 = two (the persistent variants' minimum), 64;
    # K % 64 != 0 runs variant 1 (130 only where K is not the contiguous dimension)
    for K in (320, 256, 192, 128, 64):
        c["fwd_2048x4096_k%d" % K] = problem(2048, 4096, K)
    c["wgrad_2048x4096_k130"] = problem(2048, 4096, 130, "wgrad", bias=False, out="f32")
    c["fwd_2048x4096_k136"] = problem(2048, 4096, 136)
    # exactly 128 tiles of 256x256 / 256x128 / 256x192, one tile row fewer, and exactly 127 tiles
    for N, n127 in ((4096, 127 * 256), (2048, 127 * 128), (3072, 127 * 192)):
        for layout in LAYOUTS:
            c["%s_2048x%d_k320" % (layout, N)] = problem(2048, N, 320, layout, bias=layout == "fwd")
        c["fwd_1792x%d_k320" % N] = problem(1792, N, 320)
        c["fwd_256x%d_k320" % n127] = problem(256, n127, 320)
        c["fwd_256x%d_k320" % (n127 + n127 // 127)] = problem(256, n127 + n127 // 127, 320)
    # 24 workgroups of 128x128: variant 5 with four K steps, not with three (the forward layout goes to the narrow kernel)
    for K in (256, 192):
        for layout in LAYOUTS:
            c["%s_512x768_k%d" % (layout, K)] = problem(512, 768, K, layout, bias=layout == "fwd")
    # more than one 128x128 tile each way or variant 7
    for M, N in ((128, 4096), (129, 4096), (2048, 128), (2048, 136)):
        c["dgrad_%dx%d_k256" % (M, N)] = problem(M, N, 256, "dgrad", bias=False)
    # split-K (weight gradients): the slice-major candidates, variant 5's workgroup count and K steps per slice
    for s in (0, 3, 7):
        c["wgrad_768x3072_k4096_split%d" % s] = problem(768, 3072, 4096, "wgrad", split_k=s, bias=False, out="f32")
        c["wgrad_512x768_k1024_split%d" % s] = problem(512, 768, 1024, "wgrad", split_k=s, bias=False, out="f32")
    # column blocks from N = 32 * 256
    for N in (8192, 8184):
        for K in (320, 192):
            c["fwd_2048x%d_k%d" % (N, K)] = problem(2048, N, K)
    c["dgrad_2048x8192_k320"] = problem(2048, 8192, 320, "dgrad", bias=False)
    # epilogues: GeLU (+ its derivative's store), multiply by the stored derivative with column sums, exp with row sums
    c["fwd_2048x4096_k320_gelu"] = problem(2048, 4096, 320, act=1)
    c["fwd_2048x4096_k320_gelu_preact"] = problem(2048, 4096, 320, act=1, preact=PRE, ld_preact=4096)
    c["dgrad_2048x4096_k320_dgelu_colsum"] = problem(2048, 4096, 320, "dgrad", act=2, bias=False, colsum=COLSUM)
    c["fwd_2048x4096_k320_dgelu"] = problem(2048, 4096, 320, act=2, bias=False)
    for K in (320, 256, 128):
        c["fwd_4096x8192_k%d_act5" % K] = problem(4096, 8192, K, act=5)
    c["fwd_4096x8192_k320_act5_aliased"] = problem(4096, 8192, 320, act=5, out_bf16=A)
    c["fwd_2048x4096_k320_residual"] = problem(2048, 4096, 320, residual=RES, ld_res=4096)
    c["fwd_2048x4096_k320_residual_dropout"] = problem(2048, 4096, 320, residual=RES, ld_res=4096, drop_thr16=6554, drop_scale=1.1)
    c["fwd_2048x4096_k320_nobias"] = problem(2048, 4096, 320, bias=False)
    c["fwd_2048x4096_k320_colscale64"] = problem(2048, 4096, 320, col_scale=0.125, col_scale_n=64)
    c["fwd_2048x4096_k320_colscale32"] = problem(2048, 4096, 320, col_scale=0.125, col_scale_n=32)
    c["fwd_2048x4096_k320_f32"] = problem(2048, 4096, 320, out="f32")
    # an output that aliases an input is never timed
    c["fwd_2048x4096_k320_aliased"] = problem(2048, 4096, 320, out_bf16=A)
    c["fwd_2048x4096_k320_beta"] = problem(2048, 4096, 320, out="f32", beta=1.0)
    # the narrow kernel: forward layout, at most 512 rows, fewer than 128 tiles of 128x128, plain epilogue
    c["fwd_320x768_k256"] = problem(320, 768, 256)
    c["fwd_512x3968_k256"] = problem(512, 3968, 256)
    c["fwd_512x4096_k256"] = problem(512, 4096, 256)
    c["fwd_640x768_k256"] = problem(640, 768, 256)
    c["fwd_320x768_k256_gelu"] = problem(320, 768, 256, act=1)
    c["fwd_320x768_k256_gelu_preact"] = problem(320, 768, 256, act=1, preact=PRE, ld_preact=768)
    c["fwd_320x768_k256_dropout"] = problem(320, 768, 256, drop_thr16=6554, drop_scale=1.1)
    c["fwd_320x768_k1024_split3"] = problem(320, 768, 1024, split_k=3)
    c["dgrad_320x768_k256"] = problem(320, 768, 256, "dgrad", bias=False)
    return c


def routes(lib):
    """{case: [[route for forced in FORCED] for shared_device in (0, 1)]}"""
    out = (C.c_int32 * 128)()
    table = {}
    try:
        for name, p in cases().items():
            table[name] = []
            for shared in (0, 1):
                assert lib.kmb_gemm_shared_device(shared) == 0
                row = []
                for forced in FORCED:
                    n = lib.kmb_debug_gemm_route(C.byref(p), forced, out, len(out))
                    assert n >= 4 and (n - 1) % 3 == 0, (name, shared, forced, n)
                    row.append(list(out[:n]))
                table[name].append(row)
    finally:
        lib.kmb_gemm_shared_device(0)
    return table


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from kmbart import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def got(lib):
    return routes(lib)


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


def test_every_case_is_in_the_golden_table(got, golden):
    assert sorted(got) == sorted(golden)
    assert len(got) >= 60


@pytest.mark.parametrize("shared", (0, 1))
def test_routes_match_the_previous_launch_path(got, golden, shared):
    wrong = [(name, forced, got[name][shared][i], golden[name][shared][i])
             for name in sorted(golden) for i, forced in enumerate(FORCED) if got[name][shared][i] != golden[name][shared][i]]
    assert not wrong, wrong[:8]


def test_the_cases_reach_every_route(golden):
    """the table would pin nothing if the shapes all took one path"""
    fixed = {r[1] & 15 for rows in golden.values() for r in rows[0] if r[0] == 0}
    assert fixed >= {0, 1, 5, 6, 7, 8, 9, 11, 12, 13, 14, 15}, fixed
    lists = [r for rows in golden.values() for r in (rows[0][0], rows[1][0]) if r[0] == 1]
    timed = {c for r in lists for c in r[1::3]}
    assert timed == {5, 21, 85, 7, 23, 8, 24, 11, 27, 12, 28, 13, 29, 14, 30, 15, 31, 87, 88, 9, 6}, timed
    assert {r[2] for rows in golden.values() for r in rows[1] if r[0] == 0 and r[1] == 9} == {12}   # shared device: variant 9 -> 12
    assert golden["fwd_4096x8192_k320_act5_aliased"][0][0][:3] == [0, 11, 11]
    assert golden["fwd_2048x4096_k320_aliased"][0][0][:3] == [0, 7, 7]
    assert golden["wgrad_2048x4096_k130"][0][0][:3] == [0, 1, 1]
    assert golden["fwd_320x768_k256"][0][0][:3] == [0, 0, 0]


def test_probe_refuses_what_the_launch_refuses(lib):
    out = (C.c_int32 * 128)()
    p = problem(2048, 4096, 320)
    assert lib.kmb_debug_gemm_route(C.byref(p), 0, out, 3) == -1        # cap too small for the candidate list
    assert lib.kmb_debug_gemm_route(C.byref(p), -1, out, len(out)) == -1
    p.A = A + 2
    assert lib.kmb_debug_gemm_route(C.byref(p), 0, out, len(out)) == -1  # misaligned operand: kmb_gemm_check


if __name__ == "__main__":   # --dump <path>: record the table from the library KMB_LIB_PATH names (see the module docstring)
    from kmbart import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    lib.kmb_debug_gemm_route.restype = C.c_int
    lib.kmb_debug_gemm_route.argtypes = [C.POINTER(_lib.KmbGemm), C.c_int, C.c_void_p, C.c_int32]
    with open(sys.argv[sys.argv.index("--dump") + 1], "w") as f:
        f.write("{\n" + ",\n".join('"%s": %s' % (k, json.dumps(v, separators=(",", ":"))) for k, v in sorted(routes(lib).items())) + "\n}\n")
