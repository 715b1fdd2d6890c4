"""Which kernel a GEMM takes (csrc/gemm_plan.h), on the CPU: the header is host-only code, so a small program
(tests/capi/gemm_plan_probe.cpp, built with the address and undefined-behaviour sanitizers, its own process) prints the
plan of the products that comments and GPU tests name -- the linear layers' backward pairs, the encoder fc forward and
weight gradient on the tiled kernel, the GEMM_CASES -- at 256 compute units under every value of gemm_tile and
gemm_mfma, and the lines are compared with EXPECTED below.  EXPECTED was recorded from the code as it stood before the
decisions moved into the header (gemm_plan and the pair choice of curla_linear_bwd inside gemm.hip, with the option
and compute-unit queries stubbed), not from the header."""
import os
import subprocess

import pytest

from tests.test_gpu_kernels import GEMM_CASES, LINEAR_BWD_CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "curla_amd", "csrc")
PROBE = os.path.join(ROOT, "tests", "capi", "gemm_plan_probe.cpp")
TILES = ["auto", "6464", "6432", "3232", "12864"]  # option values in the order of options.h
MFMAS = ["auto", "f32", "b3"]


def tup(kind, M, N, K, nb=1, ksplit=1, ak=0, bk=0, vecA=1, vecB=1, bias=0, mask=0, relu=0, colsum=0, nptr=0, cu=256,
        tile=0, mfma=0, linear_bwd=0, force_big=0):
    return f"{kind} {M} {N} {K} {nb} {ksplit} {ak} {bk} {vecA} {vecB} {bias} {mask} {relu} {colsum} {nptr} {cu} {tile} " \
           f"{mfma} {linear_bwd} {force_big}"


def products():
    """(name, the probe's fields without the options)"""
    out = []
    for B, N, K, nb, _shared_x, with_db in LINEAR_BWD_CASES:
        out.append((f"linear_bwd {B}x{N}x{K} nb{nb}", dict(kind="bwd", M=B, N=N, K=K, nb=nb, mask=1, colsum=int(with_db))))
        if with_db:  # an MLP's first layer as the heads run it: its input is no ReLU output, so dx has no mask
            out.append((f"linear_bwd {B}x{N}x{K} nb{nb} no mask", dict(kind="bwd", M=B, N=N, K=K, nb=nb, colsum=1)))
    # the encoder fc forward on the tiled kernel, [512 x 30752] . [30752 x 50] split 32 ways along K: one encoder by
    # strides, three by pointer (curla_gemm_multi)
    out.append(("fc fwd splitk32", dict(kind="gemm", M=512, N=50, K=30752, ksplit=32)))
    out.append(("fc fwd splitk32 x3", dict(kind="gemm", M=512, N=50, K=30752, nb=3, ksplit=32, nptr=3)))
    # its weight gradient dW[f][n] = sum_b dz[b][f] x[b][n]: M = 50, both operands k-major
    out.append(("fc dW M50", dict(kind="gemm", M=50, N=30752, K=512, ak=1, bk=1)))
    for M, N, K, ak, bk, nb in GEMM_CASES:  # as test_gemm runs them: dense operands, bias + ReLU and mask epilogues
        lda, ldb = (M if ak else K), (N if bk else K)
        vecA, vecB = int(lda % 4 == 0 and (M * K) % 4 == 0), int(ldb % 4 == 0 and (N * K) % 4 == 0)
        base = dict(kind="gemm", M=M, N=N, K=K, nb=nb, ak=ak, bk=bk, vecA=vecA, vecB=vecB)
        out.append((f"gemm {M}x{N}x{K} ak{ak} bk{bk} nb{nb}", dict(base, bias=1, relu=1)))
        out.append((f"gemm {M}x{N}x{K} ak{ak} bk{bk} nb{nb}", dict(base, mask=1)))  # (one plan for both epilogues)
    return out


def tuples():
    """(name with the option values, probe input line): every product under every gemm_tile x gemm_mfma, the backward
    pairs also as two launches (linear_bwd = split)"""
    out = []
    for name, fields in products():
        for ti, tile in enumerate(TILES):
            for mi, mfma in enumerate(MFMAS):
                out.append((f"{name} [{tile}/{mfma}]", tup(tile=ti, mfma=mi, **fields)))
        if fields["kind"] == "bwd":
            out.append((f"{name} [split]", tup(linear_bwd=1, **fields)))
    return out


def g(tbm, tbn, fast, b3, kchunk, name="gemm", small=0):
    """the probe's line for one product (none of the products here is wide or streams its output)"""
    return f"{name} rc=0 small={small} wide=0 tbm={tbm} tbn={tbn} fast={fast} b3={b3} kchunk={kchunk} stream_c=0"


def two(dw, dx):
    """... for a backward pass as two launches: the weight gradient's plan and the data gradient's, g() arguments"""
    return f"bwd rc=0 two {g(*dw, name='dW', small=int(dw[0] == 16))} {g(*dx, name='dx', small=int(dx[0] == 16))}"


def pair(kind, tiles, b3, grid, n1, n2, kchunk, second_first=0):
    """... and in one launch"""
    return f"bwd rc=0 {kind} second_first={second_first} tiles={tiles} b3={b3} grid={grid} n1={n1} n2={n2} " \
           f"kchunk={kchunk} stream_c=0,0"


ALL = "auto/auto auto/f32 auto/b3 6464/auto 6464/f32 6464/b3 6432/auto 6432/f32 6432/b3 3232/auto 3232/f32 3232/b3 " \
      "12864/auto 12864/f32 12864/b3"
SMALL = (16, 16, 0, 0, 0)

# product -> {plan line: the option settings "gemm_tile/gemm_mfma" (or "split") under which the product gets it}
EXPECTED = {
    "linear_bwd 512x1024x1024 nb2": {
        pair("big_pair", "128,64,128,64", 1, "16,8,16,4", 256, 128, "512,1024", 1): "auto/auto auto/b3 12864/auto 12864/b3",
        pair("tiled_pair", "64,64,64,32", 0, "16,16,32,8", 512, 512, "512,1024"): "auto/f32 12864/f32",
        pair("tiled_pair", "64,64,64,64", 0, "16,16,16,8", 512, 256, "512,1024"): "6464/auto 6464/f32",
        pair("tiled_pair", "64,64,64,64", 1, "16,16,16,8", 512, 256, "512,1024"): "6464/b3",
        pair("tiled_pair", "64,32,64,32", 0, "32,16,32,8", 1024, 512, "512,1024"): "6432/auto 6432/f32",
        pair("tiled_pair", "64,32,64,32", 1, "32,16,32,8", 1024, 512, "512,1024"): "6432/b3",
        two((32, 32, 1, 0, 512), (32, 32, 1, 0, 1024)): "3232/auto 3232/f32",
        two((32, 32, 1, 1, 512), (32, 32, 1, 1, 1024)): "3232/b3",
        two((128, 64, 1, 1, 512), (64, 32, 1, 0, 1024)): "split",
    },
    "linear_bwd 512x1024x1024 nb1": {
        pair("tiled_pair", "64,32,32,32", 0, "32,16,32,16", 512, 512, "512,1024"): "auto/auto auto/f32 12864/f32",
        pair("tiled_pair", "64,32,32,32", 1, "32,16,32,16", 512, 512, "512,1024"): "auto/b3",
        pair("tiled_pair", "64,64,64,64", 0, "16,16,16,8", 256, 128, "512,1024"): "6464/auto 6464/f32",
        pair("tiled_pair", "64,64,64,64", 1, "16,16,16,8", 256, 128, "512,1024"): "6464/b3",
        pair("tiled_pair", "64,32,64,32", 0, "32,16,32,8", 512, 256, "512,1024"): "6432/auto 6432/f32",
        pair("tiled_pair", "64,32,64,32", 1, "32,16,32,8", 512, 256, "512,1024"): "6432/b3",
        two((32, 32, 1, 0, 512), (32, 32, 1, 0, 1024)): "3232/auto 3232/f32",
        two((32, 32, 1, 1, 512), (32, 32, 1, 1, 1024)): "3232/b3",
        pair("big_pair", "128,64,128,64", 1, "16,8,16,4", 128, 64, "512,1024", 1): "12864/auto 12864/b3",
        two((64, 32, 1, 0, 512), (32, 32, 1, 0, 1024)): "split",
    },
    "linear_bwd 1024x1024x1024 nb2": {
        pair("big_pair", "128,64,128,64", 1, "16,8,16,8", 256, 256, "1024,1024", 1): "auto/auto auto/b3 12864/auto 12864/b3",
        pair("tiled_pair", "64,64,64,64", 0, "16,16,16,16", 512, 512, "1024,1024"): "auto/f32 6464/auto 6464/f32 12864/f32",
        pair("tiled_pair", "64,64,64,64", 1, "16,16,16,16", 512, 512, "1024,1024"): "6464/b3",
        pair("tiled_pair", "64,32,64,32", 0, "32,16,32,16", 1024, 1024, "1024,1024"): "6432/auto 6432/f32",
        pair("tiled_pair", "64,32,64,32", 1, "32,16,32,16", 1024, 1024, "1024,1024"): "6432/b3",
        two((32, 32, 1, 0, 1024), (32, 32, 1, 0, 1024)): "3232/auto 3232/f32",
        two((32, 32, 1, 1, 1024), (32, 32, 1, 1, 1024)): "3232/b3",
        two((128, 64, 1, 1, 1024), (128, 64, 1, 1, 1024)): "split",
    },
    "linear_bwd 1024x1024x1024 nb1": {
        pair("big_pair", "128,64,128,64", 1, "16,8,16,8", 128, 128, "1024,1024", 1): "auto/auto auto/b3 12864/auto 12864/b3",
        pair("tiled_pair", "64,32,64,32", 0, "32,16,32,16", 512, 512, "1024,1024"): "auto/f32 6432/auto 6432/f32 12864/f32",
        pair("tiled_pair", "64,64,64,64", 0, "16,16,16,16", 256, 256, "1024,1024"): "6464/auto 6464/f32",
        pair("tiled_pair", "64,64,64,64", 1, "16,16,16,16", 256, 256, "1024,1024"): "6464/b3",
        pair("tiled_pair", "64,32,64,32", 1, "32,16,32,16", 512, 512, "1024,1024"): "6432/b3",
        two((32, 32, 1, 0, 1024), (32, 32, 1, 0, 1024)): "3232/auto 3232/f32",
        two((32, 32, 1, 1, 1024), (32, 32, 1, 1, 1024)): "3232/b3",
        two((64, 32, 1, 0, 1024), (64, 32, 1, 0, 1024)): "split",
    },
    # (with the mask that test_linear_bwd_pair_launch passes, the data gradient is no small-output product)
    "linear_bwd 512x1024x54 nb2": {
        two(SMALL, (32, 32, 0, 0, 1024)): "auto/auto auto/f32 auto/b3 3232/auto 3232/f32 3232/b3 12864/auto 12864/f32 12864/b3 split",
        two(SMALL, (64, 64, 0, 0, 1024)): "6464/auto 6464/f32 6464/b3",
        two(SMALL, (64, 32, 0, 0, 1024)): "6432/auto 6432/f32 6432/b3",
    },
    "linear_bwd 512x1024x54 nb2 no mask": {
        pair("small_pair", "16,16,16,16", 0, "4,64,4,32", 512, 256, "0,0"): ALL,
        two(SMALL, SMALL): "split",
    },
    "linear_bwd 512x1024x50 nb1": {
        two(SMALL, (32, 32, 0, 0, 1024)): "auto/auto auto/f32 auto/b3 3232/auto 3232/f32 3232/b3 12864/auto 12864/f32 12864/b3 split",
        two(SMALL, (64, 64, 0, 0, 1024)): "6464/auto 6464/f32 6464/b3",
        two(SMALL, (64, 32, 0, 0, 1024)): "6432/auto 6432/f32 6432/b3",
    },
    "linear_bwd 512x1024x50 nb1 no mask": {
        pair("small_pair", "16,16,16,16", 0, "4,64,4,32", 256, 128, "0,0"): ALL,
        two(SMALL, SMALL): "split",
    },
    "linear_bwd 96x40x24 nb1": {
        two((64, 64, 0, 0, 96), (64, 64, 0, 0, 64)):
            "auto/auto auto/f32 auto/b3 6464/auto 6464/f32 6464/b3 12864/auto 12864/f32 12864/b3 split",
        two((64, 32, 0, 0, 96), (64, 32, 0, 0, 64)): "6432/auto 6432/f32 6432/b3",
        two((32, 32, 0, 0, 96), (32, 32, 0, 0, 64)): "3232/auto 3232/f32 3232/b3",
    },
    "linear_bwd 256x1024x1024 nb2": {
        pair("big_pair", "128,64,128,64", 1, "16,8,16,2", 256, 64, "256,1024", 1): "auto/auto auto/b3 12864/auto 12864/b3",
        two((64, 64, 1, 0, 256), (32, 32, 1, 0, 1024)): "auto/f32 12864/f32",
        pair("tiled_pair", "64,64,64,64", 0, "16,16,16,4", 512, 128, "256,1024"): "6464/auto 6464/f32",
        pair("tiled_pair", "64,64,64,64", 1, "16,16,16,4", 512, 128, "256,1024"): "6464/b3",
        pair("tiled_pair", "64,32,64,32", 0, "32,16,32,4", 1024, 256, "256,1024"): "6432/auto 6432/f32",
        pair("tiled_pair", "64,32,64,32", 1, "32,16,32,4", 1024, 256, "256,1024"): "6432/b3",
        two((32, 32, 1, 0, 256), (32, 32, 1, 0, 1024)): "3232/auto 3232/f32",
        two((32, 32, 1, 1, 256), (32, 32, 1, 1, 1024)): "3232/b3",
        two((128, 64, 1, 1, 256), (32, 32, 1, 0, 1024)): "split",
    },
    "fc fwd splitk32": {
        g(64, 32, 1, 0, 992): "auto/auto auto/f32 6432/auto 6432/f32 12864/auto 12864/f32",
        g(64, 32, 1, 1, 992): "auto/b3 6432/b3 12864/b3",
        g(64, 64, 1, 0, 992): "6464/auto 6464/f32",
        g(64, 64, 1, 1, 992): "6464/b3",
        g(32, 32, 1, 0, 992): "3232/auto 3232/f32",
        g(32, 32, 1, 1, 992): "3232/b3",
    },
    "fc fwd splitk32 x3": {
        g(64, 64, 1, 0, 992): "auto/auto auto/f32 6464/auto 6464/f32 12864/auto 12864/f32",
        g(64, 64, 1, 1, 992): "auto/b3 6464/b3 12864/b3",
        g(64, 32, 1, 0, 992): "6432/auto 6432/f32",
        g(64, 32, 1, 1, 992): "6432/b3",
        g(32, 32, 1, 0, 992): "3232/auto 3232/f32",
        g(32, 32, 1, 1, 992): "3232/b3",
    },
    "fc dW M50": {
        g(64, 64, 0, 0, 512): "auto/auto auto/f32 auto/b3 6464/auto 6464/f32 6464/b3 12864/auto 12864/f32 12864/b3",
        g(64, 32, 0, 0, 512): "6432/auto 6432/f32 6432/b3",
        g(32, 32, 0, 0, 512): "3232/auto 3232/f32 3232/b3",
    },
    "gemm 8x50x2240 ak0 bk0 nb1": {
        g(64, 32, 1, 0, 2240): "auto/auto auto/f32 6432/auto 6432/f32 12864/auto 12864/f32",
        g(64, 32, 1, 1, 2240): "auto/b3 6432/b3 12864/b3",
        g(64, 64, 1, 0, 2240): "6464/auto 6464/f32",
        g(64, 64, 1, 1, 2240): "6464/b3",
        g(32, 32, 1, 0, 2240): "3232/auto 3232/f32",
        g(32, 32, 1, 1, 2240): "3232/b3",
    },
    "gemm 70x64x50 ak0 bk0 nb1": {
        g(32, 32, 0, 0, 64): "auto/auto auto/f32 auto/b3 3232/auto 3232/f32 3232/b3 12864/auto 12864/f32 12864/b3",
        g(64, 64, 0, 0, 64): "6464/auto 6464/f32 6464/b3",
        g(64, 32, 0, 0, 64): "6432/auto 6432/f32 6432/b3",
    },
    "gemm 512x1024x52 ak0 bk0 nb2": {
        g(64, 32, 0, 0, 64): "auto/auto auto/f32 auto/b3 6432/auto 6432/f32 6432/b3 12864/auto 12864/f32 12864/b3",
        g(64, 64, 0, 0, 64): "6464/auto 6464/f32 6464/b3",
        g(32, 32, 0, 0, 64): "3232/auto 3232/f32 3232/b3",
    },
    "gemm 33x17x129 ak0 bk1 nb1": {
        g(64, 64, 0, 0, 160): "auto/auto auto/f32 auto/b3 6464/auto 6464/f32 6464/b3 12864/auto 12864/f32 12864/b3",
        g(64, 32, 0, 0, 160): "6432/auto 6432/f32 6432/b3",
        g(32, 32, 0, 0, 160): "3232/auto 3232/f32 3232/b3",
    },
    "gemm 50x301x64 ak1 bk1 nb1": {
        g(32, 32, 0, 0, 64): "auto/auto auto/f32 auto/b3 3232/auto 3232/f32 3232/b3 12864/auto 12864/f32 12864/b3",
        g(64, 64, 0, 0, 64): "6464/auto 6464/f32 6464/b3",
        g(64, 32, 0, 0, 64): "6432/auto 6432/f32 6432/b3",
    },
    "gemm 64x52x100 ak1 bk1 nb2": {
        g(32, 32, 0, 0, 128): "auto/auto auto/f32 auto/b3 3232/auto 3232/f32 3232/b3 12864/auto 12864/f32 12864/b3",
        g(64, 64, 0, 0, 128): "6464/auto 6464/f32 6464/b3",
        g(64, 32, 0, 0, 128): "6432/auto 6432/f32 6432/b3",
    },
    "gemm 5x4x64 ak0 bk0 nb1": {
        g(64, 64, 1, 0, 64): "auto/auto auto/f32 6464/auto 6464/f32 12864/auto 12864/f32",
        g(64, 64, 1, 1, 64): "auto/b3 6464/b3 12864/b3",
        g(64, 32, 1, 0, 64): "6432/auto 6432/f32",
        g(64, 32, 1, 1, 64): "6432/b3",
        g(32, 32, 1, 0, 64): "3232/auto 3232/f32",
        g(32, 32, 1, 1, 64): "3232/b3",
    },
    "gemm 128x128x128 ak0 bk1 nb2": {
        g(32, 32, 1, 0, 128): "auto/auto auto/f32 3232/auto 3232/f32 12864/f32",
        g(32, 32, 1, 1, 128): "auto/b3 3232/b3",
        g(64, 64, 1, 0, 128): "6464/auto 6464/f32",
        g(64, 64, 1, 1, 128): "6464/b3",
        g(64, 32, 1, 0, 128): "6432/auto 6432/f32",
        g(64, 32, 1, 1, 128): "6432/b3",
        g(128, 64, 1, 1, 128): "12864/auto 12864/b3",
    },
    "gemm 1x64x50 ak0 bk0 nb1": {
        g(64, 32, 0, 0, 64): "auto/auto auto/f32 auto/b3 6432/auto 6432/f32 6432/b3 12864/auto 12864/f32 12864/b3",
        g(64, 64, 0, 0, 64): "6464/auto 6464/f32 6464/b3",
        g(32, 32, 0, 0, 64): "3232/auto 3232/f32 3232/b3",
    },
}


def expected_lines():
    table = {}
    for name, by_line in EXPECTED.items():
        for line, settings in by_line.items():
            for s in settings.split():
                assert f"{name} [{s}]" not in table
                table[f"{name} [{s}]"] = line
    return table


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gemm_plan") / "gemm_plan_probe")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", CSRC, PROBE, "-o", exe])
    return exe


def test_plan_header_is_host_only_code():
    """gemm_plan.h through the probe, which includes nothing else of the library: plain C++17, no warnings, nothing from
    ROCm on the include path; and it asks neither the options nor the device anything itself."""
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", CSRC, PROBE], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr
    with open(os.path.join(CSRC, "gemm_plan.h")) as f:
        code = "\n".join(ln.split("//")[0] for ln in f.read().splitlines())
    for word in ("hip", "curla_opt", "curla_cu_count"):
        assert word not in code.replace("curla_hip.h", ""), word


def test_plans_match_the_recorded_table(probe):
    cases = tuples()
    want = expected_lines()
    assert sorted(want) == sorted({n for n, _ in cases})  # every named product under every setting, nothing else
    r = subprocess.run([probe], input="\n".join(t for _, t in cases) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = r.stdout.splitlines()
    assert len(got) == len(cases)
    wrong = [(n, g, want[n]) for (n, _), g in zip(cases, got) if g != want[n]]
    assert not wrong, "\n".join(f"{n}:\n  got  {g}\n  want {w}" for n, g, w in wrong[:10])
