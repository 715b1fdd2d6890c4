"""The shapes of the encoder fc kernel tests, in one place: tests/test_gpu_fc_edges.py runs them on the GPU and
tests/test_fc_plan_host.py proves on the CPU, through the host-only plan (csrc/fc_plan.h), which kernel instantiation
and which walk each of them reaches -- and that, taken together, they reach all of them.  No torch, no GPU here."""

MFMAS = ("auto", "f32")  # option gemm_mfma: the bf16x3 form and the f32-input form of the fc forward
MFMA_INDEX = {"auto": 0, "f32": 1, "b3": 2}  # option values in the order of options.h
LAYOUTS = (False, True)  # x of the forward: row-major and blocked, every forward case in both
DX_MASKS = (True, False)  # curla_fc_dx with and without the ReLU mask, every fc_dx case with both

# ------------------------------------------------------------------------------------------------------- forward
# (B, F, K, nprob, nsplit); every case runs under both gemm_mfma values and in both x layouts.  K / 32 slices cut into
# nsplit splits: one split of 1, 2, 3, 4, 5, 9 slices (each skip pattern of the last chunk, one chunk only, a partly
# used last chunk, three chunks); 11 slices in 3 splits (3 + 4 + 4: splits that start off a chunk boundary); 13 slices
# in 13 splits (nsplit == K / 32); 37 slices in 5 splits (7 and 8: two chunks, the second partly / wholly used).
FWD_CASES = (
    (128, 50, 32, 1, 1), (128, 52, 64, 2, 1), (256, 54, 96, 3, 1), (128, 58, 128, 4, 1), (128, 62, 160, 1, 1),
    (128, 64, 288, 2, 1), (128, 50, 64, 2, 1), (128, 50, 96, 1, 1), (256, 50, 128, 1, 1), (128, 50, 160, 4, 1),
    (128, 50, 288, 3, 1), (256, 50, 352, 2, 3), (128, 54, 352, 1, 3), (128, 50, 416, 1, 13), (128, 64, 416, 1, 13),
    (128, 52, 1184, 1, 5), (128, 50, 1184, 1, 5),
)
# the chain test (fc forward -> LayerNorm forward -> LayerNorm backward -> fc backward) under both gemm_mfma values
CHAIN_CASES = ((128, 50, 96, 1, 1), (128, 52, 96, 1, 1))

# ---------------------------------------------------------------------------------------- the separate backward kernels
# K: a single float4 in the only block; whole blocks; a last block of one float4; a last block one float4 short
BWD_KS = (4, 64, 68, 252)
_DX_FS = (1, 4, 5, 16, 17, 32, 33, 52, 53, 64)     # both sides of 16/17, 32/33, 52/53 (fc_dx_kernel<4 | 8 | 13 | 16>)
_DX_BS = (1, 3, 16, 17, 67, 130, 200)              # 1, 1, 1, 2, 5, 9 and 13 b-tiles
# (B, F, K); every case runs with and without the mask
DX_CASES = tuple((_DX_BS[(3 * i + 2 * j) % 7], F, K) for i, F in enumerate(_DX_FS) for j, K in enumerate(BWD_KS)) + \
    ((130, 52, 196), (200, 64, 196))

_DW_FS = (7, 16, 17, 24, 32, 33, 48, 50, 64)       # fc_dw_kernel<1 | 2 | 3 | 4>
# k-steps per wave (least, most): 1: 0, 1; 5: 0, 1; 13: 1, 1; 30, 32: 2, 2; 36: 2, 3; 116: 7, 8; 130, 131: 8, 9; 260: 16, 17
_DW_BS = (1, 5, 13, 30, 32, 36, 116, 130, 131, 260)
# (B, F, K).  F = 50 takes fc_dw_kernel<4> only where B is no multiple of 16 (else: the one-pass kernel's weight-gradient
# half, ONE_PASS_CASES): 32 rows become 36 there.
DW_CASES = tuple((36 if F == 50 and _DW_BS[(3 * i + j) % 10] % 16 == 0 else _DW_BS[(3 * i + j) % 10], F, K)
                 for i, F in enumerate(_DW_FS) for j, K in enumerate(BWD_KS)) + \
    ((260, 50, 68), (131, 50, 196), (32, 64, 196), (116, 7, 64), (1, 33, 4))

# ------------------------------------------------------------------------------------------- the one-pass backward
# b-tiles per wave (least, most): 16: 0, 1; 48: 0, 1; 64: 1, 1; 80: 1, 2; 128: 2, 2; 144: 2, 3; 192: 3, 3; 208: 3, 4
_OP_BS = (16, 48, 64, 80, 128, 144, 192, 208)
# (B, F, K): curla_fc_bwd (fc_bwd_kernel<13, 3, 2, true> at F = 50, <13, 4, 0, true> at 49, 51, 52) and, at F = 50,
# curla_fc_dw too (fc_bwd_kernel<13, 3, 2, false>)
ONE_PASS_CASES = tuple((_OP_BS[(3 * i + 2 * j + (i == 1)) % 8], F, K)
                       for i, F in enumerate((49, 50, 51, 52)) for j, K in enumerate(BWD_KS)) + \
    ((16, 50, 196), (80, 50, 64), (144, 50, 68), (208, 50, 252), (192, 50, 4), (128, 51, 196), (208, 49, 64),
     (144, 52, 4))
# (B, F, K): the deferred LayerNorm sums ride along (one workgroup more); these are ONE_PASS_CASES too
ONE_PASS_LN_CASES = ((16, 50, 196), (80, 50, 64), (208, 50, 252), (128, 51, 196), (208, 49, 64), (144, 52, 4))
# (B, F, K, parts, len): curla_fc_bwd_ln2, a second set of [parts][len] partial sums for the same workgroup
LN2_CASES = ((16, 50, 196, 3, 50 * 50), (208, 49, 64, 8, 49 * 49), (80, 50, 64, 17, 50 * 50), (144, 52, 4, 17, 49 * 49))

# (B, F, K): curla_fc_bwd outside the one-pass kernel (F outside 49..52, or B % 16 != 0) takes the two launches;
# (24, 50, ...) and (40, 50, ...): curla_fc_dw at F = 50 with B % 16 != 0 takes fc_dw_kernel<4>
FALLBACK_CASES = ((32, 48, 68), (32, 53, 64), (24, 50, 196), (40, 51, 64), (17, 13, 4), (40, 50, 252), (64, 64, 64))

# ------------------------------------------------------------------------------------------------------ refusals
# curla_fc_fwd_multi: (why, B, F, K, nprob, nsplit, split stride - B F); all others of the shape are in range
FWD_REFUSALS = (("F odd", 128, 51, 64, 1, 1, 0), ("F below 50", 128, 48, 64, 1, 1, 0), ("F above 64", 128, 66, 64, 1, 1, 0),
                ("B % 128 != 0", 64, 50, 64, 1, 1, 0), ("K % 32 != 0", 128, 50, 80, 1, 1, 0),
                ("nsplit above K / 32", 128, 50, 64, 1, 3, 0), ("odd split stride", 128, 50, 64, 1, 2, 1))
# the backward entry points (each of curla_fc_dx, curla_fc_dw, curla_fc_bwd): (why, B, F, K)
BWD_REFUSALS = (("F above 64", 16, 65, 64), ("K % 4 != 0", 16, 50, 66))

# ------------------------------------------------------------------------------------ LayerNorm forward from partials
LN_NSPLITS = (1, 7, 8, 9, 16, 19)   # below, at and above the 8-wide partial loop, two rounds of it, two rounds + a tail
LN_BS = (3, 5, 128)                 # fewer than a block's four rows; a second, partly filled block; whole blocks
LN_FS = (50, 64)


def probe_line(entry, B, F, K, nprob=1, nsplit=1, split_stride=None, mfma="auto", ln=0):
    """the input line of tests/capi/fc_plan_probe.cpp"""
    stride = B * F if split_stride is None else split_stride
    return f"{entry} {B} {F} {K} {nprob} {nsplit} {stride} {MFMA_INDEX[mfma]} {ln}"


def plan_cases():
    """(name, probe input line, 'run' | 'refuse') of every launch shape of the GPU module, in the order of the lists"""
    out = []
    for B, F, K, nprob, ns in FWD_CASES:
        for m in MFMAS:
            out.append((f"fwd {B}x{F}x{K} np{nprob} ns{ns} [{m}]", probe_line("fwd", B, F, K, nprob, ns, mfma=m), "run"))
    for B, F, K in DX_CASES:
        out.append((f"dx {B}x{F}x{K}", probe_line("dx", B, F, K), "run"))
    for B, F, K in DW_CASES:
        out.append((f"dw {B}x{F}x{K}", probe_line("dw", B, F, K), "run"))
    for B, F, K in ONE_PASS_CASES:
        out.append((f"bwd {B}x{F}x{K}", probe_line("bwd", B, F, K), "run"))
        if F == 50:
            out.append((f"dw {B}x{F}x{K}", probe_line("dw", B, F, K), "run"))
    for B, F, K in ONE_PASS_LN_CASES:
        out.append((f"bwd {B}x{F}x{K} ln", probe_line("bwd", B, F, K, ln=1), "run"))
        if F == 50:
            out.append((f"dw {B}x{F}x{K} ln", probe_line("dw", B, F, K, ln=1), "run"))
    for B, F, K, _parts, _len in LN2_CASES:
        out.append((f"bwd {B}x{F}x{K} ln2", probe_line("bwd", B, F, K, ln=1), "run"))
    for B, F, K in FALLBACK_CASES:
        out.append((f"bwd {B}x{F}x{K} fallback", probe_line("bwd", B, F, K), "run"))
        out.append((f"dw {B}x{F}x{K} fallback", probe_line("dw", B, F, K), "run"))
    for B, F, K, nprob, ns in CHAIN_CASES:
        for m in MFMAS:
            out.append((f"fwd {B}x{F}x{K} chain [{m}]", probe_line("fwd", B, F, K, nprob, ns, mfma=m), "run"))
        out.append((f"bwd {B}x{F}x{K} chain", probe_line("bwd", B, F, K, ln=1), "run"))
    for why, B, F, K, nprob, ns, extra in FWD_REFUSALS:
        out.append((f"fwd refused: {why}", probe_line("fwd", B, F, K, nprob, ns, split_stride=B * F + extra), "refuse"))
    for why, B, F, K in BWD_REFUSALS:
        for entry in ("dx", "dw", "bwd"):
            out.append((f"{entry} refused: {why}", probe_line(entry, B, F, K), "refuse"))
    return out
