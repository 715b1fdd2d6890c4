"""The encoder fc kernels (csrc/fc_fwd.h, fc_bwd.h with the deferred LayerNorm sums, and the LayerNorm forward of
csrc/layernorm.h that adds up the split-K partials) at every instantiation and walk regime of their plan
(csrc/fc_plan.h), against float64, inside guards.

The shapes come from tests/_fc_cases.py; tests/test_fc_plan_host.py proves on the CPU that they reach every
instantiation, every walk regime (b-tiles per wave, k-steps per wave, slices per split and the skip pattern of a split's
last chunk, the last 64-column block), every fallback and every refusal, and that none of them is refused by surprise.
Every tensor a kernel reads or writes sits between NaN guard bands (a read that the range check or the clamp does not
cover shows as a NaN in the result), outputs start as NaN, the guards are asserted after every launch, every launch is
repeated and must give the same bits, and the float64 references are tests/_fc_ref.py.  Random operands have a seed
of their own each.

Bars (none is new): the fc forward's splits and their sum 2e-6, in both arithmetics (the f32 form is held to the bf16x3
form's bar); the one-pass dW 2e-5 in both forms (the weight-gradient half alone is held to the whole kernel's bar); the
deferred LayerNorm sums and the second set of partials 2e-5 against float64 sums of the partials; everything else
tests/_util.RTOL.  The chain test compares with autograd in float64 from the inputs on, so every kernel's output there
carries the rounding of the kernels in front of it: RTOL.

Worst errors measured on an MI355X over these lists (all bars inherited, none set from a measurement): forward splits and
sums 5.5e-7 (bf16x3) and 7.1e-7 (f32) against 2e-6; one-pass dW 1.6e-7 in both forms against 2e-5; deferred LayerNorm
sums 3.5e-7 and the second set of partials 1.3e-7 against 2e-5; fc_dx and the one-pass dx 3.4e-7, fc_dw_kernel 1.7e-7,
the LayerNorm forward 2.8e-7, the chain 5.7e-7 (y) and 3.2e-7 (gradients) against RTOL = 1e-4."""
import functools

import pytest
import torch

from tests._conv_ref import NAN, _same_bits, guarded
from tests._fc_cases import (BWD_REFUSALS, CHAIN_CASES, DW_CASES, DX_CASES, DX_MASKS, FALLBACK_CASES, FWD_CASES,
                             FWD_REFUSALS, LAYOUTS, LN2_CASES, LN_BS, LN_FS, LN_NSPLITS, MFMAS, ONE_PASS_CASES,
                             ONE_PASS_LN_CASES)
from tests._fc_ref import d, dw_ref, dx_ref, fwd_ref, ln_fwd_ref, split_ranges
from tests._util import RTOL
# (fixtures of the kernel tests; _report, autouse, writes what `check` measured in this module into the kernel tests'
# parity report when the module ends)
from tests.test_gpu_kernels import _report, check, ops, rnd  # noqa: F401

pytestmark = pytest.mark.gpu

FWD_TOL = 2e-6   # fc forward: every split and the sum of the splits
DW1_TOL = 2e-5   # one-pass weight gradient, both forms
SUMS_TOL = 2e-5  # deferred LayerNorm sums and the second set of partials against float64 sums of the partials


# ------------------------------------------------------------------------------------------------------- plumbing
def put(*tensors, shifts=None):
    """every tensor inside its own NaN guards on the device (``shifts``: floats past a 16-byte boundary, per tensor):
    (the views, a function that asserts every guard intact)"""
    pairs = [guarded(data=t, shift=(shifts[i] if shifts else 0)) for i, t in enumerate(tensors)]

    def intact(what):
        for k, (_, ok) in enumerate(pairs):
            ok(f"{what} input {k}")
    return [v for v, _ in pairs], intact


def run_twice(launch, outs, name, ins=None, finite=True):
    """``launch()`` into the NaN-filled guarded outputs ``outs`` [(view, intact)], twice: written everywhere (finite),
    all guards intact (``ins``: the inputs' check), the second run bit-identical.  Returns the first run's results."""
    first = None
    for run in range(2):
        for v, _ in outs:
            v.fill_(NAN)
        launch()
        now = [v.clone() for v, _ in outs]
        for k, ((_, intact), t) in enumerate(zip(outs, now)):
            assert not finite or bool(torch.isfinite(t).all()), f"{name}: output {k} is not finite / not written everywhere"
            intact(f"{name} output {k}, run {run}")
        if ins is not None:
            ins(f"{name}, run {run}")
        if first is None:
            first = now
        else:
            for k, (a, b) in enumerate(zip(first, now)):
                assert _same_bits(a, b), f"{name}: output {k} differs between two runs"
    return first


def refused(ops, launch, outs, name):
    """``launch()`` raises CurlaHipError and leaves the NaN-filled guarded outputs and their guards untouched"""
    from curla_amd._lib import CurlaHipError
    for v, _ in outs:
        v.fill_(NAN)
    with pytest.raises(CurlaHipError):
        launch()
    torch.cuda.synchronize()
    for k, (v, intact) in enumerate(outs):
        assert bool(torch.isnan(v).all()), f"{name}: a refused call wrote output {k}"
        intact(f"{name} output {k}")


def relu_out(*shape, seed):
    """a ReLU output (exact +0.0 where it is off) with every fifth element -0.0 instead: the mask is > 0"""
    act = torch.relu(rnd(*shape, seed=seed))
    act.view(-1)[::5] = -0.0
    assert bool((act.view(-1)[::5] == 0).all()) and bool(torch.signbit(act.view(-1)[::5]).all())
    return act


def mfma_option(value):
    from curla_amd import _lib
    return _lib.option("gemm_mfma", value)


# ------------------------------------------------------------------------------------- inputs and float64 references
# (computed once per case, shared by the tests that run it, never written to)
@functools.lru_cache(maxsize=None)
def fwd_case(B, F, K, nprob, ns):
    """xs, Ws, per problem the float64 product of every split's k range, and the whole product"""
    xs = [rnd(B, K, seed=201 + i) for i in range(nprob)]
    Ws = [rnd(F, K, seed=211 + i, scale=0.05) for i in range(nprob)]
    parts = [[fwd_ref(x, W, k0, k1) for k0, k1 in split_ranges(K, ns)] for x, W in zip(xs, Ws)]
    return xs, Ws, parts, [fwd_ref(x, W) for x, W in zip(xs, Ws)]


@functools.lru_cache(maxsize=None)
def bwd_case(B, F, K):
    """dz [B, F], W [F, K], x [B, K] (a ReLU output: the mask of dx and the operand of dW), dx and dW in float64"""
    dz, W, x = rnd(B, F, seed=301), rnd(F, K, seed=302, scale=0.1), relu_out(B, K, seed=303)
    return dz, W, x, dx_ref(dz, W, x), dx_ref(dz, W), dw_ref(dz, x)


def run_fwd(ops, xs, Ws, B, F, K, ns, mfma, blocked, name, finite=True):
    """curla_fc_fwd_multi on CPU operands: the partials [ns, B, F] of every problem.  The partials of the odd problems
    start 8 bytes past a 16-byte boundary (all the kernel asks for)."""
    xin, x_ok = put(*[ops.to_blocked(x, B, K) if blocked else x for x in xs])
    Win, w_ok = put(*Ws)
    outs = [guarded((ns, B, F), shift=2 * (i % 2)) for i in range(len(xs))]

    def ins(what):
        x_ok(what + " x"), w_ok(what + " W")
    with mfma_option(mfma):
        return run_twice(lambda: ops.fc_fwd_multi(xin, Win, [o for o, _ in outs], B, F, K, ns, B * F, blocked=blocked),
                         outs, name, ins, finite)


# ------------------------------------------------------------------------------------------------ 1. forward splits
@pytest.mark.parametrize("B,F,K,nprob,ns", FWD_CASES)
def test_forward_splits(ops, B, F, K, nprob, ns):
    """every split of every problem against the float64 product over its k range, the sum of the splits against the
    whole product, in both arithmetics; the blocked layout gives the bits of the row-major one; and the two arithmetics
    differ somewhere (the option was taken)"""
    xs, Ws, parts, whole = fwd_case(B, F, K, nprob, ns)
    got = {}
    for mfma in MFMAS:
        for blocked in LAYOUTS:
            got[mfma, blocked] = run_fwd(ops, xs, Ws, B, F, K, ns, mfma, blocked,
                                         f"fc_fwd [{mfma}{' blocked' if blocked else ''}] {B}x{F}x{K} np{nprob} ns{ns}")
    for mfma in MFMAS:
        for i in range(nprob):
            P = got[mfma, False][i]
            assert _same_bits(P, got[mfma, True][i]), f"problem {i}: the blocked layout gives other bits [{mfma}]"
            for s in range(ns):
                check(f"fc_fwd [{mfma}] {B}x{F}x{K} np{nprob} p{i} split {s}/{ns}", P[s].cpu(), parts[i][s], FWD_TOL)
            check(f"fc_fwd [{mfma}] {B}x{F}x{K} np{nprob} p{i} sum of {ns}", P.double().sum(0).cpu(), whole[i], FWD_TOL)
    assert any(not _same_bits(a, b) for a, b in zip(got["auto", False], got["f32", False])), \
        "gemm_mfma = auto and = f32 give the same bits: the option was not taken"


# -------------------------------------------------------------------------------------- 2. separate backward kernels
@pytest.mark.parametrize("B,F,K", DX_CASES)
def test_data_gradient(ops, B, F, K):
    dz, W, x, ref_masked, ref_plain, _ = bwd_case(B, F, K)
    (ddz, dW_, dmask), ins = put(dz, W, x, shifts=(1, 0, 0))
    out = guarded((B, K))
    for with_mask in DX_MASKS:
        name = f"fc_dx{' masked' if with_mask else ''} {B}x{F}x{K}"
        got, = run_twice(lambda: ops.fc_dx(ddz, dW_, out[0], B, F, K, mask=dmask if with_mask else None), [out], name, ins)
        check(name, got.cpu(), ref_masked if with_mask else ref_plain)


@pytest.mark.parametrize("B,F,K", DW_CASES)
def test_weight_gradient(ops, B, F, K):
    dz, _, x, _, _, ref = bwd_case(B, F, K)
    (ddz, dx_), ins = put(dz, x, shifts=(1, 0))
    out = guarded((F, K))
    got, = run_twice(lambda: ops.fc_dw(ddz, dx_, out[0], B, F, K), [out], f"fc_dw {B}x{F}x{K}", ins)
    check(f"fc_dw {B}x{F}x{K}", got.cpu(), ref)


# ------------------------------------------------------------------------------------ 3. one-pass backward, both forms
@pytest.mark.parametrize("B,F,K", ONE_PASS_CASES)
def test_one_pass_backward(ops, B, F, K):
    """dx and dW of curla_fc_bwd and (F = 50) dW of curla_fc_dw, which takes the weight-gradient half of the same kernel,
    against float64; dx bit-identical to curla_fc_dx"""
    dz, W, x, ref_dx, _, ref_dw = bwd_case(B, F, K)
    (ddz, dW_, dx_), ins = put(dz, W, x, shifts=(1, 0, 0))
    gx, gw = guarded((B, K)), guarded((F, K))
    got_dx, got_dw = run_twice(lambda: ops.fc_bwd(ddz, dW_, dx_, gx[0], gw[0], B, F, K), [gx, gw], f"fc_bwd {B}x{F}x{K}", ins)
    check(f"fc_bwd dx {B}x{F}x{K}", got_dx.cpu(), ref_dx)
    check(f"fc_bwd dW {B}x{F}x{K}", got_dw.cpu(), ref_dw, DW1_TOL)
    sep, = run_twice(lambda: ops.fc_dx(ddz, dW_, gx[0], B, F, K, mask=dx_), [gx], f"fc_dx {B}x{F}x{K}", ins)
    assert _same_bits(got_dx, sep), "the one-pass dx is not curla_fc_dx's"
    if F == 50:
        half, = run_twice(lambda: ops.fc_dw(ddz, dx_, gw[0], B, F, K), [gw], f"fc_dw (one-pass half) {B}x{F}x{K}", ins)
        check(f"fc_dw (one-pass half) dW {B}x{F}x{K}", half.cpu(), ref_dw, DW1_TOL)


def deferred_ln(ops, B, F):
    """ops.ln_bwd(..., defer=) on random inputs: (dz on the device, 4 bytes past a 16-byte boundary; the token; the
    guarded dgamma, dbeta, dbias; the float64 sums [3, F] of the partials it left; a check of the partials' guards)"""
    gamma = (1 + 0.1 * rnd(F, seed=311)).cuda()
    xhat, rstd, dy = rnd(B, F, seed=312).cuda(), (0.5 + rnd(B, seed=313).abs()).cuda(), rnd(B, F, seed=314).cuda()
    dz, part = guarded((B, F), shift=1), guarded((ops.ln_partial_floats(B, F),), shift=1)
    sums = [guarded((F,)) for _ in range(3)]
    tok = ops.ln_bwd(dy, xhat, rstd, gamma, B, F, dz[0], dgamma=sums[0][0], dbeta=sums[1][0], dbias_in=sums[2][0],
                     defer=part[0])
    n = tok[1]
    assert n == (B + 3) // 4 and bool(torch.isfinite(part[0]).all()) and bool(torch.isfinite(dz[0]).all())
    dz[1]("ln_bwd dz"), part[1]("ln_bwd partials")
    return dz[0], tok, sums, part[0].view(n, 3, F).double().sum(0).cpu(), part[1]


def check_sums(name, got, want):
    for k, what in enumerate(("dgamma", "dbeta", "fc dbias")):
        check(f"{name} deferred {what}", got[k].cpu(), want[k], SUMS_TOL)


@pytest.mark.parametrize("B,F,K", ONE_PASS_LN_CASES)
def test_one_pass_backward_finishes_the_layernorm_sums(ops, B, F, K):
    """the extra workgroup: dgamma, dbeta and the fc bias gradient against float64 sums of the partials, and the fc
    products bit-identical with and without it -- for curla_fc_bwd_ln and (F = 50) curla_fc_dw_ln"""
    _, W, x, _, _, _ = bwd_case(B, F, K)
    dz, tok, sums, want, part_ok = deferred_ln(ops, B, F)
    (dW_, dx_), ins_ok = put(W, x)

    def ins(what):
        ins_ok(what), part_ok(what + " partials")
    gx, gw = guarded((B, K)), guarded((F, K))
    name = f"fc_bwd_ln {B}x{F}x{K}"
    dx0, dw0 = run_twice(lambda: ops.fc_bwd(dz, dW_, dx_, gx[0], gw[0], B, F, K), [gx, gw], name + " (without)", ins)
    check(f"{name} dx", dx0.cpu(), dx_ref(dz, W, x))
    check(f"{name} dW", dw0.cpu(), dw_ref(dz, x), DW1_TOL)
    dx1, dw1, *got = run_twice(lambda: ops.fc_bwd(dz, dW_, dx_, gx[0], gw[0], B, F, K, ln=tok), [gx, gw] + sums, name, ins)
    assert _same_bits(dx0, dx1) and _same_bits(dw0, dw1), "the LnReduce workgroup changes the fc products"
    check_sums(name, got, want)
    if F == 50:
        name = f"fc_dw_ln {B}x{F}x{K}"
        dw2, = run_twice(lambda: ops.fc_dw(dz, dx_, gw[0], B, F, K), [gw], name + " (without)", ins)
        check(f"{name} dW", dw2.cpu(), dw_ref(dz, x), DW1_TOL)
        dw3, *got = run_twice(lambda: ops.fc_dw(dz, dx_, gw[0], B, F, K, ln=tok), [gw] + sums, name, ins)
        assert _same_bits(dw2, dw3), "the LnReduce workgroup changes the weight gradient"
        check_sums(name, got, want)


@pytest.mark.parametrize("B,F,K,parts,length", LN2_CASES)
def test_one_pass_backward_second_set_of_partials(ops, B, F, K, parts, length):
    """curla_fc_bwd_ln2: a random [parts][len] tensor as the CURL head's dW partials -- its float64 sum, the LayerNorm
    sums, and the fc products unchanged"""
    _, W, x, _, _, _ = bwd_case(B, F, K)
    dz, tok, sums, want, part_ok = deferred_ln(ops, B, F)
    xpart = rnd(parts, length, seed=321)
    (dW_, dx_, dxpart), ins_ok = put(W, x, xpart, shifts=(0, 0, 1))

    def ins(what):
        ins_ok(what), part_ok(what + " partials")
    gx, gw, xout = guarded((B, K)), guarded((F, K)), guarded((length,), shift=1)
    name = f"fc_bwd_ln2 {B}x{F}x{K} parts {parts} len {length}"
    dx0, dw0 = run_twice(lambda: ops.fc_bwd(dz, dW_, dx_, gx[0], gw[0], B, F, K), [gx, gw], name + " (without)", ins)
    tok2 = tok + (dxpart, parts, length, xout[0])
    dx1, dw1, xo, *got = run_twice(lambda: ops.fc_bwd(dz, dW_, dx_, gx[0], gw[0], B, F, K, ln=tok2), [gx, gw, xout] + sums,
                                   name, ins)
    assert _same_bits(dx0, dx1) and _same_bits(dw0, dw1), "the LnReduce workgroup changes the fc products"
    check(f"{name} second sums", xo.cpu(), d(xpart).sum(0), SUMS_TOL)
    check_sums(name, got, want)


# --------------------------------------------------------------------------------------------------- 4. fallbacks
@pytest.mark.parametrize("B,F,K", FALLBACK_CASES)
def test_fallback_is_the_two_launches(ops, B, F, K):
    dz, W, x, ref_dx, _, ref_dw = bwd_case(B, F, K)
    (ddz, dW_, dx_), ins = put(dz, W, x, shifts=(1, 0, 0))
    gx, gw = guarded((B, K)), guarded((F, K))
    name = f"fc_bwd fallback {B}x{F}x{K}"
    got_dx, got_dw = run_twice(lambda: ops.fc_bwd(ddz, dW_, dx_, gx[0], gw[0], B, F, K), [gx, gw], name, ins)
    sep_dx, = run_twice(lambda: ops.fc_dx(ddz, dW_, gx[0], B, F, K, mask=dx_), [gx], name + " fc_dx", ins)
    sep_dw, = run_twice(lambda: ops.fc_dw(ddz, dx_, gw[0], B, F, K), [gw], name + " fc_dw", ins)
    assert _same_bits(got_dx, sep_dx) and _same_bits(got_dw, sep_dw)
    check(f"{name} dx", got_dx.cpu(), ref_dx)
    check(f"{name} dW", got_dw.cpu(), ref_dw)


# --------------------------------------------------------------------------------------------------- 5. refusals
@pytest.mark.parametrize("why,B,F,K,nprob,ns,extra", FWD_REFUSALS)
def test_forward_refusals(ops, why, B, F, K, nprob, ns, extra):
    stride = B * F + extra
    (x, W), _ = put(rnd(B, K, seed=331), rnd(F, K, seed=332))
    out = guarded((ns * stride,), shift=2)
    for mfma in MFMAS:
        with mfma_option(mfma):
            refused(ops, lambda: ops.fc_fwd_multi([x], [W], [out[0]], B, F, K, ns, stride), [out], f"fc_fwd refused: {why}")


@pytest.mark.parametrize("why,B,F,K", BWD_REFUSALS)
def test_backward_refusals(ops, why, B, F, K):
    (dz, W, x), _ = put(rnd(B, F, seed=333), rnd(F, K, seed=334), relu_out(B, K, seed=335))
    gx, gw = guarded((B, K)), guarded((F, K))
    refused(ops, lambda: ops.fc_dx(dz, W, gx[0], B, F, K, mask=x), [gx], f"fc_dx refused: {why}")
    refused(ops, lambda: ops.fc_dx(dz, W, gx[0], B, F, K), [gx], f"fc_dx refused: {why}")
    refused(ops, lambda: ops.fc_dw(dz, x, gw[0], B, F, K), [gw], f"fc_dw refused: {why}")
    refused(ops, lambda: ops.fc_bwd(dz, W, x, gx[0], gw[0], B, F, K), [gx, gw], f"fc_bwd refused: {why}")


def test_misaligned_operands_are_refused(ops):
    """x or W one float past a 16-byte boundary, a partial buffer one float past an 8-byte boundary; the backward's W,
    x / mask, dx and dW one float past a 16-byte boundary"""
    B, F, K = 128, 50, 64
    xc, Wc = rnd(B, K, seed=336), rnd(F, K, seed=337)
    (x, W, x1, W1), _ = put(xc, Wc, xc, Wc, shifts=(0, 0, 1, 1))
    out, out1 = guarded((B, F), shift=2), guarded((B, F), shift=1)
    for xs, Ws, o in ((x1, W, out), (x, W1, out), (x, W, out1)):
        refused(ops, lambda: ops.fc_fwd_multi([xs], [Ws], [o[0]], B, F, K, 1, B * F), [o], "fc_fwd misaligned")
    run_twice(lambda: ops.fc_fwd_multi([x], [W], [out[0]], B, F, K, 1, B * F), [out], "fc_fwd aligned")  # (the same call, aligned)
    B = 16
    dzc, mc = rnd(B, F, seed=338), relu_out(B, K, seed=339)
    (dz, W, m, W1, m1), _ = put(dzc, Wc, mc, Wc, mc, shifts=(1, 0, 0, 1, 1))
    gx, gw, gx1, gw1 = guarded((B, K)), guarded((F, K)), guarded((B, K), shift=1), guarded((F, K), shift=1)
    for Ws, ms, o in ((W1, m, gx), (W, m1, gx), (W, m, gx1)):
        refused(ops, lambda: ops.fc_dx(dz, Ws, o[0], B, F, K, mask=ms), [o], "fc_dx misaligned")
    for ms, o in ((m1, gw), (m, gw1)):
        refused(ops, lambda: ops.fc_dw(dz, ms, o[0], B, F, K), [o], "fc_dw misaligned")
    for Ws, ms, ox, ow in ((W1, m, gx, gw), (W, m1, gx, gw), (W, m, gx1, gw), (W, m, gx, gw1)):
        refused(ops, lambda: ops.fc_bwd(dz, Ws, ms, ox[0], ow[0], B, F, K), [ox, ow], "fc_bwd misaligned")
    run_twice(lambda: ops.fc_bwd(dz, W, m, gx[0], gw[0], B, F, K), [gx, gw], "fc_bwd aligned")


# --------------------------------------------------------------------------- 6. non-finite rows stay where they belong
def nan_rows(B):
    """the first row, the last row, the last row of the first b-tile"""
    return sorted({0, B - 1, min(15, B - 1)})


def assert_only_row(clean, dirty, b0, where, name):
    """``dirty`` [B, n] is ``clean`` bit for bit except row b0, which is NaN where ``where`` [n] (or all of it) says and
    the clean bits elsewhere"""
    keep = torch.ones(clean.shape[0], dtype=torch.bool)
    keep[b0] = False
    assert _same_bits(clean[keep], dirty[keep]), f"{name}: the NaN of row {b0} reached another row"
    where = torch.ones(clean.shape[1], dtype=torch.bool) if where is None else where.cpu()
    row, crow = dirty[b0].cpu(), clean[b0].cpu()
    assert bool(torch.isnan(row[where]).all()), f"{name}: row {b0} is not NaN everywhere it should be"
    assert _same_bits(row[~where], crow[~where]), f"{name}: row {b0} changed where the NaN has no say"


@pytest.mark.parametrize("B,F,K,entry", [(67, 52, 68, "dx"), (200, 16, 68, "dx"), (80, 50, 64, "bwd"), (144, 52, 68, "bwd"),
                                         (208, 49, 64, "bwd")])
def test_a_nan_row_of_dz_stays_in_its_row_of_dx(ops, B, F, K, entry):
    """(shapes of DX_CASES, one of them ragged in B and K, and of ONE_PASS_CASES)"""
    assert (B, F, K) in (DX_CASES if entry == "dx" else ONE_PASS_CASES)
    dz, W, x, _, _, _ = bwd_case(B, F, K)
    gx, gw = guarded((B, K)), guarded((F, K))

    def launch(ddz, dW_, dx_):
        if entry == "dx":
            return lambda: ops.fc_dx(ddz, dW_, gx[0], B, F, K, mask=dx_)
        return lambda: ops.fc_bwd(ddz, dW_, dx_, gx[0], gw[0], B, F, K)
    outs = [gx] if entry == "dx" else [gx, gw]
    ins, ok = put(dz, W, x, shifts=(1, 0, 0))
    clean = run_twice(launch(*ins), outs, f"fc_{entry} clean {B}x{F}x{K}", ok)
    for b0 in nan_rows(B):
        bad = dz.clone()
        bad[b0] = NAN
        ins, ok = put(bad, W, x, shifts=(1, 0, 0))
        name = f"fc_{entry} {B}x{F}x{K} NaN in dz row {b0}"
        dirty = run_twice(launch(*ins), outs, name, ok, finite=False)
        assert_only_row(clean[0], dirty[0], b0, x[b0] > 0, name)  # (masked off: exactly 0, as in the clean run)
        assert bool((dirty[0][b0].cpu()[~(x[b0] > 0)] == 0).all())
        if entry == "bwd":  # dW sums over the rows: NaN everywhere, and only inside the tensor (the guards: run_twice)
            assert bool(torch.isnan(dirty[1]).all()), f"{name}: dW is not NaN everywhere"


@pytest.mark.parametrize("B,F,K", [(131, 33, 252), (36, 50, 252), (260, 17, 252), (144, 50, 68)])
def test_a_nan_row_of_dz_fills_dw_and_nothing_else(ops, B, F, K):
    """(shapes of DW_CASES -- ragged B -- and, the last, of ONE_PASS_CASES: the weight-gradient half of the one-pass kernel)"""
    assert (B, F, K) in DW_CASES + ONE_PASS_CASES
    dz, _, x, _, _, _ = bwd_case(B, F, K)
    gw = guarded((F, K))
    for b0 in nan_rows(B):
        bad = dz.clone()
        bad[b0] = NAN
        (ddz, dx_), ok = put(bad, x, shifts=(1, 0))
        name = f"fc_dw {B}x{F}x{K} NaN in dz row {b0}"
        got, = run_twice(lambda: ops.fc_dw(ddz, dx_, gw[0], B, F, K), [gw], name, ok, finite=False)
        assert bool(torch.isnan(got).all()), f"{name}: dW is not NaN everywhere"


@pytest.mark.parametrize("B,F,K,nprob,ns", [(256, 50, 352, 2, 3), (128, 54, 352, 1, 3)])
def test_a_nan_of_x_stays_in_its_row_and_its_splits(ops, B, F, K, nprob, ns):
    """one NaN at x[b0][k0] of the first problem: row b0 of the split that covers k0 is NaN, nothing else changes -- in
    both arithmetics and both layouts"""
    assert (B, F, K, nprob, ns) in FWD_CASES
    xs, Ws, _, _ = fwd_case(B, F, K, nprob, ns)
    ranges = split_ranges(K, ns)
    for mfma in MFMAS:
        for blocked in LAYOUTS:
            tag = f"[{mfma}{' blocked' if blocked else ''}] {B}x{F}x{K}"
            clean = run_fwd(ops, xs, Ws, B, F, K, ns, mfma, blocked, f"fc_fwd clean {tag}")
            for n, b0 in enumerate(nan_rows(B)):
                hit = (n + 1) % ns                      # the split that gets the NaN: another one per row
                k0 = ranges[hit][0] + (5 + 9 * n) % (ranges[hit][1] - ranges[hit][0])
                bad = xs[0].clone()
                bad[b0, k0] = NAN
                name = f"fc_fwd {tag} NaN at x[{b0}][{k0}]"
                dirty = run_fwd(ops, [bad] + list(xs[1:]), Ws, B, F, K, ns, mfma, blocked, name, finite=False)
                for i in range(1, nprob):
                    assert _same_bits(clean[i], dirty[i]), f"{name}: another problem changed"
                for s in range(ns):
                    if s == hit:
                        assert_only_row(clean[0][s], dirty[0][s], b0, None, f"{name} split {s}")
                    else:
                        assert _same_bits(clean[0][s], dirty[0][s]), f"{name}: split {s} does not cover k0 and changed"


# ------------------------------------------------------------------------------- 7. LayerNorm forward from partials
def ln_job(ops, B, F, ns, ldp, seed, tanh_out, want):
    """one job of the LayerNorm forward: random partials [ns][B][ldp] (F of every ldp floats are read), parameters, the
    optional outputs named in ``want`` -- (the job's dict for fc_ln_fwd_multi, its guarded outputs by name, the float64
    reference by name, a check of the inputs' guards)"""
    P = rnd(ns, B, ldp, seed=seed)
    bias, gamma, beta = rnd(F, seed=seed + 1, scale=0.1), 1 + 0.1 * rnd(F, seed=seed + 2), rnd(F, seed=seed + 3, scale=0.1)
    act = rnd(B, 3, seed=seed + 4)
    (dP, dbias, dgamma, dbeta, dact), ins = put(P, bias, gamma, beta, act, shifts=(1, 1, 0, 3, 1))
    fc, y, xhat, rstd = ln_fwd_ref(P[:, :, :F], bias, gamma, beta, 1e-5, tanh_out)
    ref = {"y": y, "fc_out": fc, "xhat": xhat, "rstd": rstd, "xa": torch.cat([y, d(act)], 1)}
    shapes = {"y": (B, F), "fc_out": (B, F), "xhat": (B, F), "rstd": (B,), "xa": (B, F + 3)}
    outs = {n: guarded(shapes[n], shift=k % 4) for k, n in enumerate(["y"] + list(want))}
    job = dict(partial=dP, bias=dbias, gamma=dgamma, beta=dbeta, tanh_out=int(tanh_out), **{n: o for n, (o, _) in outs.items()})
    if "xa" in want:
        job["act"] = dact
    return job, outs, ref, ins


def run_single(ops, job, outs, B, F, ns, ldp, name, ins):
    kw = {k: v for k, v in job.items() if k not in ("partial", "bias", "gamma", "beta", "y")}
    names = list(outs)
    got = run_twice(lambda: ops.fc_ln_fwd(job["partial"], ns, B * ldp, ldp, job["bias"], job["gamma"], job["beta"], B, F,
                                          job["y"], **kw), [outs[n] for n in names], name, ins)
    return dict(zip(names, got))


@pytest.mark.parametrize("ns", LN_NSPLITS)
def test_layernorm_forward_from_partials(ops, ns):
    """ops.fc_ln_fwd over nsplit partials (the 8-wide loop: not at all, once, once + 1, twice, twice + 3), fewer rows
    than a block, a ragged last block, whole blocks; every optional output; tanh on and off; ldp > F once per nsplit"""
    for B in LN_BS:
        for F in LN_FS:
            ldp = F + 6 if (B, F) == (5, 50) else F
            tanh_out = (B + F // 2 + ns) % 2 == 1
            name = f"fc_ln_fwd ns{ns} {B}x{F} ldp{ldp}{' tanh' if tanh_out else ''}"
            job, outs, ref, ins = ln_job(ops, B, F, ns, ldp, 341, tanh_out, ("fc_out", "xhat", "rstd", "xa"))
            got = run_single(ops, job, outs, B, F, ns, ldp, name, ins)
            for n, t in got.items():
                check(f"{name} {n}", t.cpu(), ref[n])
            assert _same_bits(got["xa"][:, :F], got["y"]) and _same_bits(got["xa"][:, F:], job["act"])


@pytest.mark.parametrize("njobs", [2, 3, 4])
def test_layernorm_forward_several_jobs(ops, njobs):
    """ops.fc_ln_fwd_multi: tanh_out and the optional outputs differ from job to job; each job bit-identical to its own
    single-job launch and held to float64"""
    wants = (("fc_out", "xhat", "rstd", "xa"), (), ("xhat", "rstd"), ("fc_out", "xa"))[:njobs]
    for B, F, ns in ((5, 50, 9), (128, 64, 19), (3, 50, 8)):
        made = [ln_job(ops, B, F, ns, F, 351 + 10 * i, i % 2 == 1, wants[i]) for i in range(njobs)]
        flat = [(i, n, o) for i, (_, outs, _, _) in enumerate(made) for n, o in outs.items()]

        def ins(what):
            for _, _, _, ok in made:
                ok(what)
        name = f"fc_ln_fwd_multi {njobs} jobs ns{ns} {B}x{F}"
        got = run_twice(lambda: ops.fc_ln_fwd_multi([j for j, _, _, _ in made], ns, B * F, F, B, F, 1e-5, 3),
                        [o for _, _, o in flat], name, ins)
        multi = {(i, n): t for (i, n, _), t in zip(flat, got)}
        for i, (job, outs, ref, ok) in enumerate(made):
            single = run_single(ops, job, outs, B, F, ns, F, f"{name} job {i} alone", ok)
            for n, t in single.items():
                assert _same_bits(t, multi[i, n]), f"{name}: job {i} {n} differs from its single-job launch"
                check(f"{name} job {i} {n}", multi[i, n].cpu(), ref[n])


# ----------------------------------------------------------------------------------------------------- 8. the chain
@pytest.mark.parametrize("mfma", MFMAS)
@pytest.mark.parametrize("B,F,K,nprob,ns", CHAIN_CASES)
def test_the_chain_against_autograd(ops, B, F, K, nprob, ns, mfma):
    """fc_fwd_multi -> fc_ln_fwd (tanh on and off) -> ln_bwd(defer=) -> fc_bwd(ln=) against autograd in float64 through
    tanh(layer_norm(relu(h) W^T + b)) and the same without the tanh; the tanh's own backward is applied on the host"""
    h, W = rnd(B, K, seed=361), rnd(F, K, seed=362, scale=0.05)
    bias, gamma, beta = rnd(F, seed=363, scale=0.1), 1 + 0.1 * rnd(F, seed=364), rnd(F, seed=365, scale=0.1)
    gy = rnd(B, F, seed=366)
    x = torch.relu(h)
    (dx_, dW_, dbias, dgamma, dbeta), ins = put(x, W, bias, gamma, beta)
    P = guarded((ns, B, F), shift=2)
    with mfma_option(mfma):
        run_twice(lambda: ops.fc_fwd_multi([dx_], [dW_], [P[0]], B, F, K, ns, B * F), [P], f"chain fc_fwd [{mfma}]", ins)
    for tanh_out in (True, False):
        name = f"chain [{mfma}] {B}x{F}x{K}{' tanh' if tanh_out else ''}"
        leaf = [t.double().requires_grad_() for t in (h, W, bias, gamma, beta)]
        z = torch.nn.functional.layer_norm(torch.relu(leaf[0]) @ leaf[1].t() + leaf[2], (F,), leaf[3], leaf[4], 1e-5)
        yref = torch.tanh(z) if tanh_out else z
        yref.backward(gy.double())
        y, xhat, rstd = guarded((B, F)), guarded((B, F)), guarded((B,))
        gotf = run_twice(lambda: ops.fc_ln_fwd(P[0], ns, B * F, F, dbias, dgamma, dbeta, B, F, y[0], xhat=xhat[0],
                                               rstd=rstd[0], tanh_out=int(tanh_out)), [y, xhat, rstd], name + " fc_ln_fwd", ins)
        check(f"{name} y", gotf[0].cpu(), yref.detach())
        dy = gy.cuda() * (1 - gotf[0] * gotf[0]) if tanh_out else gy.cuda()
        dz, part = guarded((B, F)), guarded((ops.ln_partial_floats(B, F),))
        sums = [guarded((F,)) for _ in range(3)]
        tok = ops.ln_bwd(dy, xhat[0], rstd[0], dgamma, B, F, dz[0], dgamma=sums[0][0], dbeta=sums[1][0],
                         dbias_in=sums[2][0], defer=part[0])
        dz[1](name + " dz"), part[1](name + " partials")
        gx, gw = guarded((B, K)), guarded((F, K))
        got_dx, got_dw, dg, db, dbi = run_twice(lambda: ops.fc_bwd(dz[0], dW_, dx_, gx[0], gw[0], B, F, K, ln=tok),
                                                [gx, gw] + sums, name + " fc_bwd", ins)
        for what, got, ref in (("dx", got_dx, leaf[0].grad), ("dW", got_dw, leaf[1].grad), ("fc dbias", dbi, leaf[2].grad),
                               ("dgamma", dg, leaf[3].grad), ("dbeta", db, leaf[4].grad)):
            check(f"{name} {what}", got.cpu(), ref)
