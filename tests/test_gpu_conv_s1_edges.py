"""The stride-1 3x3 convolution kernels (csrc/conv_rw.h, conv_rw43.h, conv_rwb.h, conv_rw_wgrad.h, conv_rw_wgrad2.h and
the generic conv_generic.h) at every regime of their strip plan (csrc/conv_plan.h), against float64, inside guards.

The kernels walk whatever the host planner hands them -- full strips, remainder columns cut into segments, remainder
strips -- and rely on buffer range checks for everything outside the image.  The geometry lists below were chosen with
tests/capi/conv_plan_probe.cpp so that every regime of the plan occurs in them; tests/test_conv_plan_host.py proves that
on the CPU, for every form.  Every tensor a kernel writes sits between NaN guard bands and starts as NaN, every tensor it
reads sits between NaN guard bands too (a read the range check does not cover shows as a NaN in the result), the
weight-gradient workspace is NaN throughout, every comparison is with float64 at the project's RTOL, and every launch
is repeated and must give the same bits."""
import functools

import pytest
import torch

from tests._conv_ref import NAN, _same_bits, dgrad_ref, fwd_ref, guarded, wgrad_ref
# (fixtures of the kernel tests; _report, autouse, writes what `check` measured in this module into the kernel tests'
# parity report when the module ends)
from tests.test_gpu_kernels import _report, check, ops, rnd, s1_impl, s1_wgrad  # noqa: F401

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------------- the geometries
# (Ho, Wo) = the PLANNED extents of the operation (what conv_plan_probe takes): the forward's output (its input is
# Ho + 2 x Wo + 2), the data gradient's output gin (the gradient it reads is Ho - 2 x Wo - 2: 3 x 3 is the entry
# point's Ho = Wo = 1), the weight gradient's gradient extents (its input is Ho + 2 x Wo + 2).  The first four of every
# list are the fixed small shapes (1 x 1, 1 x N, N x 1, 2 x 2 -- of the gradient the data gradient reads); the next ones
# a greedy cover of the regime attributes of test_conv_plan_host.py over both plan forms; then the header's worked
# example, the largest tensor of the sweep, the tiny geometry of the batch tests and a few more parities and strips.
#
# What the hand-picked cases of test_gpu_kernels.py (test_conv_s1_fwd / _dgrad / _wgrad) never had, by the probe, and
# these lists have (per = 16 lane groups, the weight gradient 4):
#   forward, f23 / b3:   brem = 15; a remainder strip whose last strip is full; two or more remainder strips without a
#                        full strip; a single segment (nr == Ho)
#   forward, f43:        brem = 15; two or more remainder strips beside full strips; nr == Ho
#   data gradient, f23 / b3: an even height; brem = 0, 1 and 15 (only 3, 5, 8, 10 occurred); two or more remainder strips
#                        without a full strip; nr == 1, nr == Ho, equal segments (Ho % nr == 0)
#   data gradient, f43:  an even height; Wo mod 4 = 2; brem = 0, 1 and 15 (only 4, 5, 10, 11); two full strips; two or
#                        more remainder strips beside full strips; nr == Ho, equal segments
#   weight gradient, x:  two or more remainder strips without a full strip
#   weight gradient, xy: two or more remainder strips at all (with and without full strips); nr == 1
# and for every operation: outputs of 1 x 1, 1 x N, N x 1 and 2 x 2 (the forward and the weight gradient had 1 x 1).
FWD_GEOMS = ((1, 1), (1, 9), (9, 1), (2, 2), (16, 87), (2, 60), (14, 23), (1, 125), (1, 31),
             (35, 35), (38, 138), (3, 4), (7, 30), (6, 64), (11, 34), (13, 16), (5, 7), (8, 5), (21, 12))
DGRAD_GEOMS = ((3, 3), (3, 11), (11, 3), (4, 4), (32, 101), (3, 58), (9, 21), (3, 125), (3, 31), (3, 33),
               (35, 35), (40, 140), (5, 6), (8, 30), (6, 64), (14, 17), (7, 8), (12, 5), (10, 29), (9, 23))
WGRAD_GEOMS = ((1, 1), (1, 9), (9, 1), (2, 2), (7, 21), (7, 3), (1, 7), (3, 5), (7, 5),
               (33, 33), (38, 138), (3, 4), (6, 8), (12, 16), (5, 17), (10, 31), (33, 2))
TINY = (3, 4)  # output of the 5 x 6 input of the batch tests (forward / weight gradient); the data gradient's gin is 5 x 6
# the one-launch backward: gradient extents, each in WGRAD_GEOMS and (+ 2) in DGRAD_GEOMS at the same batch
BWD_GEOMS = ((1, 1), (1, 9), (7, 21), (33, 33))
FWD2_GEOMS = ((14, 23), (2, 60), (11, 34))
# the stack: forward outputs whose inputs have Hi, Wi >= 7 (three layers) and Hi * Wi <= 1000
STACK_GEOMS = ((14, 23), (7, 30), (6, 64), (11, 34), (13, 16), (5, 7), (8, 5), (21, 12))
# generic filter counts: forward outputs 1 x 1, 1 x N, N x 1, an odd and an even rectangle, and B Ho Wo below, at and
# above the 256 positions one pass of conv_wgrad_kernel's threads covers (B = 2: 2 x 7 x 9 = 126, 2 x 8 x 16 = 256,
# 2 x 9 x 15 = 270)
GENERIC_GEOMS = ((1, 1), (1, 6), (6, 1), (5, 7), (4, 6), (7, 9), (8, 16), (9, 15))


def batch_of(Ho, Wo):
    """2 or 3 samples"""
    return 2 + (Ho + Wo) % 2


# ------------------------------------------------------------------------------------- inputs and float64 references
# (computed once per case, shared by the forms and options that run it, never written to)
@functools.lru_cache(maxsize=None)
def weights(nf=32, seed=0):
    return rnd(nf, nf, 3, 3, seed=40 + seed, scale=0.1), rnd(nf, seed=50 + seed, scale=0.1)


@functools.lru_cache(maxsize=None)
def fwd_case(B, Ho, Wo, nf=32, seed=0):
    """x [B, Ho+2, Wo+2, nf], w, b and relu(conv2d) in float64"""
    x = rnd(B, Ho + 2, Wo + 2, nf, seed=1 + seed)
    w, b = weights(nf, seed)
    return x, w, b, fwd_ref(x, w, b)


@functools.lru_cache(maxsize=None)
def dgrad_case(B, Ho, Wo, nf=32):
    """g [B, Ho-2, Wo-2, nf], w, the activation below [B, Ho, Wo, nf] and the masked data gradient in float64.  The
    activation is a ReLU output (exact +0.0 where it is off); every fifth element is -0.0 instead: the mask is > 0."""
    g = rnd(B, Ho - 2, Wo - 2, nf, seed=4)
    w, _ = weights(nf)
    act = torch.relu(rnd(B, Ho, Wo, nf, seed=6))
    act.view(-1)[::5] = -0.0
    assert bool((act.view(-1)[::5] == 0).all()) and bool(torch.signbit(act.view(-1)[::5]).all())
    return g, w, act, dgrad_ref(g, w, act)


@functools.lru_cache(maxsize=None)
def wgrad_case(B, Ho, Wo, nf=32):
    """x [B, Ho+2, Wo+2, nf] (a ReLU output), g [B, Ho, Wo, nf] (ReLU-masked), dW and db in float64"""
    x = torch.relu(rnd(B, Ho + 2, Wo + 2, nf, seed=7))
    g = rnd(B, Ho, Wo, nf, seed=8) * (rnd(B, Ho, Wo, nf, seed=9) > 0)
    dw, db = wgrad_ref(x, g)
    return x, g, dw, db


def put(*tensors):
    """every tensor inside its own NaN guards on the device: the views"""
    return [guarded(data=t)[0] for t in tensors]


def run_twice(launch, outs, name):
    """``launch()`` into the NaN-filled guarded outputs ``outs`` [(view, intact)], twice: finite, guards intact, the
    second run bit-identical.  Returns the first run's results (clones)."""
    for v, _ in outs:
        v.fill_(NAN)
    launch()
    first = [v.clone() for v, _ in outs]
    for k, ((v, intact), f) in enumerate(zip(outs, first)):
        assert bool(torch.isfinite(f).all()), f"{name}: output {k} is not finite / not written everywhere"
        intact(f"{name} output {k}")
    for v, _ in outs:
        v.fill_(NAN)
    launch()
    for k, ((v, intact), f) in enumerate(zip(outs, first)):
        assert _same_bits(v, f), f"{name}: output {k} differs between two runs"
        intact(f"{name} output {k}, second run")
    return first


def run_fwd(ops, B, Ho, Wo, name, nf=32):
    x, w, b, ref = fwd_case(B, Ho, Wo, nf)
    dx, dw, db = put(x, w, b)
    out = guarded((B, Ho, Wo, nf))
    got, = run_twice(lambda: ops.conv_s1_fwd(dx, dw, db, out[0]), [out], name)
    check(name, got.cpu(), ref)
    return got


def run_dgrad(ops, B, Ho, Wo, name, nf=32):
    g, w, act, ref = dgrad_case(B, Ho, Wo, nf)
    dg, dw, dact = put(g, w, act)
    gin = guarded((B, Ho, Wo, nf))
    got, = run_twice(lambda: ops.conv_s1_dgrad(dg, dw, dact, gin[0]), [gin], name)
    check(name, got.cpu(), ref)
    return got


def poisoned_workspace(ops, nf=32):
    return torch.full((ops.wgrad_workspace_floats(nf),), NAN, device="cuda")


def check_slabs(ws, n, nf, dw_ref, db_ref, name):
    """the first n slabs [nf nf 9 | nf] written everywhere, nothing behind them touched, their float64 sum = dW | db"""
    slab = nf * nf * 9 + nf
    assert n * slab <= ws.numel()
    assert not bool(torch.isnan(ws[:n * slab]).any()), f"{name}: a slab was left (partly) unwritten"
    assert bool(torch.isnan(ws[n * slab:]).all()), f"{name}: a store behind the {n} slabs"
    total = ws[:n * slab].view(n, slab).double().sum(0).cpu()
    check(f"{name} dW", total[:nf * nf * 9].view(nf, nf, 3, 3), dw_ref)
    check(f"{name} db", total[nf * nf * 9:], db_ref)


def run_wgrad(ops, B, Ho, Wo, name, want_slabs, nf=32):
    x, g, dw_ref, db_ref = wgrad_case(B, Ho, Wo, nf)
    dx, dg = put(x, g)
    ws = poisoned_workspace(ops, nf)
    n = ops.conv_s1_wgrad_slabs(dx, dg, ws)
    assert n == want_slabs, (n, want_slabs)
    check_slabs(ws, n, nf, dw_ref, db_ref, f"{name} slabs")
    dw, db = guarded((nf, nf, 3, 3)), guarded((nf,))

    def launch():
        ws.fill_(NAN)  # (a kernel that accumulates into its slab, or reads one it did not write, meets NaN)
        ops.conv_s1_wgrad(dx, dg, dw[0], db[0], ws)
    got_dw, got_db = run_twice(launch, [dw, db], name)
    check(f"{name} dW", got_dw.cpu(), dw_ref)
    check(f"{name} db", got_db.cpu(), db_ref)


# ------------------------------------------------------------------------------------------------------- the sweeps
@pytest.mark.parametrize("Ho,Wo", FWD_GEOMS)
def test_forward_sweep(ops, s1_impl, Ho, Wo):
    B = batch_of(Ho, Wo)
    run_fwd(ops, B, Ho, Wo, f"s1 edges fwd [{s1_impl}] B{B} out {Ho}x{Wo}")


@pytest.mark.parametrize("Ho,Wo", DGRAD_GEOMS)
def test_data_gradient_sweep(ops, s1_impl, Ho, Wo):
    B = batch_of(Ho, Wo)
    run_dgrad(ops, B, Ho, Wo, f"s1 edges dgrad [{s1_impl}] B{B} gin {Ho}x{Wo}")


@pytest.mark.parametrize("Ho,Wo", WGRAD_GEOMS)
def test_weight_gradient_sweep(ops, s1_wgrad, Ho, Wo):
    B = batch_of(Ho, Wo)
    run_wgrad(ops, B, Ho, Wo, f"s1 edges wgrad [{s1_wgrad}] B{B} g {Ho}x{Wo}", min(B, 2 * ops.cu_count()))


# ------------------------------------------------------------------------------------------------ batch against grid
# Workgroups own samples k, k + n, ...: the uneven last round is where a stride or a bound goes wrong.  C = the CU
# count: the forward and the b3 / f43 data gradients launch min(B, C) workgroups, the f23 data gradient and the weight
# gradient min(B, 2 C).
@pytest.mark.parametrize("rounds", ["1", "C-1", "C+1", "2C+1", "4C+3"])
def test_forward_batch_against_grid(ops, s1_impl, rounds):
    C = ops.cu_count()
    B = {"1": 1, "C-1": C - 1, "C+1": C + 1, "2C+1": 2 * C + 1, "4C+3": 4 * C + 3}[rounds]
    run_fwd(ops, B, *TINY, f"s1 edges fwd [{s1_impl}] B = {rounds} = {B} in 5x6")


@pytest.mark.parametrize("rounds", ["1", "C-1", "C+1", "2C+1", "4C+3"])
def test_data_gradient_batch_against_grid(ops, s1_impl, rounds):
    C = ops.cu_count()
    B = {"1": 1, "C-1": C - 1, "C+1": C + 1, "2C+1": 2 * C + 1, "4C+3": 4 * C + 3}[rounds]
    run_dgrad(ops, B, 5, 6, f"s1 edges dgrad [{s1_impl}] B = {rounds} = {B} gin 5x6")


@pytest.mark.parametrize("rounds", ["1", "2C-1", "2C+1", "4C+3"])
def test_weight_gradient_batch_against_grid(ops, s1_wgrad, rounds):
    C = ops.cu_count()
    B = {"1": 1, "2C-1": 2 * C - 1, "2C+1": 2 * C + 1, "4C+3": 4 * C + 3}[rounds]
    run_wgrad(ops, B, *TINY, f"s1 edges wgrad [{s1_wgrad}] B = {rounds} = {B} in 5x6", min(B, 2 * C))


# ----------------------------------------------------------------------------------------------- sample independence
def _poisoned_sample(which, B, C):
    return {"first": 0, "last": B - 1, "second round": C}[which]


@pytest.mark.parametrize("which", ["first", "last", "second round"])
def test_forward_sample_independence(ops, s1_impl, which):
    """B = C + 2: one input sample all NaN -- its output holds NaN, every other sample's bits are those of the clean run"""
    C = ops.cu_count()
    B = C + 2
    s = _poisoned_sample(which, B, C)
    x, w, b, _ = fwd_case(B, *TINY)
    dx, dw, db = put(x, w, b)
    clean, bad = guarded((B,) + TINY + (32,)), guarded((B,) + TINY + (32,))
    ops.conv_s1_fwd(dx, dw, db, clean[0])
    dx[s] = NAN
    ops.conv_s1_fwd(dx, dw, db, bad[0])
    clean[1]("clean"), bad[1]("poisoned")
    assert bool(torch.isnan(bad[0][s]).any()), "the NaN sample's output holds no NaN"
    keep = [i for i in range(B) if i != s]
    assert _same_bits(bad[0][keep], clean[0][keep])
    assert bool(torch.isfinite(clean[0]).all())


@pytest.mark.parametrize("which", ["first", "last", "second round"])
def test_data_gradient_sample_independence(ops, s1_impl, which):
    C = ops.cu_count()
    B = C + 2
    s = _poisoned_sample(which, B, C)
    g, w, act, _ = dgrad_case(B, 5, 6)
    dg, dw, dact = put(g, w, act)
    clean, bad = guarded((B, 5, 6, 32)), guarded((B, 5, 6, 32))
    ops.conv_s1_dgrad(dg, dw, dact, clean[0])
    dg[s] = NAN
    ops.conv_s1_dgrad(dg, dw, dact, bad[0])
    clean[1]("clean"), bad[1]("poisoned")
    assert bool(torch.isnan(bad[0][s]).any()), "the NaN sample's output holds no NaN"
    keep = [i for i in range(B) if i != s]
    assert _same_bits(bad[0][keep], clean[0][keep])
    assert bool(torch.isfinite(clean[0]).all())


# ------------------------------------------------------------------------------------------- two problems, the stack
@pytest.mark.parametrize("Ho,Wo", FWD2_GEOMS)
@pytest.mark.parametrize("batches", ["1,C+1", "C+1,1", "3,2"])
def test_forward_two_problems(ops, s1_impl, batches, Ho, Wo):
    """conv_s1_fwd2: each problem's output bit-identical to its single launch, inside guards"""
    assert (Ho, Wo) in FWD_GEOMS
    C = ops.cu_count()
    B1, B2 = {"1,C+1": (1, C + 1), "C+1,1": (C + 1, 1), "3,2": (3, 2)}[batches]
    x1, w1, b1, _ = fwd_case(B1, Ho, Wo)
    x2, _, _, _ = fwd_case(B2, Ho, Wo, seed=1)
    w2, b2 = weights(32, 1)
    d1, d2 = put(x1, w1, b1), put(x2, w2, b2)
    r1, r2 = guarded((B1, Ho, Wo, 32)), guarded((B2, Ho, Wo, 32))
    ops.conv_s1_fwd(*d1, r1[0])
    ops.conv_s1_fwd(*d2, r2[0])
    o1, o2 = guarded((B1, Ho, Wo, 32)), guarded((B2, Ho, Wo, 32))
    ops.conv_s1_fwd2(*d1, o1[0], *d2, o2[0])
    for t, what in ((r1, "single 1"), (r2, "single 2"), (o1, "pair 1"), (o2, "pair 2")):
        t[1](what)
    assert bool(torch.isfinite(r1[0]).all()) and bool(torch.isfinite(r2[0]).all())
    assert _same_bits(o1[0], r1[0]) and _same_bits(o2[0], r2[0])


@pytest.mark.parametrize("Ho,Wo", STACK_GEOMS)
def test_forward_stack(ops, s1_impl, Ho, Wo):
    """conv_s1_fwd_stack, B = the granule, three layers from the sweep geometry's input: every layer bit-identical to
    the per-layer launches, inside guards"""
    assert (Ho, Wo) in FWD_GEOMS and Ho + 2 >= 7 and Wo + 2 >= 7 and (Ho + 2) * (Wo + 2) <= 1000
    B, L = ops.stack_granule(), 3
    x = guarded(data=torch.relu(rnd(B, Ho + 2, Wo + 2, 32, seed=101)))[0]
    ws = put(*[rnd(32, 32, 3, 3, seed=110 + i, scale=0.1) for i in range(L)])
    bs = put(*[rnd(32, seed=130 + i, scale=0.1) for i in range(L)])
    mk = lambda: [guarded((B, Ho - 2 * i, Wo - 2 * i, 32)) for i in range(L)]  # noqa: E731
    r, o = mk(), mk()
    for i in range(L):
        ops.conv_s1_fwd(x if i == 0 else r[i - 1][0], ws[i], bs[i], r[i][0])
    assert ops.conv_s1_fwd_stack(x, ws, bs, [t[0] for t in o])
    for i in range(L):
        r[i][1](f"layer {i}, single"), o[i][1](f"layer {i}, stack")
        assert bool(torch.isfinite(r[i][0]).all()), i
        assert _same_bits(o[i][0], r[i][0]), i


# -------------------------------------------------------------------------------------------- backward in one launch
@pytest.mark.parametrize("Ho,Wo,rounds", [g + ("sweep",) for g in BWD_GEOMS] + [TINY + ("2C+1",)])
@pytest.mark.parametrize("split", ["0", "1"])
def test_backward_one_launch(ops, s1_impl, s1_wgrad, split, Ho, Wo, rounds):
    """conv_s1_bwd_slabs under bwd_split: gin bit-identical to the stand-alone data gradient (which the sweep / the batch
    test above hold to float64 at this very case), the documented number of slabs, their sum against float64, a rerun"""
    from curla_amd import _lib
    C = ops.cu_count()
    B = batch_of(Ho, Wo) if rounds == "sweep" else 2 * C + 1
    assert ((Ho, Wo) in WGRAD_GEOMS and (Ho + 2, Wo + 2) in DGRAD_GEOMS) if rounds == "sweep" else (Ho + 2, Wo + 2) == (5, 6)
    # the layer: input x = the activation below (its ReLU mask), output gradient g
    g, w, act, _ = dgrad_case(B, Ho + 2, Wo + 2)
    dw_ref, db_ref = _bwd_wgrad_ref(B, Ho, Wo)
    dg, dw, dx = put(g, w, act)
    alone = guarded((B, Ho + 2, Wo + 2, 32))
    ops.conv_s1_dgrad(dg, dw, dx, alone[0])
    gin = guarded((B, Ho + 2, Wo + 2, 32))
    ws = poisoned_workspace(ops)
    name = f"s1 edges bwd_slabs [{s1_impl}/{s1_wgrad}/split {split}] B{B} g {Ho}x{Wo}"
    with _lib.option("bwd_split", split):
        # (f43: two launches, the weight gradient's own grid; else one or two workgroups of each kind per CU)
        want = min(B, 2 * C) if s1_impl == "f43" else min(B, (1 if split == "1" else 2) * C)
        n = [0]

        def launch():
            ws.fill_(NAN)
            n[0] = ops.conv_s1_bwd_slabs(dx, dg, dw, gin[0], ws)
        got, = run_twice(launch, [gin], name)
        assert n[0] == want, (n[0], want)
        alone[1]("stand-alone dgrad")
        assert _same_bits(got, alone[0])
        check_slabs(ws, n[0], 32, dw_ref, db_ref, name)
        first = ws[:n[0] * (32 * 288 + 32)].clone()
        launch()
        assert _same_bits(ws[:first.numel()], first), "the slabs differ between two runs"


@functools.lru_cache(maxsize=None)
def _bwd_wgrad_ref(B, Ho, Wo):
    g, _, act, _ = dgrad_case(B, Ho + 2, Wo + 2)
    return wgrad_ref(act, g)


# ---------------------------------------------------------------------------------------------- generic filter counts
@pytest.mark.parametrize("Ho,Wo", GENERIC_GEOMS)
@pytest.mark.parametrize("nf", [8, 16, 64])
def test_generic_filter_counts(ops, nf, Ho, Wo):
    """num_filters != 32 (conv_generic.h): forward, data gradient, weight gradient (one slab) and the one-call backward
    with the same guards, NaN workspace and float64 references"""
    B = 2
    tag = f"nf{nf} B{B} out {Ho}x{Wo}"
    run_fwd(ops, B, Ho, Wo, f"s1 edges generic fwd {tag}", nf)
    run_dgrad(ops, B, Ho + 2, Wo + 2, f"s1 edges generic dgrad {tag}", nf)
    run_wgrad(ops, B, Ho, Wo, f"s1 edges generic wgrad {tag}", 1, nf)
    g, w, act, ref = dgrad_case(B, Ho + 2, Wo + 2, nf)
    dw_ref, db_ref = wgrad_ref(act, g)
    dg, dw, dx = put(g, w, act)
    gin = guarded((B, Ho + 2, Wo + 2, nf))
    ws = poisoned_workspace(ops, nf)
    n = [0]

    def launch():
        ws.fill_(NAN)
        n[0] = ops.conv_s1_bwd_slabs(dx, dg, dw, gin[0], ws)
    got, = run_twice(launch, [gin], f"s1 edges generic bwd_slabs {tag}")
    assert n[0] == 1
    check(f"s1 edges generic bwd_slabs gin {tag}", got.cpu(), ref)
    check_slabs(ws, 1, nf, dw_ref, db_ref, f"s1 edges generic bwd_slabs {tag}")


@pytest.mark.parametrize("nf", [8, 16, 64])
def test_generic_forward_sample_independence(ops, nf):
    """the generic forward's ReLU keeps a NaN too: the NaN sample stays NaN, the other sample keeps its bits"""
    B = 2
    x, w, b, _ = fwd_case(B, *TINY, nf)
    dx, dw, db = put(x, w, b)
    clean, bad = guarded((B,) + TINY + (nf,)), guarded((B,) + TINY + (nf,))
    ops.conv_s1_fwd(dx, dw, db, clean[0])
    dx[1] = NAN
    ops.conv_s1_fwd(dx, dw, db, bad[0])
    clean[1]("clean"), bad[1]("poisoned")
    assert bool(torch.isnan(bad[0][1]).any()), "the NaN sample's output holds no NaN"
    assert _same_bits(bad[0][0], clean[0][0]) and bool(torch.isfinite(clean[0]).all())
