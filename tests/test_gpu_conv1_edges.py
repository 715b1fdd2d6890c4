"""The first-layer conv kernels (3x3, stride 2, C -> 32: csrc/conv1_u8_rw.h, conv1_rw.h, conv1_band.h, conv1_wgrad.h,
conv1_dgrad.h) at every regime of their plans (csrc/conv1_plan.h), against float64, inside guards.

The geometry lists below were chosen with tests/capi/conv_plan_probe.cpp so that every regime of the plans occurs in
them -- per operation, source and form; tests/test_conv1_plan_host.py proves that on the CPU.  Every float tensor a
kernel reads or writes sits between NaN guard bands, outputs and the weight-gradient workspace start as NaN, every
comparison is with float64 at the project's RTOL, and every launch is repeated and must give the same bits.  The uint8
ring has no NaN bytes: its runs are repeated with the 32 readable bytes behind the ring flipped and with every byte no
sample reads complemented, and must give the same bits again.

NaN semantics: a NaN weight or bias (either sign bit) makes its output channel NaN and leaves every other channel's bits
alone; a NaN (or Inf) pixel of a float source reaches exactly the outputs whose window holds it."""
import functools

import numpy as np
import pytest
import torch

from tests._conv_ref import NAN, _same_bits, conv1_dgrad_ref, conv1_fwd_ref, conv1_wgrad_ref, crop_ref, guarded
from tests.test_gpu_conv_s1_edges import put, run_twice
# (fixtures of the kernel tests; _report, autouse, writes what `check` measured in this module into the kernel tests'
# parity report when the module ends)
from tests.test_gpu_kernels import _report, check, ops, rnd  # noqa: F401

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------------- the geometries
# (C, Hc, Wc) = channels and crop of the observation; the output is (Hc - 3) // 2 + 1 x (Wc - 3) // 2 + 1 x 32.  Each
# list is a greedy cover of the regime attributes of tests/test_conv1_plan_host.py over every form that runs it,
# smallest crops first.  The weight-gradient lists carry the band count of their banded forms as a fourth entry (the
# slab count the launch must report follows from it; the host test checks it against the plan).
#
# What the hand-picked CONV1_CASES (and the two conv1_fwd2 shapes) of test_gpu_kernels.py never ran, by the probe, and
# these lists do:
#   every operation:          output rows of 1, of 2..7 and of more than 128 pixels
#   uint8 forward, banded:    two full bands; three or more bands (last one full, short, one row); a first staging pass of
#                             exactly 7 x 512 runs; a band of fewer than 8 tiles whose pixels are a multiple of 16
#   row walks (uint8 rw, rwb, hybrid; float NHWC rw; 16 lane groups): one and 15 remainder columns; a full last remainder
#                             strip; a single segment (nr == Ho); an output of one row
#   hybrid:                   everything the option hands to the banded kernel beyond a crop of one band
#   float forward, banded:    a second band at all (full, short, one row) and three or more
#   uint8 weight gradient:    rows of 7 and 8 pixels (the bf16 form's limit), two full bands, three or more bands, the
#                             C = 9 tail column at rows of 1, 2..7 and > 128 pixels, the bf16 form above 128
#   float weight gradient:    row walk (4 lane groups): no full strip and exactly one, a partly filled last remainder
#                             strip, nr == 1, nr == Ho, several remainder strips without a full one; banded: two bands
#                             (full, one row), three or more
U8_FWD_GEOMS = ((3, 7, 19), (6, 6, 64), (9, 96, 3), (12, 3, 34), (3, 3, 260), (3, 145, 5), (3, 7, 51), (9, 3, 115), (9, 3, 130),
                (6, 3, 230), (6, 3, 290), (9, 27, 235), (12, 7, 682), (3, 159, 155), (9, 145, 57), (12, 39, 310), (9, 68, 245),
                (12, 166, 310))
F32_FWD_GEOMS = ((3, 7, 19), (6, 9, 50), (9, 4, 3), (3, 40, 14), (12, 3, 33), (3, 3, 290), (3, 5, 31), (3, 7, 51), (3, 159, 39),
                 (3, 89, 71), (9, 61, 35), (9, 19, 168), (9, 11, 310), (12, 21, 125))
U8_WGRAD_GEOMS = ((9, 3, 15, 1), (3, 5, 18, 1), (6, 4, 3, 1), (12, 4, 34, 1), (3, 13, 39, 1), (3, 3, 290, 1), (9, 3, 3, 1),
                  (9, 3, 33, 1), (9, 3, 17, 1), (12, 3, 17, 1), (9, 3, 35, 1), (12, 3, 35, 1), (9, 3, 260, 1), (12, 3, 260, 1),
                  (3, 159, 155, 2), (9, 145, 57, 2), (12, 39, 310, 3), (9, 68, 245, 3), (12, 166, 310, 10))
F32_WGRAD_GEOMS = ((3, 9, 7, 1), (6, 3, 20, 1), (9, 34, 3, 1), (3, 16, 38, 1), (12, 3, 33, 1), (3, 3, 290, 1), (3, 5, 15, 1),
                   (3, 9, 15, 1), (3, 168, 75, 2), (3, 180, 70, 2), (9, 61, 70, 2), (12, 7, 676, 3), (9, 168, 41, 3),
                   (12, 19, 295, 3))
# (C, H, W) of the observation gradient: 3 x 3, even and odd extents, every C, more than one 256-thread block
DGRAD_GEOMS = ((3, 3, 3), (3, 4, 4), (6, 7, 10), (9, 17, 19), (12, 12, 9), (9, 40, 35))
# two minibatches in one launch: (C, Hc, Wc) of U8_FWD_GEOMS, 3 + 2 samples; the first minibatch's steps end inside a
# wave's share (in both row walks, by the host test), so a wave's piece ends in the first problem and its next begins in
# the second
FWD2_GEOMS = ((3, 3, 260), (6, 3, 230), (9, 68, 245))
# NaN semantics: one geometry per C, odd and even widths, crops wide enough for an interior column
NAN_GEOMS = ((3, 9, 11), (6, 8, 13), (9, 11, 10), (12, 7, 9))
# the uint8 row walks' unrolled rotation (15 steps): one strip of 16 columns, 34 rows, whole frames of 8 ring slots
WRAP_GEOM = (3, 69, 33)
WRAP_SLOTS = 8
# bands from WIDE rows: 300 x 12 bytes a row leave ten rows of LDS to a band -- two bands of 6 and 5 output rows
WIDE_GEOM = (12, 23, 300)

U8_FORMS = ("hybrid", "band", "rw", "rwb")          # option conv1_u8
F32_SOURCES = ("nchw band", "nhwc rw", "nhwc band")  # source and option conv1_f32 (NCHW has the banded form only)
U8_WGRAD_FORMS = ("f32", "b16")                     # option wgrad1_u8
N_SLOTS = 5
POS_NAN, NEG_NAN = 0x7FC00000, 0xFFC00000 - (1 << 32)  # (as int32)


def out_hw(Hc, Wc):
    return (Hc - 3) // 2 + 1, (Wc - 3) // 2 + 1


def batch_of(Hc, Wc):
    """2 or 3 samples"""
    return 2 + (Hc + Wc) % 2


def ring_of(C, Hc, Wc):
    """(slots, Hs, Ws) of the ring a crop is cut from: two rows and one to three columns larger, so that row pitches
    Ws C of every residue mod 4 occur (the uint8 walks load aligned dwords where it is 0)"""
    return N_SLOTS, Hc + 2, Wc + 1 + (Hc + Wc) % 3


def u8_rw_grid(pool, b16, cus):
    """conv1_plan.h's conv1_u8_rw_grid: (workgroups, waves per workgroup) of the uint8 row walk for a pool of steps
    (tests/test_conv1_plan_host.py holds this copy to the probe)"""
    nw, per_cu = (4, 3) if b16 else (8, 2)
    return max(1, min(-(-pool // (8 * nw)), per_cu * cus)), nw


def wrap_batch(b16, cus):
    """the smallest batch of WRAP_GEOM whose capped grid leaves every wave a share of at least 17 steps"""
    Ho, _ = out_hw(*WRAP_GEOM[1:])
    nw, per_cu = (4, 3) if b16 else (8, 2)
    return -(-17 * nw * per_cu * cus // Ho)


# ------------------------------------------------------------------------------------- inputs and float64 references
# (computed once per case, shared by the forms that run it, never written to)
@functools.lru_cache(maxsize=None)
def conv1_weights(C, seed=0):
    return rnd(32, C, 3, 3, seed=11 + seed, scale=0.2), rnd(32, seed=12 + seed, scale=0.1)


@functools.lru_cache(maxsize=None)
def sampled(C, Hc, Wc, B=None, seed=0):
    """a ring [slots, Hs, Ws, C] of random bytes, B samples (slot, crop origin) of it and their crops [B, Hc, Wc, C]: the
    last sample is the LAST slot cropped at its bottom-right corner, and at least one slot is never sampled"""
    N, Hs, Ws = ring_of(C, Hc, Wc)
    B = B or batch_of(Hc, Wc)
    rs = np.random.RandomState(1000 * C + 7 * Hc + Wc + seed)
    ring = torch.from_numpy(rs.randint(0, 256, (N, Hs, Ws, C), dtype=np.uint8))
    idx = rs.randint(0, N - 2, B)  # (slot N - 2 stays unsampled)
    h1, w1 = rs.randint(0, Hs - Hc + 1, B), rs.randint(0, Ws - Wc + 1, B)
    idx[-1], h1[-1], w1[-1] = N - 1, Hs - Hc, Ws - Wc
    return ring, idx, h1, w1, crop_ref(ring, idx, h1, w1, Hc, Wc)


@functools.lru_cache(maxsize=None)
def u8_fwd_ref(C, Hc, Wc, B=None, seed=0):
    return conv1_fwd_ref(sampled(C, Hc, Wc, B, seed)[4], *conv1_weights(C, seed))


@functools.lru_cache(maxsize=None)
def f32_case(C, Hc, Wc, B=None):
    """x [B, Hc, Wc, C] in [0, 255), w, b and relu(conv2d(x / 255)) in float64"""
    B = B or batch_of(Hc, Wc)
    x = torch.rand(B, Hc, Wc, C, generator=torch.Generator().manual_seed(1000 * C + 7 * Hc + Wc)) * 255.0
    w, b = conv1_weights(C)
    return x, w, b, conv1_fwd_ref(x, w, b)


@functools.lru_cache(maxsize=None)
def gradient(B, Ho, Wo):
    """a ReLU-masked output gradient [B, Ho, Wo, 32]"""
    return rnd(B, Ho, Wo, 32, seed=13) * (rnd(B, Ho, Wo, 32, seed=14) > 0)


@functools.lru_cache(maxsize=None)
def u8_wgrad_ref(C, Hc, Wc, B=None):
    x = sampled(C, Hc, Wc, B)[4]
    return conv1_wgrad_ref(x, gradient(x.shape[0], *out_hw(Hc, Wc)))


@functools.lru_cache(maxsize=None)
def f32_wgrad_ref(C, Hc, Wc, B=None):
    x = f32_case(C, Hc, Wc, B)[0]
    return conv1_wgrad_ref(x, gradient(x.shape[0], *out_hw(Hc, Wc)))


def device_ring(ops, ring, idx, h1, w1, Hc, Wc):
    """the ring on the device, followed by the 32 readable bytes the entry points ask for (zero), and its handle"""
    n = ring.numel()
    store = torch.zeros(n + 32, dtype=torch.uint8, device="cuda")
    store[:n].copy_(ring.view(-1))
    dev = lambda a, t: torch.as_tensor(np.asarray(a)).to(t).cuda()  # noqa: E731
    obs = ops.ObsRef.from_ring(store[:n].view(ring.shape), dev(idx, torch.int64), dev(h1, torch.int32),
                               dev(w1, torch.int32), len(idx), (Hc, Wc))
    return store, obs


def f32_obs(ops, x, source, shift=0):
    """x [B, Hc, Wc, C] inside NaN guards as the float NCHW / NHWC source, and its handle"""
    if source.startswith("nchw"):
        view, intact = guarded(data=x.permute(0, 3, 1, 2).contiguous())
        return view, intact, ops.ObsRef.from_tensor(view)
    view, intact = guarded(data=x, shift=shift)
    return view, intact, ops.ObsRef.from_nhwc(view)


def f32_option(source):
    from curla_amd import _lib
    return _lib.option("conv1_f32", source.split()[1])


def relaunch_same_bits(launch, out, first, what):
    out[0].fill_(NAN)
    launch()
    assert _same_bits(out[0], first), f"{what}: other bits"
    out[1](what)


def unread_bytes_do_not_matter(launch, out, first, store, ring, idx, h1, w1, Hc, Wc, name):
    """the uint8 ring has no NaN bytes: the run again with the 32 bytes behind the ring 0xFF instead of 0x00, and with
    every byte outside the sampled crops (every unsampled slot included) complemented"""
    n = ring.numel()
    store[n:] = 255
    relaunch_same_bits(launch, out, first, f"{name}, 0xFF behind the ring")
    keep = torch.zeros(ring.shape, dtype=torch.bool)
    for i, y, x in zip(idx, h1, w1):
        keep[int(i), int(y):int(y) + Hc, int(x):int(x) + Wc] = True
    assert not bool(keep.view(ring.shape[0], -1).any(1).all()), "an unsampled slot"
    store[:n].copy_(torch.where(keep, ring, 255 - ring).view(-1))
    relaunch_same_bits(launch, out, first, f"{name}, bytes outside the crops complemented")


def run_u8_fwd(ops, C, Hc, Wc, name, B=None):
    ring, idx, h1, w1, _ = sampled(C, Hc, Wc, B)
    store, obs = device_ring(ops, ring, idx, h1, w1, Hc, Wc)
    dw, db = put(*conv1_weights(C))
    out = guarded((len(idx),) + out_hw(Hc, Wc) + (32,))
    launch = lambda: ops.conv1_fwd(obs, dw, db, out[0])  # noqa: E731
    got, = run_twice(launch, [out], name)
    check(name, got.cpu(), u8_fwd_ref(C, Hc, Wc, B))
    unread_bytes_do_not_matter(launch, out, got, store, ring, idx, h1, w1, Hc, Wc, name)


def run_f32_fwd(ops, C, Hc, Wc, source, name, B=None, shift=0):
    x, w, b, ref = f32_case(C, Hc, Wc, B)
    _, src_intact, obs = f32_obs(ops, x, source, shift)
    dw, db = put(w, b)
    out = guarded((x.shape[0],) + out_hw(Hc, Wc) + (32,))
    with f32_option(source):
        got, = run_twice(lambda: ops.conv1_fwd(obs, dw, db, out[0]), [out], name)
    src_intact(f"{name} source")
    check(name, got.cpu(), ref)


def check_slabs(ws, n, C, dw_ref, db_ref, name):
    """the first n slabs [32 C 9 | 32] written everywhere, nothing behind them touched, their float64 sum = dW | db"""
    slab = 32 * C * 9 + 32
    assert 1 <= n and n * slab <= ws.numel()
    assert not bool(torch.isnan(ws[:n * slab]).any()), f"{name}: a slab was left (partly) unwritten"
    assert bool(torch.isnan(ws[n * slab:]).all()), f"{name}: a store behind the {n} slabs"
    total = ws[:n * slab].view(n, slab).double().sum(0).cpu()
    check(f"{name} dW", total[:32 * C * 9].view(32, C, 3, 3), dw_ref)
    check(f"{name} db", total[32 * C * 9:], db_ref)


def run_wgrad(ops, obs, C, Hc, Wc, refs, want_slabs, name):
    """conv1_wgrad_slabs (the documented number of slabs, nothing behind them) and conv1_wgrad (twice) of the handle"""
    dw_ref, db_ref = refs
    dg, = put(gradient(obs.B, *out_hw(Hc, Wc)))
    ws = torch.full((ops.wgrad_workspace_floats(C),), NAN, device="cuda")
    n = ops.conv1_wgrad_slabs(obs, dg, ws, 32)
    assert n == want_slabs, (n, want_slabs)
    check_slabs(ws, n, C, dw_ref, db_ref, f"{name} slabs")
    dw, db = guarded((32, C, 3, 3)), guarded((32,))

    def launch():
        ws.fill_(NAN)  # (a kernel that accumulates into its slab, or reads one it did not write, meets NaN)
        ops.conv1_wgrad(obs, dg, dw[0], db[0], ws)
    got_dw, got_db = run_twice(launch, [dw, db], name)
    check(f"{name} dW", got_dw.cpu(), dw_ref)
    check(f"{name} db", got_db.cpu(), db_ref)
    return launch, dw, got_dw


def run_u8_wgrad(ops, C, Hc, Wc, nbands, name, B=None):
    ring, idx, h1, w1, _ = sampled(C, Hc, Wc, B)
    store, obs = device_ring(ops, ring, idx, h1, w1, Hc, Wc)
    want = min(len(idx) * nbands, 2 * ops.cu_count())
    launch, dw, first = run_wgrad(ops, obs, C, Hc, Wc, u8_wgrad_ref(C, Hc, Wc, B), want, name)
    unread_bytes_do_not_matter(launch, dw, first, store, ring, idx, h1, w1, Hc, Wc, name)


def run_f32_wgrad(ops, C, Hc, Wc, nbands, source, name, B=None, shift=0):
    x = f32_case(C, Hc, Wc, B)[0]
    _, src_intact, obs = f32_obs(ops, x, source, shift)
    cus = ops.cu_count()
    want = min(x.shape[0], cus) if source == "nhwc rw" else min(x.shape[0] * nbands, cus)
    with f32_option(source):
        run_wgrad(ops, obs, C, Hc, Wc, f32_wgrad_ref(C, Hc, Wc, B), want, name)
    src_intact(f"{name} source")


@pytest.fixture(params=U8_FORMS)
def u8_form(request):
    from curla_amd import _lib
    with _lib.option("conv1_u8", request.param):
        yield request.param


@pytest.fixture(params=U8_WGRAD_FORMS)
def u8_wgrad_form(request):
    from curla_amd import _lib
    with _lib.option("wgrad1_u8", request.param):
        yield request.param


# ------------------------------------------------------------------------------------------------------- the sweeps
@pytest.mark.parametrize("C,Hc,Wc", U8_FWD_GEOMS)
def test_u8_forward_sweep(ops, u8_form, C, Hc, Wc):
    run_u8_fwd(ops, C, Hc, Wc, f"conv1 edges fwd u8 [{u8_form}] C{C} {Hc}x{Wc}")


@pytest.mark.parametrize("C,Hc,Wc", F32_FWD_GEOMS)
@pytest.mark.parametrize("source", F32_SOURCES)
def test_f32_forward_sweep(ops, source, C, Hc, Wc):
    run_f32_fwd(ops, C, Hc, Wc, source, f"conv1 edges fwd f32 [{source}] C{C} {Hc}x{Wc}")


@pytest.mark.parametrize("C,Hc,Wc,nbands", U8_WGRAD_GEOMS)
def test_u8_weight_gradient_sweep(ops, u8_wgrad_form, C, Hc, Wc, nbands):
    run_u8_wgrad(ops, C, Hc, Wc, nbands, f"conv1 edges wgrad u8 [{u8_wgrad_form}] C{C} {Hc}x{Wc}")


@pytest.mark.parametrize("C,Hc,Wc,nbands", F32_WGRAD_GEOMS)
@pytest.mark.parametrize("source", F32_SOURCES)
def test_f32_weight_gradient_sweep(ops, source, C, Hc, Wc, nbands):
    run_f32_wgrad(ops, C, Hc, Wc, nbands, source, f"conv1 edges wgrad f32 [{source}] C{C} {Hc}x{Wc}")


@pytest.mark.parametrize("C,H,W", DGRAD_GEOMS)
@pytest.mark.parametrize("nf", [32, 8])
def test_observation_gradient(ops, nf, C, H, W):
    B = batch_of(H, W)
    Ho, Wo = out_hw(H, W)
    g, w = rnd(B, Ho, Wo, nf, seed=21), rnd(nf, C, 3, 3, seed=22, scale=0.2)
    dg, dw = put(g, w)
    dobs = guarded((B, C, H, W))
    name = f"conv1 edges dgrad nf{nf} C{C} {H}x{W}"
    got, = run_twice(lambda: ops.conv1_dgrad(dg, dw, dobs[0]), [dobs], name)
    check(name, got.cpu(), conv1_dgrad_ref(g, w, H, W))


@pytest.mark.parametrize("C,Hc,Wc", [(12, 9, 11), (9, 10, 13)])  # rows of 132 and 117 floats: 0 and 1 mod 4
@pytest.mark.parametrize("source", ["nhwc rw", "nhwc band"])
def test_nhwc_source_four_bytes_past_alignment(ops, source, C, Hc, Wc):
    """a float NHWC tensor that starts 4 bytes past a 16-byte boundary (the entry points do not ask for more)"""
    run_f32_fwd(ops, C, Hc, Wc, source, f"conv1 edges fwd f32 [{source}, 4 bytes off] C{C} {Hc}x{Wc}", shift=1)
    nbands = 1  # (crops this small are one band)
    run_f32_wgrad(ops, C, Hc, Wc, nbands, source, f"conv1 edges wgrad f32 [{source}, 4 bytes off] C{C} {Hc}x{Wc}", shift=1)


# ------------------------------------------------------------------------------------------- two problems, one launch
@pytest.mark.parametrize("C,Hc,Wc", FWD2_GEOMS)
def test_u8_forward_two_problems(ops, u8_form, C, Hc, Wc):
    """conv1_fwd2, 3 + 2 samples with their own slots, origins and weights: each output against float64, bit-identical to
    its single launch, inside guards, twice"""
    assert (C, Hc, Wc) in U8_FWD_GEOMS
    cases = [sampled(C, Hc, Wc, B, seed) for B, seed in ((3, 0), (2, 1))]
    ring = cases[0][0]
    n = ring.numel()
    store = torch.zeros(n + 32, dtype=torch.uint8, device="cuda")
    store[:n].copy_(ring.view(-1))
    dev = lambda a, t: torch.as_tensor(np.asarray(a)).to(t).cuda()  # noqa: E731
    refs, wb, singles, outs = [], [], [], []
    for k, (_, idx, h1, w1, _) in enumerate(cases):
        refs.append(ops.ObsRef.from_ring(store[:n].view(ring.shape), dev(idx, torch.int64), dev(h1, torch.int32),
                                         dev(w1, torch.int32), len(idx), (Hc, Wc)))
        wb.append(put(*conv1_weights(C, k)))
        singles.append(guarded((len(idx),) + out_hw(Hc, Wc) + (32,)))
        outs.append(guarded((len(idx),) + out_hw(Hc, Wc) + (32,)))
        ops.conv1_fwd(refs[k], *wb[k], singles[k][0])
        singles[k][1](f"single {k}")
    assert ops.conv1_pairable(refs[0], refs[1])
    name = f"conv1 edges fwd2 u8 [{u8_form}] C{C} {Hc}x{Wc}"
    got = run_twice(lambda: ops.conv1_fwd2(refs[0], *wb[0], outs[0][0], refs[1], *wb[1], outs[1][0]), outs, name)
    for k, (B, seed) in enumerate(((3, 0), (2, 1))):
        # (the second problem's crops come from the FIRST problem's ring: its float64 reference is computed from them)
        _, idx, h1, w1, _ = cases[k]
        ref = conv1_fwd_ref(crop_ref(ring, idx, h1, w1, Hc, Wc), *conv1_weights(C, k))
        check(f"{name} problem {k}", got[k].cpu(), ref)
        assert _same_bits(got[k], singles[k][0]), f"problem {k} differs from its single launch"


# ------------------------------------------------------------------------------------------------------ NaN semantics
def nan_weight_and_bias(launch, dw, db, out, name):
    """one weight, then one bias element, NaN with its sign bit clear and set: that output channel is NaN at every
    pixel, every other channel keeps the bits of the clean run"""
    out[0].fill_(NAN)
    launch()
    clean = out[0].clone()
    assert bool(torch.isfinite(clean).all()), f"{name}: the clean run"
    C = dw.shape[1]
    for what, t, k, co in (("weight", dw, (5 * C + C - 1) * 9 + 5, 5), ("bias", db, 19, 19)):
        cell = t.view(-1).view(torch.int32)[k:k + 1]
        saved = cell.clone()
        for bits in (POS_NAN, NEG_NAN):
            cell.fill_(bits)
            out[0].fill_(NAN)
            launch()
            cell.copy_(saved)
            out[1](f"{name}, NaN {what}")
            got = out[0]
            assert bool(torch.isnan(got[..., co]).all()), f"{name}: a NaN {what} ({bits & 0xFFFFFFFF:#x}) left channel {co} finite"
            others = [c for c in range(32) if c != co]
            assert _same_bits(got[..., others], clean[..., others]), f"{name}: a NaN {what} changed another channel"


@pytest.mark.parametrize("C,Hc,Wc", NAN_GEOMS)
def test_u8_forward_keeps_a_nan_weight_or_bias(ops, u8_form, C, Hc, Wc):
    ring, idx, h1, w1, _ = sampled(C, Hc, Wc)
    _, obs = device_ring(ops, ring, idx, h1, w1, Hc, Wc)
    dw, db = put(*conv1_weights(C))
    out = guarded((len(idx),) + out_hw(Hc, Wc) + (32,))
    nan_weight_and_bias(lambda: ops.conv1_fwd(obs, dw, db, out[0]), dw, db, out, f"u8 [{u8_form}] C{C} {Hc}x{Wc}")


@pytest.mark.parametrize("C,Hc,Wc", NAN_GEOMS)
@pytest.mark.parametrize("source", F32_SOURCES)
def test_f32_forward_keeps_a_nan_weight_or_bias(ops, source, C, Hc, Wc):
    x, w, b, _ = f32_case(C, Hc, Wc)
    _, _, obs = f32_obs(ops, x, source)
    dw, db = put(w, b)
    out = guarded((x.shape[0],) + out_hw(Hc, Wc) + (32,))
    with f32_option(source):
        nan_weight_and_bias(lambda: ops.conv1_fwd(obs, dw, db, out[0]), dw, db, out, f"f32 [{source}] C{C} {Hc}x{Wc}")


@pytest.mark.parametrize("C,Hc,Wc", NAN_GEOMS)
@pytest.mark.parametrize("source", F32_SOURCES)
def test_f32_forward_nonfinite_pixel_reaches_its_windows_only(ops, source, C, Hc, Wc):
    """One NaN, then one Inf, in channel 0 of one pixel -- the channel a lane group's zero-weight padding lanes read when
    they reach into the next pixel (0 x NaN = NaN): interior (column 3 = the first pixel past output column 0's window),
    first column (what follows the last window of the row above in memory), last column, last row; first and last sample.
    The outputs float64 torch makes NaN are NaN (an Inf: +Inf or 0 behind the ReLU, as float64 has them) and EVERY other
    output keeps the bits of the clean run."""
    x, w, b, ref_clean = f32_case(C, Hc, Wc)
    B = x.shape[0]
    view, intact, obs = f32_obs(ops, x, source)
    dw, db = put(w, b)
    out = guarded((B,) + out_hw(Hc, Wc) + (32,))
    with f32_option(source):
        ops.conv1_fwd(obs, dw, db, out[0])
        clean = out[0].clone()
        assert bool(torch.isfinite(clean).all())
        for where, (r, c) in (("interior", (2, 3)), ("first column", (3, 0)), ("last column", (1, Wc - 1)),
                              ("last row", (Hc - 1, 2))):
            for s in (0, B - 1):
                for value in (NAN, float("inf")):
                    xb = x.clone()
                    xb[s, r, c, 0] = value
                    ref = conv1_fwd_ref(xb, w, b)
                    hit = ref != ref_clean  # (NaN != anything; +Inf and the 0 of a -Inf differ from the clean value)
                    view.copy_(xb.permute(0, 3, 1, 2) if source.startswith("nchw") else xb)
                    out[0].fill_(NAN)
                    ops.conv1_fwd(obs, dw, db, out[0])
                    what = f"f32 [{source}] C{C} {Hc}x{Wc}: {value} at {where} of sample {s}"
                    out[1](what), intact(what)
                    got = out[0].cpu()
                    assert torch.equal(torch.isnan(got), torch.isnan(ref)), \
                        f"{what}: {int(torch.isnan(got).sum())} NaN outputs, float64 has {int(torch.isnan(ref).sum())}"
                    assert torch.equal(got[hit & ~torch.isnan(ref)], ref[hit & ~torch.isnan(ref)].float()), what
                    assert _same_bits(got[~hit], clean.cpu()[~hit]), f"{what}: an output outside its windows changed"


# ------------------------------------------------------------------------------------------------ batch against grid
# Persistent loops take a second item only when there are more items than workgroups.  CUs = the device's count (the
# granule of the stride-1 stack); crops of 5 x 7 x 3 (outputs of 2 x 3) keep 2 CUs + 3 samples at a few hundred KB.
def test_float_band_forward_second_item(ops):
    """conv1_fwd_kernel: min(B nbands, 2 CUs) workgroups"""
    B = 2 * ops.stack_granule() + 3
    for source in ("nchw band", "nhwc band"):
        run_f32_fwd(ops, 3, 5, 7, source, f"conv1 edges fwd f32 [{source}] B = 2 CUs + 3 = {B} in 5x7", B=B)


def test_float_row_walk_second_item(ops):
    """conv1_rw and wgrad1_rw: min(B, CUs) workgroups"""
    B = ops.stack_granule() + 3
    run_f32_fwd(ops, 3, 5, 7, "nhwc rw", f"conv1 edges fwd f32 [nhwc rw] B = CUs + 3 = {B} in 5x7", B=B)
    run_f32_wgrad(ops, 3, 5, 7, 1, "nhwc rw", f"conv1 edges wgrad f32 [nhwc rw] B = CUs + 3 = {B} in 5x7", B=B)


def test_float_band_weight_gradient_second_item(ops):
    """wgrad1_kernel: min(B nbands, CUs) workgroups"""
    B = ops.stack_granule() + 3
    for source in ("nchw band", "nhwc band"):
        run_f32_wgrad(ops, 3, 5, 7, 1, source, f"conv1 edges wgrad f32 [{source}] B = CUs + 3 = {B} in 5x7", B=B)


def test_u8_weight_gradient_second_item(ops, u8_wgrad_form):
    """wgrad1_u8 / wgrad1_u8b: min(B nbands, 2 CUs) workgroups.  The bf16 form needs output rows of 8 pixels: 5 x 19 crops
    there (a 5 x 7 crop takes the f32 form under either option: run under both all the same)"""
    B = 2 * ops.stack_granule() + 3
    for Wc in (7, 19):
        run_u8_wgrad(ops, 3, 5, Wc, 1, f"conv1 edges wgrad u8 [{u8_wgrad_form}] B = 2 CUs + 3 = {B} in 5x{Wc}", B=B)


def per_slot_case(C, Hc, Wc, B, seed):
    """B samples of WHOLE frames of a small ring: the ring, the slots, the float64 forward per slot"""
    rs = np.random.RandomState(seed)
    ring = torch.from_numpy(rs.randint(0, 256, (WRAP_SLOTS, Hc, Wc, C), dtype=np.uint8))
    idx = rs.randint(0, WRAP_SLOTS, B)
    idx[:WRAP_SLOTS] = np.arange(WRAP_SLOTS)  # (sample s < slots is slot s: every slot has a representative)
    return ring, idx


def check_per_slot(name, got, idx, ref_slots):
    """every sample of a slot bit-identical to the slot's first sample (compared on the device), the representatives
    against float64"""
    first = got[:WRAP_SLOTS]
    assert _same_bits(got, first[torch.as_tensor(idx).cuda()]), f"{name}: samples of one slot differ"
    check(name, first.cpu(), ref_slots)


def test_wide_rows_make_the_bands(ops):
    """nbands = 2 because ROWS are wide (300 x 12 bytes), not because the image is tall; B nbands just above 2 CUs: the
    banded uint8 forward and both uint8 weight gradients"""
    from curla_amd import _lib
    C, Hc, Wc = WIDE_GEOM
    B = ops.stack_granule() + 2
    Ho, Wo = out_hw(Hc, Wc)
    ring, idx = per_slot_case(C, Hc, Wc, B, 5)
    z = np.zeros(B, dtype=np.int64)
    _, obs = device_ring(ops, ring, idx, z, z, Hc, Wc)
    w, b = conv1_weights(C)
    dw, db = put(w, b)
    out = guarded((B, Ho, Wo, 32))
    name = f"conv1 edges fwd u8 [band] B = CUs + 2 = {B} in {Hc}x{Wc}x{C}"
    with _lib.option("conv1_u8", "band"):
        got, = run_twice(lambda: ops.conv1_fwd(obs, dw, db, out[0]), [out], name)
    check_per_slot(name, got, idx, conv1_fwd_ref(ring, w, b))
    # the weight gradient: float64 per slot under the slot's summed gradients (dW is linear in g)
    g = gradient(B, Ho, Wo)
    gsum = torch.zeros(WRAP_SLOTS, Ho, Wo, 32, dtype=torch.float64).index_add_(0, torch.as_tensor(idx), g.double())
    refs = conv1_wgrad_ref(ring, gsum)
    for form in U8_WGRAD_FORMS:
        with _lib.option("wgrad1_u8", form):
            run_wgrad(ops, obs, C, Hc, Wc, refs, min(2 * B, 2 * ops.cu_count()),
                      f"conv1 edges wgrad u8 [{form}] B = CUs + 2 = {B} in {Hc}x{Wc}x{C}")


@pytest.mark.parametrize("form", ["rw", "rwb"])
def test_u8_row_walk_rotation_wraps(ops, form):
    """The uint8 row walks unroll 15 steps of their register rotation; a wave gets about 8 steps until the grid reaches
    its cap.  Here the pool is just large enough that every wave's share is 17 steps of the 34-row strips: pieces of 17
    consecutive rows, the rotation wraps.  (The one large case: ~140 MB of output on 256 CUs.)"""
    from curla_amd import _lib
    C, Hc, Wc = WRAP_GEOM
    Ho, Wo = out_hw(Hc, Wc)
    b16 = form == "rwb"
    cus = ops.stack_granule()
    B = wrap_batch(b16, cus)
    grid, nw = u8_rw_grid(B * Ho, b16, cus)
    assert (B * Ho // grid) // nw >= 17, "the smallest share of a wave"
    ring, idx = per_slot_case(C, Hc, Wc, B, 6)
    z = np.zeros(B, dtype=np.int64)
    _, obs = device_ring(ops, ring, idx, z, z, Hc, Wc)
    w, b = conv1_weights(C)
    dw, db = put(w, b)
    out = guarded((B, Ho, Wo, 32))
    name = f"conv1 edges fwd u8 [{form}] rotation wrap B{B} {Hc}x{Wc}x{C}"
    with _lib.option("conv1_u8", form):
        got, = run_twice(lambda: ops.conv1_fwd(obs, dw, db, out[0]), [out], name)
    check_per_slot(name, got, idx, conv1_fwd_ref(ring, w, b))
