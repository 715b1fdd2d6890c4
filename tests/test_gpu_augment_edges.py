"""The float augmentation kernels of ``curla_amd/csrc/augment.hip`` at their edges, on the MI355X.

Colour jitter (``curla_color_jiggle``: the three pixel-per-thread instances, the flat kernel, the NCHW kernel) against
the float64 restatement ``tests/_augment_ref.color_jiggle_f64`` on the edge-case pixels and parameters, all 24 orders;
noisy cover (explicit noise, NCHW, drawn noise) and the plain gather bit for bit against float32 / byte restatements.
Every output lies in a NaN-filled buffer with GUARD floats on either side that must still be NaN afterwards, every
ring carries 32 bytes of slack that must still be zero.

THE BOUND of the jitter, per element, absolute on the [0, 255] output: |kernel - f64| <= 4 x floor, where
floor = max |oracle_f32 - f64| of the float32 oracle (``oracle.curla_oracle.color_jiggle``) on the SAME inputs and
order, computed on the host inside the test (tests/test_augment_edges_host.py holds it under 2e-3; it is 3.4e-4 to
1.04e-3, by order).  The floor is what float32 rounding costs an honest implementation; the factor 4 pays for the
kernel's 1-ulp reciprocals in place of divisions and its saturation change evaluated in RGB, each of the floor's own
order.  Nothing in the bound comes from the kernel.  No element is excluded.

Worst |kernel - f64| / floor over the 24 orders, gathered rows and idx = None, per C: NOT MEASURED on the MI355X yet
(MEASURED_WORST_RATIO below is to be filled from the printout of the first
run).  What exists is a rehearsal on the host with the kernels replaced by a NumPy float32 emulation of
``jiggle_rgb`` (correctly rounded 1 / x for v_rcp_f32): 0.6 .. 1.0 of the floor at every C, 0.5 .. 0.75 at the small
geometries; the same emulation with reciprocals 2^-17 off fails the bound at 35 x floor (0.0119 absolute, which the
1e-4-relative bound of tests/test_gpu_augment.py lets through).
"""
import numpy as np
import pytest
import torch

from tests import _augment_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64      # floats on either side of every output
FACTOR = 4.0    # the issue's: |kernel - f64| <= FACTOR * floor
NAN = float("nan")

# worst |kernel - f64| / floor seen on the MI355X, per C (to be recorded from this file's own printout; None = not
# measured; not used by any assertion)
MEASURED_WORST_RATIO = {3: None, 6: None, 9: None, 12: None, 15: None}

_seen = {}  # C -> worst ratio of this run, printed as it grows


# ------------------------------------------------------------------------------------------------ helpers
def _guarded(shape, lead=0):
    """(buffer, view): a NaN-filled float buffer and the tensor ``shape`` inside it, GUARD + lead floats in -- on the
    16-byte grid for lead = 0 (the allocator's alignment), off it for lead in 1..3."""
    n = int(np.prod(shape))
    buf = torch.full((GUARD + lead + n + GUARD,), NAN, device="cuda")
    view = buf[GUARD + lead:GUARD + lead + n].view(shape)
    assert (view.data_ptr() % 16 == 0) == (lead % 4 == 0)
    return buf, view


def _guards_intact(buf, view):
    """Both guards still NaN, no NaN left inside; returns the tensor on the host."""
    host = buf.cpu()
    lo = (view.data_ptr() - buf.data_ptr()) // 4
    n = view.numel()
    assert lo >= GUARD and host.numel() - (lo + n) >= GUARD
    assert bool(torch.isnan(host[:lo]).all()), "written before the output"
    assert bool(torch.isnan(host[lo + n:]).all()), "written behind the output"
    got = host[lo:lo + n].view(view.shape)
    assert not bool(torch.isnan(got).any()), "elements of the output left unwritten"
    return got


class _Ring:
    """uint8 NHWC frames in a zeroed store with ``lead`` bytes before and 32 bytes of slack behind them."""

    def __init__(self, frames_nhwc, lead=0):
        n = frames_nhwc.size
        self.store = torch.zeros(lead + n + 32, dtype=torch.uint8, device="cuda")
        self.ring = self.store[lead:lead + n].view(frames_nhwc.shape)
        self.ring.copy_(torch.from_numpy(frames_nhwc))
        self.lead, self.n = lead, n
        assert self.ring.data_ptr() % 4 == lead % 4

    def untouched(self, frames_nhwc):
        host = self.store.cpu()
        assert not bool(host[:self.lead].any()) and not bool(host[self.lead + self.n:].any()), "ring slack written"
        assert torch.equal(host[self.lead:self.lead + self.n].view(frames_nhwc.shape), torch.from_numpy(frames_nhwc))


def _nchw(a):
    return np.ascontiguousarray(a.transpose(0, 3, 1, 2))


def _nhwc(a):
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1))


def _order(order):
    return torch.tensor(order, dtype=torch.int32, device="cuda")


def _ref_and_floor(batch_nhwc, params, order):
    """(float64 reference as NHWC, floor = max |oracle_f32 - f64|): both from the host, on the launch's inputs."""
    imgs = _nchw(batch_nhwc)
    ref = R.color_jiggle_f64(imgs, params, order)
    floor = float(np.abs(R.color_jiggle_oracle_f32(imgs, params, order) - ref).max())
    return _nhwc(ref), floor


def _per_image(x_nhwc, k):
    B, H, W, C = x_nhwc.shape
    return x_nhwc.reshape(B, H, W, k, 3).transpose(0, 3, 1, 2, 4).reshape(B * k, H, W, 3)


def _jiggle(ring, idx, params, order, B, lead=0):
    from curla_amd import ops
    _, H, W, C = ring.shape
    buf, out = _guarded((B, H, W, C), lead)
    ops.color_jiggle(ring, idx, params, order, B, out)
    return _guards_intact(buf, out)


# ------------------------------------------------------------------------------------------------ jitter vs float64
@pytest.mark.parametrize("first", [0, 1, 2, 3])
@pytest.mark.parametrize("C", [3, 6, 9, 12, 15])
def test_color_jiggle_against_float64_on_the_edge_set(C, first):
    """jiggle_case(C, 23, 29) in the six orders that begin with ``first`` (all 24 over the parametrisation), the
    minibatch once gathered by an index with repeats from the ring of the case and once read in place (idx = None)
    from a ring that holds the gathered rows: one reference serves both.  C = 3, 6, 9, 12 take
    color_jiggle_pixel_kernel<1..4> (HW = 667: blocks of 256 and a last wave of 27 pixels), C = 15 the flat kernel."""
    k = C // 3
    frames, params = R.jiggle_case(C, *R.CASE_HW)
    B = frames.shape[0]
    rows = np.random.RandomState(C).randint(0, B, B)
    rows[1] = rows[0]
    batch = frames[rows]
    gathered, plain = _Ring(frames), _Ring(batch)
    d_rows, d_params = torch.from_numpy(rows).cuda(), torch.from_numpy(params).cuda()
    off = params[:, 0] == 0
    assert int(off.sum()) >= 1
    bytes_off = _per_image(batch, k)[off].astype(np.float32)
    for order in [o for o in R.ORDERS if o[0] == first]:
        ref, floor = _ref_and_floor(batch, params, order)
        assert 0.0 < floor <= 2e-3
        for name, ring, idx in (("gathered", gathered.ring, d_rows), ("idx=None", plain.ring, None)):
            got = _jiggle(ring, idx, d_params, _order(order), B).numpy()
            err = np.abs(got.astype(np.float64) - ref)
            worst = float(err.max())
            _seen[C] = max(_seen.get(C, 0.0), worst / floor)
            print(f"C={C} order={order} {name}: worst |kernel - f64| = {worst:.3e}, floor = {floor:.3e}, "
                  f"ratio {worst / floor:.2f} (worst ratio for C={C} so far: {_seen[C]:.2f})")
            where = np.unravel_index(int(err.argmax()), err.shape)
            assert worst <= FACTOR * floor, (C, order, name, where, worst, floor)
            # apply = 0: (byte * (1 / 255)) * 255 in float32, within one ulp of the byte
            got_off = _per_image(got, k)[off]
            assert bool((np.abs(got_off - bytes_off) <= np.spacing(bytes_off)).all()), (C, order, name)
    gathered.untouched(frames)
    plain.untouched(batch)


# ------------------------------------------------------------------------------------------------ jitter, paths
@pytest.mark.parametrize("H,W", [(1, 1), (7, 9), (5, 13), (1, 257)])
def test_color_jiggle_short_waves_and_small_batches(H, W):
    """HW = 1, 63, 65, 257: a single lane, a wave one pixel short, one pixel into a second wave, one pixel into a
    second block (``p_raw`` clamped to HW - 1, ``nvalid``, whole waves leaving).  K in 1..4, B in {1, 3}, all 24
    orders, gathered rows and idx = None in turn.  A launch here has as few as 3 elements, too few for a floor of its
    own (a black pixel has floor 0): the floor is the oracle's worst distance over ALL the launches of the case -- the
    same inputs the kernel's worst error is taken over."""
    rs = np.random.RandomState(H * W)
    shift, n_launch = 0, 0
    worst, worst_at, floor = 0.0, None, 0.0
    for K in (1, 2, 3, 4):
        for B in (1, 3):
            d_order = {tuple(o): _order(o) for o in R.ORDERS}
            for j, order in enumerate(R.ORDERS):
                frames, params = R.jiggle_case(3 * K, H, W, B=B + 2, shift=shift)
                shift += 7
                params = params[:B * K]
                if j % 2 == 0:
                    rows = rs.randint(0, B + 2, B)
                    rows[-1] = rows[0]
                    idx = torch.from_numpy(rows).cuda()
                else:
                    rows, idx = np.arange(B), None
                ring = _Ring(frames)
                got = _jiggle(ring.ring, idx, torch.from_numpy(params).cuda(), d_order[tuple(order)], B).numpy()
                ref, fl = _ref_and_floor(frames[rows], params, order)
                floor = max(floor, fl)
                e = float(np.abs(got.astype(np.float64) - ref).max())
                if e > worst:
                    worst, worst_at = e, (K, B, order, idx is not None)
                if j % 8 == 0:
                    ring.untouched(frames)
                n_launch += 1
    print(f"HW={H * W}: {n_launch} launches, worst |kernel - f64| = {worst:.3e} at {worst_at}, floor = {floor:.3e}, "
          f"ratio {worst / floor:.2f}")
    assert 0.0 < floor <= 2e-3
    assert worst <= FACTOR * floor, (worst_at, worst, floor)


@pytest.mark.parametrize("H,W", [(5, 13), R.CASE_HW])
def test_color_jiggle_unaligned_out_and_ring_equal_the_aligned_run(H, W):
    """C = 12: ``out`` one float off the 16-byte grid takes the direct per-lane stores instead of the LDS-staged
    16-byte ones; a ring 1 or 3 bytes off the dword grid takes the byte loads instead of the three dwords.  Each is
    the aligned run bit for bit (and that one is within the bound of the float64 reference)."""
    B = 3
    frames, params = R.jiggle_case(12, H, W, B=B + 2, shift=H)
    params = params[:B * 4]
    rows = np.array([4, 1, 4])
    idx, d_params = torch.from_numpy(rows).cuda(), torch.from_numpy(params).cuda()
    aligned_ring = _Ring(frames)
    for order in ([0, 1, 2, 3], [3, 2, 1, 0], [2, 3, 0, 1]):
        base = _jiggle(aligned_ring.ring, idx, d_params, _order(order), B)
        ref, floor = _ref_and_floor(frames[rows], params, order)
        assert float(np.abs(base.numpy().astype(np.float64) - ref).max()) <= FACTOR * floor
        for lead in (1, 2, 3):
            assert torch.equal(_jiggle(aligned_ring.ring, idx, d_params, _order(order), B, lead=lead), base), ("out", lead)
        for lead in (1, 3):
            ring = _Ring(frames, lead=lead)
            assert torch.equal(_jiggle(ring.ring, idx, d_params, _order(order), B), base), ("ring", lead)
            assert torch.equal(_jiggle(ring.ring, None, d_params, _order(order), B, lead=1),
                               _jiggle(aligned_ring.ring, None, d_params, _order(order), B)), ("ring + out", lead)
            ring.untouched(frames)
    aligned_ring.untouched(frames)


@pytest.mark.parametrize("C", [6, 15])
def test_color_jiggle_nchw_equals_nhwc_and_runs_in_place(C):
    """The NCHW kernel (the reference's tensor contract) is the NHWC kernel bit for bit at C = 6 (pixel kernel<2>) and
    C = 15 (flat kernel) -- tests/test_gpu_augment.py has C = 12 --, and ``out=x`` is the out-of-place result."""
    from curla_amd import ops
    frames, params = R.jiggle_case(C, *R.CASE_HW)
    B = frames.shape[0]
    d_params = torch.from_numpy(params).cuda()
    ring = _Ring(frames)
    x_host = torch.from_numpy(_nchw(frames).astype(np.float32))
    for order in ([1, 3, 2, 0], [2, 0, 3, 1]):
        nhwc = _jiggle(ring.ring, None, d_params, _order(order), B)
        x = x_host.cuda()
        buf, out = _guarded(tuple(x.shape))
        ops.color_jiggle_nchw(x, d_params, _order(order), out)
        apart = _guards_intact(buf, out)
        assert torch.equal(x.cpu(), x_host)  # the argument is left alone
        assert torch.equal(apart, nhwc.permute(0, 3, 1, 2).contiguous())
        buf, inplace = _guarded(tuple(x.shape))
        inplace.copy_(x)
        ops.color_jiggle_nchw(inplace, d_params, _order(order), inplace)
        assert torch.equal(_guards_intact(buf, inplace), apart)
    ring.untouched(frames)


def test_color_jiggle_flat_kernel_equals_the_pixel_kernel():
    """B = 65536 samples of 1 x 2 x 12 in one launch exceed a grid's 65535 rows and take the flat kernel; the same rows
    as two launches of 32768 take color_jiggle_pixel_kernel<4>.  The flat kernel's comment promises bit-identical
    results."""
    from curla_amd import ops
    B, H, W, C = 65536, 1, 2, 12
    half = B // 2
    frames, params = R.jiggle_case(C, H, W, B=B)
    ring = _Ring(frames)
    d_params = torch.from_numpy(params).cuda()
    for order in ([0, 1, 2, 3], [3, 2, 0, 1]):
        flat = _jiggle(ring.ring, None, d_params, _order(order), B)
        buf, out = _guarded((B, H, W, C))
        for h in (0, 1):
            ops.color_jiggle(ring.ring[h * half:], None, d_params[h * half * 4:], _order(order), half, out[h * half:(h + 1) * half])
        assert torch.equal(_guards_intact(buf, out), flat)
    # ... and the two agree with the float64 reference on a slice that holds every parameter row
    n = 116
    ref, floor = _ref_and_floor(frames[:n], params[:n * 4], [3, 2, 0, 1])
    assert float(np.abs(flat[:n].numpy().astype(np.float64) - ref).max()) <= FACTOR * floor
    ring.untouched(frames)


# ------------------------------------------------------------------------------------------------ noisy cover
COVERS = [(21, 0, 0), (21, 7, 5), (21, 21, 0), (21, 0, 21), (21, 15, 10), (21, 24, 24), (21, 0, 1), (21, 1, 0),
          (1, 1, 0), (1, 0, 0)]  # (H, top, bottom)
COLORS = (17.5, -3.0, 300.25)
W_COVER = 23


def _cover_case(C, B, H, seed):
    rs = np.random.RandomState(seed)
    frames = rs.randint(0, 256, (7, H, W_COVER, C), dtype=np.uint8)
    rows = rs.randint(0, 7, B)
    rows[-1] = rows[0]
    noise = (rs.randn(B, H, W_COVER, C) * 60.0).astype(np.float32)
    noise.flat[0], noise.flat[-1] = -1000.0, 1000.0  # both clamps fire whatever lies beneath
    return frames, rows, noise


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("C", [1, 3, 4, 9, 12])
def test_noisy_cover_bit_exact(C, B):
    """``noisy_cover`` (NHWC from the ring, gathered rows with a repeat) and ``noisy_cover_nchw`` (apart and in place)
    against the float32 restatement with ``torch.equal``: no cover, the fixture's kind, everything covered from the
    top / from the bottom / by overlap / by rows beyond the frame, single rows, H = 1; fractional colours and colours
    outside [0, 255]; channel counts that are no multiple of 3."""
    from curla_amd import ops
    for H, top, bottom in COVERS:
        frames, rows, noise = _cover_case(C, B, H, 1000 * C + 10 * B + top)
        want = torch.from_numpy(R.noisy_cover_f32(frames, rows, noise, COLORS, top, bottom))
        assert float(want.min()) == 0.0 and float(want.max()) == 255.0
        ring = _Ring(frames)
        buf, out = _guarded((B, H, W_COVER, C))
        ops.noisy_cover(ring.ring, torch.from_numpy(rows).cuda(), torch.from_numpy(noise).cuda(), COLORS, top, bottom, B, out)
        assert torch.equal(_guards_intact(buf, out), want), ("nhwc", H, top, bottom)
        ring.untouched(frames)
        want_nchw = want.permute(0, 3, 1, 2).contiguous()
        x_host = torch.from_numpy(_nchw(frames[rows]).astype(np.float32))
        x, d_noise = x_host.cuda(), torch.from_numpy(_nchw(noise)).cuda()
        buf, out = _guarded(tuple(x.shape))
        ops.noisy_cover_nchw(x, d_noise, COLORS, top, bottom, out)
        assert torch.equal(_guards_intact(buf, out), want_nchw), ("nchw", H, top, bottom)
        assert torch.equal(x.cpu(), x_host)
        buf, inplace = _guarded(tuple(x.shape))
        inplace.copy_(x)
        ops.noisy_cover_nchw(inplace, d_noise, COLORS, top, bottom, inplace)
        assert torch.equal(_guards_intact(buf, inplace), want_nchw), ("nchw in place", H, top, bottom)


@pytest.mark.parametrize("C", [3, 12])
def test_noisy_cover_rng_equals_the_explicit_kernel_at_every_cover(C):
    """``noisy_cover_rng`` works out its covered byte ranges on the host (``lo`` / ``hi``), the explicit kernel
    compares rows on the device: the same picture at every (top, bottom), rows beyond the frame included
    (tests/test_gpu_graph_aug.py has (7, 5)).  Output and recorded noise between guards; the recorded noise fed to the
    explicit kernel and to the float32 restatement gives the drawn kernel's output bit for bit."""
    from curla_amd import ops
    B, std = 5, 60.0
    for H, top, bottom in COVERS:
        frames, rows, _ = _cover_case(C, B, H, 77 * C + top)
        ring, idx = _Ring(frames), torch.from_numpy(rows).cuda()
        shape = (B, H, W_COVER, C)
        buf, out = _guarded(shape)
        nbuf, nz = _guarded(shape)
        ops.noisy_cover_rng(ring.ring, idx, std, (0x5EED_0000_0000_0001 + top, 2 ** 33 + bottom), COLORS, top, bottom, B, out,
                            noise_out=nz)
        drawn, noise = _guards_intact(buf, out), _guards_intact(nbuf, nz)
        buf, ref = _guarded(shape)
        ops.noisy_cover(ring.ring, idx, nz, COLORS, top, bottom, B, ref)
        assert torch.equal(_guards_intact(buf, ref), drawn), (H, top, bottom)
        assert torch.equal(drawn, torch.from_numpy(R.noisy_cover_f32(frames, rows, noise.numpy(), COLORS, top, bottom)))
        if H > 1:  # 7245 elements or more at std 60: both clamps fire
            assert float(drawn.min()) == 0.0 and float(drawn.max()) == 255.0
        ring.untouched(frames)


# ------------------------------------------------------------------------------------------------ gather
@pytest.mark.parametrize("C,H,W", [(1, 1, 1), (5, 3, 7), (12, 9, 11)])
def test_gather_nhwc_is_the_bytes(C, H, W):
    from curla_amd import ops
    rs = np.random.RandomState(C + H + W)
    frames = rs.randint(0, 256, (6, H, W, C), dtype=np.uint8)
    frames[0].flat[0], frames[-1].flat[-1] = 255, 0
    ring = _Ring(frames)
    for rows in (np.array([5, 2, 5, 0, 3, 3, 1]), None):
        B = 6 if rows is None else len(rows)
        buf, out = _guarded((B, H, W, C))
        ops.gather_nhwc(ring.ring, None if rows is None else torch.from_numpy(rows).cuda(), B, out)
        want = frames if rows is None else frames[rows]
        assert torch.equal(_guards_intact(buf, out), torch.from_numpy(want.astype(np.float32)))
    ring.untouched(frames)
