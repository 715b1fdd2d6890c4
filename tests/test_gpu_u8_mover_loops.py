"""The two loops of the uint8 movers' frame (``u8_mover_kernel`` for the shift and the translate, its written-out copy in
``cutout_u8_kernel``) that the per-mover kernel tests do not reach, once per mover, bit for bit against the movers' NumPy
restatements:

* more samples than grid rows (the grid has at most 65 535): n = 65 536 + 3 samples of a 4 x 4 x 3 frame (48 bytes, three
  whole groups: the vector path; the translate onto a 4 x 8 x 3 canvas), period 5 with an index.  Samples 65 535 ... are
  the second trip of the sample loop of grid rows 0 ...; every sample has parameters of its own, and those of the second
  trip differ from those of the rows' first trip.
* a frame of more than 4 x 64 x 256 = 65 536 groups (the grid has at most 64 blocks of 256 threads, a thread takes 4 groups
  per trip): n = 2 samples of 256 x 512 x 9 (73 728 groups; the translate onto 264 x 520 x 9: 77 220).  The group loop
  takes a second trip in which only the first of a thread's four groups exists.

One launch per case, ``out`` on the 16-byte grid between guard bytes."""
import numpy as np
import pytest
import torch

from tests.test_gpu_cutout import cut_nhwc
from tests.test_gpu_random_shift import shifted
from tests.test_gpu_translate import translate_nhwc

pytestmark = pytest.mark.gpu

GUARD, GUARD_BYTE = 256, 0xA5
GRID_ROWS = 65535
N_MANY = 65536 + 3
PAD = 2            # of the shift in the many-samples case
BIG = (256, 512, 9)
BIG_CANVAS = (264, 520)
BOUNDARY = 65536 * 16  # first byte of the group loop's second trip


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _many_params(mover, rs):
    """Per-sample parameters of N_MANY samples; a sample of the second trip gets those of its grid row's first sample
    moved on by one, so serving it with the first trip's parameters shows."""
    n, first, second = N_MANY, slice(0, N_MANY - GRID_ROWS), slice(GRID_ROWS, N_MANY)
    if mover == "shift":
        dy, dx = rs.randint(0, 2 * PAD + 1, n), rs.randint(0, 2 * PAD + 1, n)
        dy[second] = (dy[first] + 1) % (2 * PAD + 1)
        return [_i32(dy), _i32(dx)]
    if mover == "cutout":
        y0, x0, bh, bw = rs.randint(0, 3, n), rs.randint(0, 3, n), rs.randint(1, 3, n), rs.randint(1, 3, n)
        rgb = rs.randint(0, 2 ** 24, n)
        y0[second] = (y0[first] + 1) % 3
        return [_i32(y0), _i32(x0), _i32(bh | (bw << 16)), _i32(rgb)]
    tx = rs.randint(0, 5, n)
    tx[second] = (tx[first] + 1) % 5
    return [_i32(np.zeros(n)), _i32(tx)]


def _big_params(mover):
    H, W, C = BIG
    if mover == "shift":  # a corner of the offset range and the centre (a pure copy), pad 4
        return [_i32([8, 4]), _i32([0, 4])]
    if mover == "cutout":
        rb = W * C
        y, xb = BOUNDARY // rb, BOUNDARY % rb  # the boundary lies in row y, xb bytes into it
        assert 8 < y < H - 8 and 30 * C < xb < rb - 30 * C
        # a box around the boundary byte, and full-width rows around it (the fill runs on across rows and the boundary)
        y0, x0, bh, bw = [y - 7, y - 1], [xb // C - 15, 0], [16, 4], [30, W]
        return [_i32(y0), _i32(x0), _i32(np.array(bh) | (np.array(bw) << 16)), _i32([0x0A6F03, 0x7FC811E2])]
    return [_i32([8, 0]), _i32([8, 3])]


def _restated(mover, src, params, pad, canvas):
    if mover == "shift":
        return shifted(src, params[0], params[1], pad)
    if mover == "cutout":
        return cut_nhwc(src, *params)
    return translate_nhwc(src, params[0], params[1], *canvas)


@pytest.mark.parametrize("case", ["many_samples", "big_frame"])
@pytest.mark.parametrize("mover", ["shift", "cutout", "translate"])
def test_second_trip_of_the_skeletons_loops(mover, case):
    from curla_amd import ops
    rs = np.random.RandomState(len(mover) + len(case))
    if case == "many_samples":
        (H, W, C), canvas, n, pad, ring_rows, rows = (4, 4, 3), (4, 8), N_MANY, PAD, 8, np.array([6, 0, 3, 6, 7])
        params = _many_params(mover, rs)
    else:
        (H, W, C), canvas, n, pad, ring_rows, rows = BIG, BIG_CANVAS, 2, 4, 3, np.array([2, 0])
        params = _big_params(mover)
    Ho, Wo = canvas if mover == "translate" else (H, W)
    frame, oframe, period = H * W * C, Ho * Wo * C, len(rows)
    assert oframe % 16 == 0 and frame >= 16
    assert (n > GRID_ROWS) if case == "many_samples" else (oframe // 16 > 65536)
    host = rs.randint(1, 256, (ring_rows, H, W, C), dtype=np.uint8)  # (no zero byte: a margin byte is told from a pixel)
    store = torch.zeros(ring_rows * frame + 32, dtype=torch.uint8, device="cuda")
    ring = store[:ring_rows * frame].view(ring_rows, H, W, C)
    ring.copy_(torch.from_numpy(host))
    want = _restated(mover, host[rows[np.arange(n) % period]], params, pad, canvas)
    assert want.shape == (n, Ho, Wo, C)
    if case == "many_samples":  # the second trip's samples are not their grid rows' first samples over again
        assert all(not np.array_equal(want[s], want[s - GRID_ROWS]) for s in range(GRID_ROWS, n))
    elif mover == "cutout":     # both boxes cover the boundary byte, and bytes on either side of it
        flat = want.reshape(n, -1) != host[rows].reshape(n, -1)
        assert flat[:, BOUNDARY - 64:BOUNDARY].any(axis=1).all() and flat[:, BOUNDARY:BOUNDARY + 64].any(axis=1).all()
    idx = torch.from_numpy(rows.astype(np.int64)).cuda()
    d = [torch.from_numpy(a).cuda() for a in params]
    buf = torch.full((GUARD + n * oframe + GUARD,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
    out = buf[GUARD:GUARD + n * oframe].view(n, Ho, Wo, C)
    assert out.data_ptr() % 16 == 0
    if mover == "shift":
        ops.random_shift_u8(ring, idx, period, d[0], d[1], pad, n, out)
    elif mover == "cutout":
        ops.cutout_u8(ring, idx, period, *d, n, out)
    else:
        ops.translate_u8(ring, idx, period, d[0], d[1], n, out)
    got = buf.cpu()
    assert torch.equal(got[GUARD:GUARD + n * oframe].view(n, Ho, Wo, C), torch.from_numpy(want))
    assert bool((got[:GUARD] == GUARD_BYTE).all()) and bool((got[GUARD + n * oframe:] == GUARD_BYTE).all())
    assert torch.equal(ring.cpu(), torch.from_numpy(host)) and not bool(store[-32:].any())  # the source is only read
