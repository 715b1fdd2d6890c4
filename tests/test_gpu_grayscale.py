"""``RandomGrayscale`` on the device: ``curla_grayscale_u8`` against the integer formula in NumPy, and the replay buffer's
routes, whole updates and update graphs through the checks of tests/test_gpu_dihedral.py.  Everything is bit for bit
(``torch.equal``): the mix is integer arithmetic on bytes."""
import numpy as np
import pytest
import torch

from tests.test_gpu_dihedral import (GUARD, GUARD_BYTE, check_buffer_route, check_graph_replay_is_eager,
                                     check_updates_are_those_of_host_transformed_pixels)

pytestmark = pytest.mark.gpu


def grey_nhwc(frames, flags):
    """The restatement on uint8 [n, H, W, 3k]: where flags[s] != 0 every triplet (R, G, B) becomes (g, g, g) with
    g = (77 R + 150 G + 29 B + 128) >> 8."""
    out = frames.copy()
    n, H, W, C = frames.shape
    t = frames.reshape(n, H, W, C // 3, 3).astype(np.int64)
    g = ((77 * t[..., 0] + 150 * t[..., 1] + 29 * t[..., 2] + 128) >> 8).astype(np.uint8)
    for s in range(n):
        if flags[s]:
            out[s] = np.repeat(g[s], 3, axis=-1)
    return out


GEOMETRIES = [  # (H, W, C)
    (5, 7, 3),      # 105 bytes: no vector path
    (2, 8, 3),      # three groups; triplets straddle both of their borders
    (8, 8, 9),
    (4, 4, 6),
    (1, 5, 3),      # a frame shorter than a group
    (84, 84, 9),    # the training geometry
]
FLAGS = [0, 1, -1, 2, 1, 0, 0x40000000]


@pytest.mark.parametrize("geo", GEOMETRIES, ids=["%dx%dx%d" % g for g in GEOMETRIES])
def test_kernel_equals_the_restatement(geo):
    """Flags 0, 1, -1 and 2 (any non-zero word counts); some input pixels are grey already and stay what they are.  ``out``
    on and one byte off a 16-byte boundary, between guard bytes; rows given with a repeat, rows None with period n and
    with period < n; ring row 0 is the start of its allocation."""
    from curla_amd import ops
    H, W, C = geo
    frame = H * W * C
    n = len(FLAGS)
    rows_in_ring = n + 3
    rs = np.random.RandomState(H * W + C)
    host = rs.randint(0, 256, (rows_in_ring, H, W, C), dtype=np.uint8)
    grey_px = rs.rand(rows_in_ring, H, W, C // 3) < 0.25  # a quarter of the triplets are (v, v, v) already
    trip = host.reshape(rows_in_ring, H, W, C // 3, 3)
    trip[grey_px] = trip[grey_px][:, :1]
    assert np.array_equal(grey_nhwc(host, [1] * rows_in_ring).reshape(trip.shape)[grey_px], trip[grey_px])
    store = torch.zeros(rows_in_ring * frame + 32, dtype=torch.uint8, device="cuda")
    ring = store[:rows_in_ring * frame].view(rows_in_ring, H, W, C)  # ring row 0 = the first bytes of its allocation
    assert ring.data_ptr() == store.data_ptr()
    ring.copy_(torch.from_numpy(host))
    d_flags = torch.from_numpy(np.array(FLAGS, dtype=np.int32)).cuda()
    period = n - 2
    rows = rs.randint(0, rows_in_ring, size=period)
    rows[0] = rows[1] = 0  # ring row 0 is a source, copied (sample 0) and greyed (sample 1): nothing lies in front of it
    rows[-1] = rows[2]  # a repeat
    rows[3] = rows_in_ring - 1  # the last row: only the slack lies behind it
    cases = [(torch.from_numpy(rows.astype(np.int64)).cuda(), period, rows[np.arange(n) % period]),
             (None, n, np.arange(n)),
             (None, period, np.arange(n) % period)]
    for idx, per, src_rows in cases:
        want_np = grey_nhwc(host[src_rows], FLAGS)
        want = torch.from_numpy(want_np)
        for lead in (0, 1):  # out on a 16-byte boundary, and one byte off it (no vector path)
            buf = torch.full((GUARD + lead + n * frame + GUARD,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
            out = buf[GUARD + lead:GUARD + lead + n * frame].view(n, H, W, C)
            assert (out.data_ptr() % 16 == 0) == (lead == 0)
            ops.grayscale_u8(ring, idx, per, d_flags, n, out)
            got = buf.cpu()
            assert torch.equal(got[GUARD + lead:GUARD + lead + n * frame].view(n, H, W, C), want), (per, lead)
            assert bool((got[:GUARD + lead] == GUARD_BYTE).all()) and bool((got[GUARD + lead + n * frame:] == GUARD_BYTE).all())
        for s, f in enumerate(FLAGS):
            if f == 0:
                assert np.array_equal(want_np[s], host[src_rows[s]])
            else:
                assert np.array_equal(want_np[s], grey_nhwc(host[src_rows[s]][None], [1])[0])
                assert np.array_equal(grey_nhwc(want_np[s][None], [1])[0], want_np[s])  # idempotent
    assert torch.equal(ring.cpu(), torch.from_numpy(host)) and not bool(store[-32:].any())  # the source is only read


def test_kernel_refuses_bad_arguments_before_any_launch():
    from curla_amd import _lib
    lib = _lib.load()
    ring = torch.zeros(4 * 4 * 3 + 32, dtype=torch.uint8, device="cuda")
    w = torch.zeros(8, dtype=torch.int32, device="cuda")
    out = torch.full((4 * 4 * 4,), 0x5A, dtype=torch.uint8, device="cuda")
    P = w.data_ptr()

    def rc(frames=ring.data_ptr(), idx=None, period=1, grey=P, n=1, chw=(3, 4, 4), o=out.data_ptr()):
        return lib.curla_grayscale_u8(frames, idx, period, grey, n, *chw, o, None)
    assert rc(o=None) == -1 and rc(frames=None) == -1 and rc(grey=None) == -1     # null pointers
    assert rc(grey=P + 1) == -1 and rc(grey=P + 2) == -1                          # the words off their 4 bytes
    assert rc(idx=P + 4) == -1                                                    # idx off its 8 bytes
    assert rc(n=0) == -1 and rc(period=0) == -1
    assert rc(chw=(0, 4, 4)) == -1 and rc(chw=(3, 0, 4)) == -1 and rc(chw=(3, 4, 0)) == -1
    assert rc(chw=(4, 4, 3)) == -1 and rc(chw=(1, 4, 4)) == -1 and rc(chw=(5, 4, 4)) == -1   # C is no multiple of 3
    assert rc(chw=(3, 2 ** 15, 2 ** 15)) == -3      # H W C = 3 * 2^30: over the 31 bits of the byte arithmetic
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all())                # nothing was launched
    ring.fill_(7)
    assert rc() == 0                                # ... and the same arguments, all valid, are taken
    torch.cuda.synchronize()
    assert bool((out[:48] == 7).all()) and bool((out[48:] == 0x5A).all())


ROUTES = [((12, 12), r) for r in ("plain", "dedup", "n_step")] + \
         [((11, 13), r) for r in ("plain", "dedup", "two_allocations", "n_step")]


@pytest.mark.parametrize("hw,route", ROUTES, ids=["%dx%d-%s" % (h[0], h[1], r) for h, r in ROUTES])
def test_buffer_routes_give_the_restated_bytes(hw, route):
    """(A frame of 9 x 12 x 12 bytes is a multiple of 4, so both rings always share an allocation there: the rings in two
    allocations run at (9, 11, 13).)"""
    check_buffer_route("grayscale", hw, route)


def test_three_updates_are_the_updates_of_the_host_greyed_pixels():
    check_updates_are_those_of_host_transformed_pixels("grayscale", (40, 44))


def test_graph_replay_is_the_eager_update_bit_for_bit():
    check_graph_replay_is_eager("grayscale")
