"""``Compose(move, paint)`` on the device: ``curla_move_cutout_u8`` -- the crop, shift and translate movers with the
cutout's box painted over their output in one launch -- against a NumPy restatement of clamp, move and paint, against the
existing single-purpose entry points, the replay buffer's four routes, a whole update against the update of frames
composed on the host, update graphs and batched acting.  Everything is bit for bit (``torch.equal``): the kernel only
moves and replaces bytes, and the update downstream of it is the existing uint8-ring update."""
import collections

import numpy as np
import pytest
import torch

from tests.test_gpu_agent import HP, NullLogger
from tests.test_gpu_graph_aug import _episode, _run, _state
from tests.test_gpu_random_shift import _HostShiftedBuffer

pytestmark = pytest.mark.gpu

GUARD, GUARD_BYTE = 256, 0xA5
CROP, SHIFT, TRANSLATE = 0, 1, 2


# ------------------------------------------------------------------------------------------------ 1. the kernel
def moved_nhwc(frames, move, a, b, pad, Ho, Wo):
    """The movers' restatement on uint8 [n, H, W, C] -> [n, Ho, Wo, C], with the kernels' clamp rules."""
    n, H, W, C = frames.shape
    out = np.zeros((n, Ho, Wo, C), dtype=np.uint8)
    clamp = lambda v, lo, hi: min(max(int(v), lo), hi)  # noqa: E731
    for s in range(n):
        if move == CROP:
            h1, w1 = clamp(a[s], 0, H - Ho), clamp(b[s], 0, W - Wo)
            out[s] = frames[s, h1:h1 + Ho, w1:w1 + Wo]
        elif move == SHIFT:
            oy, ox = clamp(a[s], 0, 2 * pad) - pad, clamp(b[s], 0, 2 * pad) - pad
            ys, xs = np.clip(np.arange(H) + oy, 0, H - 1), np.clip(np.arange(W) + ox, 0, W - 1)
            out[s] = frames[s][ys[:, None], xs[None, :]]
        else:
            ty, tx = clamp(a[s], 0, Ho - H), clamp(b[s], 0, Wo - W)
            out[s, ty:ty + H, tx:tx + W] = frames[s]
    return out


def painted_nhwc(mid, y0, x0, size, rgb):
    """The cutout's restatement over [n, Ho, Wo, C], the box clamped as ``cutout_u8_kernel`` clamps it."""
    out = mid.copy()
    n, Ho, Wo, C = mid.shape
    chan = np.arange(C) % 3
    for s in range(n):
        sz, col = int(size[s]) & 0xFFFFFFFF, int(rgb[s]) & 0xFFFFFFFF
        yc, xc = min(max(int(y0[s]), 0), Ho), min(max(int(x0[s]), 0), Wo)
        bh, bw = min(sz & 0xFFFF, Ho - yc), min(sz >> 16, Wo - xc)
        colour = np.array([col & 0xFF, (col >> 8) & 0xFF, (col >> 16) & 0xFF], dtype=np.uint8)
        out[s, yc:yc + bh, xc:xc + bw] = colour[chan]
    return out


def _boxes(Ho, Wo, rs):
    """(y0, x0, bh, bw): empty, 1 x 1 in each corner, the whole frame, flush with each edge, a full-width band and a
    full-height column, out of range on either side (the clamp), and five random ones."""
    h2, w2 = max(1, Ho // 2), max(1, Wo // 2)
    boxes = [(2, 3, 0, 0), (1, 1, 3, 0), (1, 1, 0, 3),
             (0, 0, 1, 1), (0, Wo - 1, 1, 1), (Ho - 1, 0, 1, 1), (Ho - 1, Wo - 1, 1, 1),
             (0, 0, Ho, Wo),
             (0, 1, h2, w2), (Ho - h2, 1, h2, w2), (1, 0, h2, w2), (1, Wo - w2, h2, w2),
             (1, 0, h2, Wo), (0, 1, Ho, w2),
             (-2, -3, 5, 5), (Ho - 1, Wo - 1, 0x7FFF, 0x7FFF), (Ho + 5, 0, 3, 3), (0, Wo + 1, 3, 3), (-0x7FFF, 1, 0x7FFF, 2),
             (0, 0, 0x7FFF, 0x7FFF)]
    for _ in range(5):
        bh, bw = rs.randint(1, Ho + 1), rs.randint(1, Wo + 1)
        boxes.append((rs.randint(0, Ho - bh + 1), rs.randint(0, Wo - bw + 1), bh, bw))
    return boxes


def _offsets(move, H, W, Ho, Wo, pad):
    """Both ends of both ranges, the middle, and values out of range on either side."""
    my, mx = {CROP: (H - Ho, W - Wo), SHIFT: (2 * pad, 2 * pad), TRANSLATE: (Ho - H, Wo - W)}[move]
    return [(0, 0), (my, mx), (0, mx), (my, 0), (my // 2, mx // 2), (-3, 0x7FFF), (0x7FFF, -3), (my + 1, mx + 1)]


GEOMETRIES = [  # move, C, (H, W), (Ho, Wo), pad, lead
    (CROP, 9, (16, 20), (12, 12), 0, 0),       # vector path; 108-byte rows, every row boundary straddled
    (CROP, 3, (10, 8), (8, 4), 0, 0),          # 12-byte rows: groups over three rows
    (CROP, 9, (9, 8), (7, 5), 0, 0),           # 315 bytes: byte path
    (CROP, 9, (16, 20), (12, 12), 0, 1),       # out one byte off the 16-byte grid: byte path
    (CROP, 9, (12, 12), (12, 12), 0, 0),       # H == Ho, W == Wo
    (TRANSLATE, 9, (10, 12), (16, 14), 0, 0),  # straddling vector groups
    (TRANSLATE, 9, (12, 14), (12, 14), 0, 0),  # Wo == W
    (SHIFT, 9, (12, 12), (12, 12), 2, 0),
    (SHIFT, 4, (6, 6), (6, 6), 1, 0),          # C % 3 != 0; 144 bytes, vector path
    # beyond the issue's list: a crop as wide as the frame and a canvas as wide as the frame on the vector path (the two
    # runs of a straddling group are one run of the source; 12 x 14 x 9 above is 94.5 groups, so it goes byte by byte)
    (CROP, 9, (16, 12), (12, 12), 0, 0),
    (TRANSLATE, 9, (10, 16), (14, 16), 0, 0),
]


@pytest.mark.parametrize("move,C,hw,out_hw,pad,lead", GEOMETRIES,
                         ids=["%s-%dx%dx%d-%dx%d%s" % (("crop", "shift", "translate")[m], h[0], h[1], c, o[0], o[1], "-off1" * l)
                              for m, c, h, o, _, l in GEOMETRIES])
def test_kernel_equals_the_restatement(move, C, hw, out_hw, pad, lead):
    from curla_amd import ops
    (H, W), (Ho, Wo) = hw, out_hw
    frame, oframe = H * W * C, Ho * Wo * C
    rs = np.random.RandomState(7 * H * W + C + Wo + move)
    boxes, offs = _boxes(Ho, Wo, rs), _offsets(move, H, W, Ho, Wo, pad)
    pairs = [(bx, offs[s % len(offs)]) for s, bx in enumerate(boxes)]
    # ... and the whole frame, the full-width band, the full-height column, a clamped box and a random one under EVERY offset
    pairs += [(boxes[k], o) for k in (7, 12, 13, 15, 20) for o in offs]
    boxes, n = [bx for bx, _ in pairs], len(pairs)
    a = np.array([o[0] for _, o in pairs], dtype=np.int32)
    b = np.array([o[1] for _, o in pairs], dtype=np.int32)
    y0, x0 = (np.array([bx[k] for bx in boxes], dtype=np.int32) for k in (0, 1))
    size = np.array([bx[2] | (bx[3] << 16) for bx in boxes], dtype=np.int32)
    rgb = rs.randint(1, 256, (n, 3))
    rgb = (rgb[:, 0] | (rgb[:, 1] << 8) | (rgb[:, 2] << 16) | (0x7F << 24)).astype(np.int32)  # (the top byte is ignored)
    rgb[::3] = 0  # black and coloured boxes
    rows_in_ring = n + 3
    host = rs.randint(1, 256, (rows_in_ring, H, W, C), dtype=np.uint8)
    store = torch.zeros(rows_in_ring * frame + 32, dtype=torch.uint8, device="cuda")
    ring = store[:rows_in_ring * frame].view(rows_in_ring, H, W, C)  # ring row 0 = the first bytes of its allocation
    assert ring.data_ptr() == store.data_ptr()
    ring.copy_(torch.from_numpy(host))
    dev = lambda v: torch.from_numpy(v).cuda()  # noqa: E731
    d_a, d_b, d_box = dev(a), dev(b), tuple(dev(v) for v in (y0, x0, size, rgb))
    period = n - 2
    rows = rs.randint(0, rows_in_ring, size=period)
    rows[0], rows[1], rows[-1] = 0, rows_in_ring - 1, 0  # ring row 0 and the last ring row are sources; a repeat
    cases = [(dev(rows.astype(np.int64)), period, rows[np.arange(n) % period]), (None, n, np.arange(n))]
    for idx, per, src_rows in cases:
        mid = moved_nhwc(host[src_rows], move, a, b, pad, Ho, Wo)
        for box, want in ((d_box, painted_nhwc(mid, y0, x0, size, rgb)), (None, mid)):  # (None: size == NULL)
            buf = torch.full((GUARD + lead + n * oframe + GUARD,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
            out = buf[GUARD + lead:GUARD + lead + n * oframe].view(n, Ho, Wo, C)
            assert (out.data_ptr() % 16 == 0) == (lead == 0)
            ops.move_cutout_u8(ring, idx, per, move, d_a, d_b, pad, box, n, out)
            got = buf.cpu()
            assert torch.equal(got[GUARD + lead:GUARD + lead + n * oframe].view(n, Ho, Wo, C), torch.from_numpy(want)), \
                (per, box is None)
            assert bool((got[:GUARD + lead] == GUARD_BYTE).all()) and bool((got[GUARD + lead + n * oframe:] == GUARD_BYTE).all())
    assert torch.equal(ring.cpu(), torch.from_numpy(host)) and not bool(store[-32:].any())  # the source is only read
    painted = painted_nhwc(mid, y0, x0, size, rgb)
    assert all(np.array_equal(painted[s], mid[s]) for s in (0, 1, 2, 16, 17))  # empty boxes are plain moves
    assert (painted[7] == np.array([rgb[7] & 0xFF, (rgb[7] >> 8) & 0xFF, (rgb[7] >> 16) & 0xFF])[np.arange(C) % 3]).all()
    assert sum(not np.array_equal(painted[s], mid[s]) for s in range(n)) >= 15 and n == 65


def _ring(rows, H, W, C, seed):
    host = np.random.RandomState(seed).randint(1, 256, (rows, H, W, C), dtype=np.uint8)
    store = torch.zeros(host.size + 32, dtype=torch.uint8, device="cuda")
    ring = store[:host.size].view(host.shape)
    ring.copy_(torch.from_numpy(host))
    return ring, store


def test_no_box_and_an_empty_box_are_the_existing_movers_and_a_still_move_is_the_cutout():
    from curla_amd import ops
    n, C = 12, 9
    rs = np.random.RandomState(3)
    i32 = lambda v: torch.from_numpy(np.asarray(v, dtype=np.int32)).cuda()  # noqa: E731
    idx = torch.from_numpy(rs.randint(0, 6, 5).astype(np.int64)).cuda()
    y0, x0 = i32(rs.randint(0, 6, n)), i32(rs.randint(0, 6, n))
    size, rgb = i32(rs.randint(1, 7, n) | (rs.randint(1, 7, n) << 16)), i32(rs.randint(0, 1 << 24, n))
    empty = i32([0, 3, 3 << 16, 0] * 3)  # bh or bw of zero
    # move 1 against curla_random_shift_u8, move 2 against curla_translate_u8: no box, and an empty box
    for move, (H, W), (Ho, Wo), pad in ((SHIFT, (12, 12), (12, 12), 2), (TRANSLATE, (10, 12), (16, 14), 0)):
        ring, _ = _ring(6, H, W, C, 5)
        a, b = i32(rs.randint(-1, 7, n)), i32(rs.randint(-1, 7, n))
        want = torch.zeros((n, Ho, Wo, C), dtype=torch.uint8, device="cuda")
        if move == SHIFT:
            ops.random_shift_u8(ring, idx, 5, a, b, pad, n, want)
        else:
            ops.translate_u8(ring, idx, 5, a, b, n, want)
        assert bool(want.any())
        for box in (None, (y0, x0, empty, rgb)):
            got = torch.zeros_like(want)
            ops.move_cutout_u8(ring, idx, 5, move, a, b, pad, box, n, got)
            assert torch.equal(got, want), (move, box is None)
        got = torch.zeros_like(want)
        ops.move_cutout_u8(ring, idx, 5, move, a, b, pad, (y0, x0, size, rgb), n, got)
        assert not torch.equal(got, want)  # (a real box does paint)
    # moves that move nothing -- a shift of pad 0, a crop and a translate of the frame's own size -- against curla_cutout_u8
    for C, (H, W) in ((9, (12, 12)), (4, (6, 6)), (9, (9, 8))):
        ring, _ = _ring(6, H, W, C, 6)
        want = torch.zeros((n, H, W, C), dtype=torch.uint8, device="cuda")
        ops.cutout_u8(ring, idx, 5, y0, x0, size, rgb, n, want)
        zero = i32(np.zeros(n))
        for move in (CROP, SHIFT, TRANSLATE):
            got = torch.zeros_like(want)
            ops.move_cutout_u8(ring, idx, 5, move, zero, zero, 0, (y0, x0, size, rgb), n, got)
            assert torch.equal(got, want), (move, C)


def test_kernel_refuses_bad_arguments_before_any_launch():
    from curla_amd import _lib
    lib = _lib.load()
    ring = torch.zeros(4 * 6 * 6 * 3 + 32, dtype=torch.uint8, device="cuda")
    w = torch.zeros(8, dtype=torch.int32, device="cuda")
    out = torch.full((8 * 8 * 3,), 0x5A, dtype=torch.uint8, device="cuda")
    P = w.data_ptr()
    fits = {CROP: (4, 4), SHIFT: (6, 6), TRANSLATE: (8, 8)}

    def rc(move=SHIFT, frames=ring.data_ptr(), idx=None, period=1, a=P, b=P, pad=1, y0=P, x0=P, size=P, rgb=P, n=1,
           chw=(3, 6, 6), hw=None, o=out.data_ptr()):
        return lib.curla_move_cutout_u8(frames, idx, period, move, a, b, pad, y0, x0, size, rgb, n, *chw,
                                        *(hw or fits.get(move, (6, 6))), o, None)
    assert rc(move=3) == -1 and rc(move=-1) == -1                                                   # unknown move
    assert rc(o=None) == -1 and rc(frames=None) == -1 and rc(a=None) == -1 and rc(b=None) == -1     # null pointers
    assert rc(y0=None) == -1 and rc(x0=None) == -1 and rc(rgb=None) == -1                           # ... of a box
    assert rc(a=P + 2) == -1 and rc(b=P + 1) == -1 and rc(size=P + 2) == -1 and rc(rgb=P + 1) == -1  # odd pointers
    assert rc(idx=P + 4) == -1                                                                      # idx off its 8 bytes
    assert rc(n=0) == -1 and rc(n=-1) == -1 and rc(period=0) == -1 and rc(chw=(0, 6, 6)) == -1 and rc(pad=-1) == -1
    assert rc(move=CROP, pad=-1) == -1 and rc(move=TRANSLATE, pad=-1) == -1
    assert rc(move=CROP, hw=(7, 4)) == -1 and rc(move=CROP, hw=(4, 7)) == -1                        # a crop that grows
    assert rc(move=SHIFT, hw=(6, 5)) == -1 and rc(move=SHIFT, hw=(7, 6)) == -1                      # a shift that resizes
    assert rc(move=TRANSLATE, hw=(5, 8)) == -1 and rc(move=TRANSLATE, hw=(8, 5)) == -1              # a canvas too small
    assert rc(move=CROP, hw=(0, 4)) == -1
    assert rc(move=SHIFT, pad=2 ** 29) == -3                                     # 2 pad C over 30 bits
    assert rc(move=SHIFT, chw=(3, 2 ** 15, 2 ** 15), hw=(2 ** 15, 2 ** 15)) == -3  # H W C over 31 bits
    assert rc(move=TRANSLATE, hw=(2 ** 15, 2 ** 15)) == -3                         # Ho Wo C over 31 bits
    assert rc(move=TRANSLATE, chw=(1, 1, 4), hw=(1, 2 ** 30)) == -3                # an output row of 2^30 bytes
    assert rc(move=CROP, chw=(3, 2 ** 15, 2 ** 15), hw=(4, 4)) == -3               # the crop's SOURCE frame over 31 bits
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all())  # nothing was launched
    for move in (CROP, SHIFT, TRANSLATE):  # ... and the same arguments, all valid, are taken, with and without a box
        for size in (P, None):
            out.fill_(0x5A)
            assert rc(move=move, size=size) == 0
            torch.cuda.synchronize()
            nb = 3 * fits[move][0] * fits[move][1]
            assert not bool((out[:nb] == 0x5A).any()) and bool((out[nb:] == 0x5A).all())


# ------------------------------------------------------------------------------------------------ 2. buffer routes
C9, IN_HW, B8, CAP, N_FILL = 9, (34, 40), 8, 32, 28
PAIRS = {"random_crop+cutout_color": (28, 34), "random_shift+cutout": None, "translate+cutout_color": (40, 48)}


def _augmentor(name, in_hw=IN_HW, out_hw="pair", **kw):
    """(boxes of 4 .. 16 a side unless told otherwise: the default 10 .. 30 does not fit the smaller frames here)"""
    import curla_amd
    return curla_amd.make_augmentor(name, in_hw, PAIRS[name] if out_hw == "pair" else out_hw,
                                    **{"pad": 3, "min_cut": 4, "max_cut": 16, **kw})


def _filled(name, in_hw=IN_HW, out_hw="pair", capacity=CAP, n_fill=N_FILL, cls=None, aug_kw=None, **kw):
    import curla_amd
    aug = _augmentor(name, in_hw, out_hw, **(aug_kw or {}))
    rb = (cls or curla_amd.ReplayBuffer)((C9,) + in_hw, (2,), capacity, B8, torch.device("cuda"), aug, **kw)
    ep = _episode(n_fill, C9 // 3, in_hw, 6)
    rb.add_batch(*ep)
    return rb, ep


def _injected(rb, n_fill, seed):
    """(idxs, offs [18, B]) with a repeated row and words drawn by the augmentor from a private seed."""
    B = rb.batch_size
    keep = np.random.get_state()
    np.random.seed(seed)
    idxs = np.random.randint(0, n_fill, size=B)
    idxs[1] = idxs[0]
    offs = np.zeros((18, B), dtype=np.int32)
    for j in range(3):
        for r, word in enumerate(rb.augmentor.draw_index_words(B)):
            offs[6 * (r // 2) + 2 * j + r % 2] = word
    np.random.set_state(keep)
    return idxs, offs


def _host_composed(aug, stacks, words):
    """(n, C, H, W) stacks through the augmentor's host functions with the six recorded words of a tensor."""
    import curla_amd
    a, b, y0, x0, size, rgb = (np.asarray(w).astype(np.int64) for w in words)
    move = aug.move
    if isinstance(move, curla_amd.RandomCrop):
        oh, ow = move.output_shape
        mid = np.stack([s[:, a[i]:a[i] + oh, b[i]:b[i] + ow] for i, s in enumerate(stacks)])
    elif isinstance(move, curla_amd.RandomShift):
        mid = move.shift(stacks, a, b)
    else:
        mid = move.translate(stacks, a, b)
    colours = np.stack([rgb & 0xFF, (rgb >> 8) & 0xFF, (rgb >> 16) & 0xFF], 1) if aug.paint.color else None
    return aug.paint.cut(mid, y0, x0, size & 0xFFFF, size >> 16, colours)


def _restated(aug, stored, idxs, offs, next_rows=None):
    """(obs | next_obs | pos) as uint8 [3B, Ho, Wo, C]; ``stored`` = (obs stacks, -, -, next_obs stacks)."""
    next_rows = idxs if next_rows is None else next_rows
    outs = [_host_composed(aug, stacks, [offs[6 * (r // 2) + 2 * j + r % 2] for r in range(6)])
            for j, stacks in enumerate((stored[0][idxs], stored[3][next_rows], stored[0][idxs]))]
    return np.ascontiguousarray(np.concatenate(outs).transpose(0, 2, 3, 1))


def _check_refs(rb, sample, want):
    B = rb.batch_size
    obs, _, _, nxt, _, kw = sample
    scratch = obs.src
    assert scratch.dtype == torch.uint8 and tuple(scratch.shape) == tuple(want.shape)
    assert torch.equal(scratch.cpu(), torch.from_numpy(want))
    for ref, row0 in ((obs, 0), (nxt, B), (kw["obs_pos"], 2 * B)):
        assert ref.src.data_ptr() == scratch.data_ptr() and ref.is_u8 == 1 and ref.B == B
        assert ref.idx.tolist() == list(range(row0, row0 + B)) and not bool(ref.h1.any()) and not bool(ref.w1.any())
        assert (ref.Hc, ref.Wc) == (ref.Hs, ref.Ws) == tuple(rb.augmentor.output_shape)
        ref.check()
    pair, second = obs.pair
    assert second is nxt and pair.B == 2 * B and pair.idx.tolist() == list(range(2 * B)) and not bool(pair.h1.any())


def _routes_agree(rb, ep, n_fill, route):
    B, aug = rb.batch_size, rb.augmentor
    oh, ow = aug.output_shape
    oframe = C9 * oh * ow
    assert rb._scratch_frame() == oframe and rb._shift_store.stride(0) % 256 == 0
    stored = (rb.stacks(0, n_fill, 0), None, None, rb.stacks(0, n_fill, 1))
    assert np.array_equal(stored[0], ep[0]) and np.array_equal(stored[3], ep[3])  # the stored frames stay (C, H, W)
    next_of = lambda idxs: None  # noqa: E731
    if route == "n_step":  # next_obs comes from the bootstrap rows: up to two flagged steps further on
        def next_of(idxs):
            last = []
            for r in idxs:
                m = 1
                while m < 3 and rb._cont_h[r]:
                    r, m = (r + 1) % rb.capacity, m + 1
                last.append(r)
            return np.array(last)
    for seed, injected in ((11, True), (13, False)):
        if injected:
            idxs, offs = _injected(rb, n_fill, seed)
            sample = rb.sample_cpc_refs((idxs, offs))
        else:  # the buffer's own draw, recorded by drawing it once more from the same seed
            np.random.seed(seed)
            sample = rb.sample_cpc_refs()
            after = np.random.get_state()
            np.random.seed(seed)
            idxs, offs = rb.draw_indices()
            now = np.random.get_state()
            assert np.array_equal(after[1], now[1]) and after[2] == now[2] and offs.shape == (18, B)
        last = next_of(idxs)
        want = _restated(aug, stored, idxs, offs, last)
        _check_refs(rb, sample, want)
        assert torch.equal(sample[1].cpu(), torch.from_numpy(ep[1][idxs]))
        assert not bool(rb._shift_store[rb._sample_slot][3 * B * oframe:].any())  # the slack is never written
    plain = offs.copy()
    plain[12:] = 0  # no boxes
    assert bool((want != _restated(aug, stored, idxs, plain, last)).any())  # (the boxes did paint)
    o, _, _, nx, _, kwargs = rb.sample_cpc((idxs, offs))
    want_f = torch.from_numpy(want.transpose(0, 3, 1, 2).astype(np.float32))
    for t, j in ((o, 0), (nx, 1), (kwargs["obs_pos"], 2)):
        assert t.dtype == torch.float32 and tuple(t.shape) == (B, C9, oh, ow)
        assert torch.equal(t.cpu(), want_f[j * B:(j + 1) * B])


@pytest.mark.parametrize("name", list(PAIRS))
@pytest.mark.parametrize("route", ["plain", "dedup", "two_launches", "n_step"])
def test_buffer_routes_give_the_host_restatement(route, name):
    """9 x 34 x 40 frames, B = 8, capacity 32.  Frames of 12240 bytes always put the second ring on a dword, so the route
    of rings in two allocations -- one launch per tensor -- is taken here by withdrawing the double ring from the buffer
    (``_both``: the only thing ``_sources`` asks); the test below runs it on a buffer that really has two allocations."""
    kw = dict(dedup_frames=True) if route == "dedup" else dict(n_step=3, discount=0.99) if route == "n_step" else {}
    rb, ep = _filled(name, **kw)
    assert rb._frame == C9 * IN_HW[0] * IN_HW[1]
    if route != "dedup":
        assert rb._both is not None
    if route == "two_launches":
        rb._both = None
    _routes_agree(rb, ep, N_FILL, route)


def test_rings_in_two_allocations_give_the_host_restatement():
    """(C, H, W) = (9, 11, 13): a frame of 1287 bytes and capacity 41 leave the second ring off a dword."""
    rb, ep = _filled("random_crop+cutout_color", in_hw=(11, 13), out_hw=(8, 9), capacity=41, n_fill=30,
                     aug_kw=dict(min_cut=2, max_cut=6))
    assert rb._both is None and not rb.graph_supported()
    _routes_agree(rb, ep, 30, "two_allocations")


# ------------------------------------------------------------------------------------------------ 3. a whole update
def _agent(seed, name, in_hw, out_hw="pair"):
    import curla_amd
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    np.random.seed(seed)
    aug = _augmentor(name, in_hw, out_hw)
    return curla_amd.CurlSacAgent((C9,) + tuple(aug.output_shape), (2,), torch.device("cuda"), aug, hidden_dim=64, **HP)


def test_an_update_is_the_update_of_the_host_composed_pixels():
    """Steps 0, 1, 2 from a ``random_crop+cutout_color`` buffer with injected draws against the same agent fed frames
    cropped and cut on the host (handles of the same structure over a host-made ring of cropped frames): the logged
    losses, gradient buffers, parameters, targets, Adam moments, log_alpha and the device generator end bit-identical --
    and differ from a run on the same crops without boxes."""
    import curla_amd
    name, B, in_hw, out_hw, n_fill = "random_crop+cutout_color", 32, (40, 44), (32, 36), 200
    aug = _augmentor(name, in_hw, out_hw)
    ep = _episode(n_fill, C9 // 3, in_hw, 6)

    class Injected(curla_amd.ReplayBuffer):
        queue = collections.deque()

        def draw_indices(self):
            return self.queue.popleft()

    rb = Injected((C9,) + in_hw, (2,), 256, B, torch.device("cuda"), aug)
    rb.add_batch(*ep)
    draws = [_injected(rb, n_fill, 30 + s) for s in range(3)]
    Injected.queue.extend(draws)

    def unboxed(o):
        o = o.copy()
        o[12:] = 0
        return o
    scal = lambda i: (ep[1][i], ep[2][i], 1.0 - ep[4][i].astype(np.float32))  # noqa: E731
    batches = [(_restated(aug, ep, i, o),) + scal(i) for i, o in draws]
    plain = [(_restated(aug, ep, i, unboxed(o)),) + scal(i) for i, o in draws]
    runs = []
    for source in (rb, _HostShiftedBuffer(batches, B, out_hw), _HostShiftedBuffer(plain, B, out_hw)):
        agent, L = _agent(5, name, in_hw, out_hw), NullLogger()
        losses = []
        for step in range(3):
            agent.update(source, L, step)
            losses.append(dict(L.scalars))
        torch.cuda.synchronize()
        state = _state(agent, source)
        state["critic_grad"], state["actor_grad"] = agent._critic_gflat.cpu().clone(), agent._actor_gflat.cpu().clone()
        runs.append((state, losses))
    assert not Injected.queue
    (a, la), (b, lb), (c, _) = runs
    assert la == lb and len(la[2]) >= 4
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert float(a["critic_steps"][0]) == 3 and float(a["actor_steps"][0]) == 2
    assert not torch.equal(a["critic"], c["critic"])  # ... and the boxes did matter


# ------------------------------------------------------------------------------------------------ 4. update graphs
@pytest.mark.parametrize("dedup", [False, True], ids=["crop+cutout_color", "crop+cutout_color+dedup"])
def test_graph_replay_is_the_eager_update_bit_for_bit(dedup):
    """The protocol of tests/test_gpu_graph_aug.py: 14 mixed steps with log_interval 5 (0, 5, 10 log and run eagerly;
    1, 2 warm up; 3, 4, 6, 7 capture; 8, 9, 11, 12, 13 replay) of ``random_crop+cutout_color`` at (40, 44) -> (34, 37);
    the state compared includes NumPy's stream, torch's CPU generator and the device generator."""
    setup = dict(aug="random_crop+cutout_color", dedup_frames=dedup)
    eager, calls_e, logs_e, _, _ = _run(False, **setup)
    graph, calls_g, logs_g, agent, rb = _run(True, **setup)
    replayed = [8, 9, 11, 12, 13]
    assert tuple(rb.augmentor.output_shape) == (34, 37) and rb.obs_shape == (9, 40, 44) and rb.graph_supported()
    assert all(calls_e[s].get("curla_move_cutout_u8") == 1 and calls_e[s].get("curla_sample_stage") == 1 for s in range(14))
    assert all(calls_e[s].get("curla_gather_stacks", 0) == (2 if dedup else 0) for s in range(14))
    assert all(calls_e[s].get(k, 0) == 0 for s in range(14)
               for k in ("curla_random_shift_u8", "curla_cutout_u8", "curla_translate_u8"))
    assert [sum(calls_g[s].values()) for s in replayed] == [0] * len(replayed), calls_g
    assert all(sum(calls_g[s].values()) > 15 and calls_g[s].get("curla_move_cutout_u8", 0) >= 1
               for s in (0, 1, 2, 3, 4, 5, 6, 7, 10)), calls_g
    assert len(agent._graphs) == 2 and all(len(r) == 2 and all(g["graph"] is not None for g in r)
                                           for r in agent._graphs.values())
    assert logs_e == logs_g
    for k in eager:
        assert torch.equal(eager[k], graph[k]), k
    assert float(eager["critic_steps"][0]) == 14 and float(eager["actor_steps"][0]) == 7
    B, oframe = rb.batch_size, 9 * 34 * 37
    assert len(rb._graph_blocks) == 4
    for g in rb._graph_blocks.values():  # the slots' scratch is sized for CROPPED frames and sits between intact guards
        assert len(g["guards"]) == (4 if dedup else 2)
        assert all(guard.numel() >= rb.GUARD and bool((guard == rb.GUARD_BYTE).all()) for guard in g["guards"])
        assert g["shift_u8"].numel() == 3 * B * oframe + 32
        assert bool(g["shift_u8"][:3 * B * oframe].any()) and not bool(g["shift_u8"][-32:].any())


# ------------------------------------------------------------------------------------------------ 5. batched acting
@pytest.mark.parametrize("name", ["random_crop+cutout_color", "translate+cutout_color"])
def test_batched_acting_on_frames_of_the_input_size(name):
    """select_actions / sample_actions on N = 3 frames of ``input_shape`` equal the calls on their
    ``evaluation_augmentation`` (the move's: centre window under a crop, centred canvas under a translate), bit for bit."""
    in_hw = (40, 44)
    out_hw = (33, 36) if name.startswith("random_crop") else (47, 52)  # (odd margins: the centring floors)
    agent = _agent(3, name, in_hw, out_hw)
    frames = np.random.RandomState(8).randint(0, 256, (3, C9) + in_hw, dtype=np.uint8)
    evald = np.ascontiguousarray(np.stack([agent.augmentor.evaluation_augmentation(f) for f in frames]))
    assert evald.shape == (3, C9) + out_hw
    want = agent.select_actions(evald)
    assert want.shape == (3, 2) and np.isfinite(want).all()
    for route in (lambda x: x, list, lambda x: torch.from_numpy(x).cuda(), lambda x: x.astype(np.float32)):
        assert np.array_equal(agent.select_actions(route(frames)), agent.select_actions(route(evald)))
    assert np.array_equal(agent.select_actions(frames), want)
    noise = torch.randn(3, 2, generator=torch.Generator().manual_seed(2))
    assert np.array_equal(agent.sample_actions(frames, noise=noise), agent.sample_actions(evald, noise=noise))
    singles = []
    for obs in (frames[0], evald[0]):  # sample_action goes through evaluation_augmentation; the same seeded noise
        torch.manual_seed(4)
        torch.cuda.manual_seed_all(4)
        singles.append(agent.sample_action(obs))
    assert np.array_equal(*singles)
    with pytest.raises(ValueError):
        agent.select_actions(np.zeros((3, C9, 42, 44), np.uint8))
    assert not np.array_equal(want, agent.select_actions(np.ascontiguousarray(evald[:, :, ::-1])))  # (pixels matter)
