"""``Compose(move, paint)`` (a crop, shift or translate with a cutout painted over its output) without a GPU: the
constructor's validation, ``make_augmentor``'s six ``'<move>+<paint>'`` names, the order of the NumPy draws, the host
restatement against a per-pixel loop, evaluation, the replay buffer's draws, the block layout for six index words (and
that of every other augmentor, unchanged), scratch sizes, where the one fused launch sits in the launch schedule of the
four routes (trace hook: nothing is computed), the agent's batched acting arguments and the C ABI's declaration."""
import os
import re

import numpy as np
import pytest
import torch

import curla_amd
from curla_amd import _lib, ops
from curla_amd.utils import ReplayBuffer
from tests.test_host_logic import HP

C, HW, B, CAP = 9, (34, 40), 8, 32
CROP, CANVAS = (28, 34), (42, 48)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [m + "+" + p for m in ("random_crop", "random_shift", "translate") for p in ("cutout", "cutout_color")]
MOVES = {"random_crop": (curla_amd.RandomCrop, CROP, ops.MOVE_CROP), "random_shift": (curla_amd.RandomShift, None, ops.MOVE_SHIFT),
         "translate": (curla_amd.RandomTranslate, CANVAS, ops.MOVE_TRANSLATE)}


def _make(name, **kw):
    """(max_cut 20: the default 30 is taller than the cropped frame)"""
    return curla_amd.make_augmentor(name, HW, MOVES[name.split("+")[0]][1], **{"max_cut": 20, **kw})


def _out_hw(name):
    return MOVES[name.split("+")[0]][1] or HW


def _same_stream(a, b):
    return np.array_equal(a[1], b[1]) and a[2] == b[2]


def compose_loop(imgs, move, a, b, y0, x0, bh, bw, rgb, out_hw, pad=0):
    """The issue's formula, pixel by pixel: mid = move(in), then the box in output coordinates.  (B, C, H, W) in."""
    n, c, h, w = imgs.shape
    out = np.empty((n, c) + tuple(out_hw), dtype=imgs.dtype)
    for s in range(n):
        for ch in range(c):
            for y in range(out_hw[0]):
                for x in range(out_hw[1]):
                    if move == "random_crop":
                        v = imgs[s, ch, y + a[s], x + b[s]]
                    elif move == "random_shift":
                        v = imgs[s, ch, min(max(y + a[s] - pad, 0), h - 1), min(max(x + b[s] - pad, 0), w - 1)]
                    else:
                        inside = 0 <= y - a[s] < h and 0 <= x - b[s] < w
                        v = imgs[s, ch, y - a[s], x - b[s]] if inside else 0
                    if y0[s] <= y < y0[s] + bh[s] and x0[s] <= x < x0[s] + bw[s]:
                        v = 0 if rgb is None else rgb[s][ch % 3]
                    out[s, ch, y, x] = v
    return out


# ------------------------------------------------------------------------------------------------ augmentor API
def test_constructor_validation():
    crop, shift, tr = curla_amd.RandomCrop(HW, CROP), curla_amd.RandomShift(HW, 3), curla_amd.RandomTranslate(HW, CANVAS)
    for move in (crop, shift, tr):
        paint = curla_amd.RandomCutout(move.output_shape, 4, 9, color=True)
        aug = curla_amd.Compose(move, paint)
        assert aug.move is move and aug.paint is paint
        assert aug.input_shape == tuple(move.input_shape) == HW and aug.output_shape == tuple(move.output_shape)
        assert aug.sample_kind == "scratch" and aug.index_rows == 6
        with pytest.raises(ValueError):  # the other order
            curla_amd.Compose(paint, move)
    cut = curla_amd.RandomCutout(HW)
    for bad_move in (curla_amd.IdentityAugmentation(HW), curla_amd.ColorJiggle(HW), curla_amd.RandomConv(HW), cut, None,
                     curla_amd.Compose(shift, cut)):
        with pytest.raises(ValueError):
            curla_amd.Compose(bad_move, cut)
    for bad_paint in (curla_amd.IdentityAugmentation(HW), shift, curla_amd.NoisyCover(HW), None, "cutout"):
        with pytest.raises(ValueError):
            curla_amd.Compose(shift, bad_paint)
    # a paint built for the stored size cannot follow a move that changes it, and the other way round
    for move in (crop, tr):
        with pytest.raises(ValueError):
            curla_amd.Compose(move, cut)
    with pytest.raises(ValueError):
        curla_amd.Compose(shift, curla_amd.RandomCutout(CROP))
    from curla_amd.augmentations import Compose
    assert Compose is curla_amd.Compose and "Compose" in curla_amd.__all__


def test_make_augmentor_builds_the_six_names_and_rejects_the_rest():
    for name in NAMES:
        move, paint = name.split("+")
        cls, out, _ = MOVES[move]
        aug = _make(name, pad=3, min_cut=5, max_cut=7)
        assert type(aug) is curla_amd.Compose and type(aug.move) is cls and type(aug.paint) is curla_amd.RandomCutout
        assert aug.output_shape == (out or HW) == tuple(aug.paint.input_shape) and aug.input_shape == HW
        assert (aug.paint.min_cut, aug.paint.max_cut, aug.paint.color) == (5, 7, paint == "cutout_color")
        if move == "random_shift":
            assert aug.move.pad == 3
    assert curla_amd.make_augmentor("random_crop+cutout", HW, max_cut=20).output_shape == (29, 34)  # the crop's default
    with pytest.raises(ValueError):  # the paint is built for the cropped frame: the default max_cut of 30 does not fit 29
        curla_amd.make_augmentor("random_crop+cutout", HW)
    assert curla_amd.make_augmentor("translate+cutout", HW).output_shape == (42, 48)         # the translate's default
    for other in ("cutout+random_crop", "random_crop+random_shift", "random_crop+color_jiggle", "identity+cutout",
                  "random_crop+cutout+cutout", "random_crop+", "+cutout", "+", "random_conv+cutout", "cutout+cutout"):
        with pytest.raises(ValueError, match="augmentation is not supported"):
            curla_amd.make_augmentor(other, HW)
    for name, cls, out in (("identity", curla_amd.IdentityAugmentation, HW), ("random_crop", curla_amd.RandomCrop, (29, 34)),
                           ("random_shift", curla_amd.RandomShift, HW), ("cutout", curla_amd.RandomCutout, HW),
                           ("cutout_color", curla_amd.RandomCutout, HW), ("color_jiggle", curla_amd.ColorJiggle, HW),
                           ("noisy_cover", curla_amd.NoisyCover, HW), ("random_conv", curla_amd.RandomConv, HW),
                           ("translate", curla_amd.RandomTranslate, (42, 48))):
        aug = curla_amd.make_augmentor(name, HW)
        assert type(aug) is cls and tuple(aug.output_shape) == out


# ------------------------------------------------------------------------------------------------ draws
def _bare_draws(name, n, pad=4, min_cut=10, max_cut=20):
    """The expected ``randint`` calls of one tensor, in order: the mover's two, then RandomCutout.draw_boxes'."""
    move, paint = name.split("+")
    oh, ow = _out_hw(name)
    if move == "random_crop":
        a, b = np.random.randint(0, HW[0] - oh, n), np.random.randint(0, HW[1] - ow, n)
    elif move == "random_shift":
        a, b = np.random.randint(0, 2 * pad + 1, n), np.random.randint(0, 2 * pad + 1, n)
    else:
        a, b = np.random.randint(0, oh - HW[0] + 1, n), np.random.randint(0, ow - HW[1] + 1, n)
    bh = np.random.randint(min_cut, max_cut + 1, n)
    bw = np.random.randint(min_cut, max_cut + 1, n)
    y0 = np.random.randint(0, oh - bh + 1)
    x0 = np.random.randint(0, ow - bw + 1)
    rgb = np.random.randint(0, 256, (n, 3)) if paint == "cutout_color" else None
    return a, b, y0, x0, bh, bw, rgb


def _words(d):
    a, b, y0, x0, bh, bw, rgb = d
    return [a, b, y0, x0, bh | (bw << 16), np.zeros_like(a) if rgb is None else rgb[:, 0] | (rgb[:, 1] << 8) | (rgb[:, 2] << 16)]


@pytest.mark.parametrize("name", NAMES)
def test_draw_index_words_are_the_movers_two_calls_then_the_boxes(name):
    aug, n = _make(name), 500
    np.random.seed(17)
    got = aug.draw_index_words(n)
    after = np.random.get_state()
    np.random.seed(17)
    want = _words(_bare_draws(name, n))
    assert _same_stream(after, np.random.get_state())  # nothing else was drawn
    assert len(got) == 6
    for g, w in zip(got, want):
        assert np.array_equal(np.broadcast_to(g, (n,)), w)
    oh, ow = aug.output_shape  # the box lies inside the OUTPUT frame
    bh, bw = want[4] & 0xffff, want[4] >> 16
    assert (want[2] + bh).max() <= oh and (want[3] + bw).max() <= ow and want[2].min() >= 0 and want[3].min() >= 0


# ------------------------------------------------------------------------------------------------ host restatement
@pytest.mark.parametrize("name", NAMES)
def test_training_augmentation_is_the_per_pixel_formula(name):
    move = name.split("+")[0]
    hw, out = (9, 11), {"random_crop": (6, 7), "random_shift": None, "translate": (12, 13)}[move]
    aug = curla_amd.make_augmentor(name, hw, out, pad=2, min_cut=2, max_cut=5)
    imgs = np.random.RandomState(2).randint(1, 256, (5, 6) + hw, dtype=np.uint8)
    keep = imgs.copy()
    np.random.seed(23)
    got = aug.training_augmentation(imgs)
    after = np.random.get_state()
    np.random.seed(23)
    a, b = aug.move.draw_index_words(5)
    y0, x0, bh, bw, rgb = aug.paint.draw_boxes(5)
    assert _same_stream(after, np.random.get_state())
    want = compose_loop(imgs, move, a, b, y0, x0, bh, bw, rgb, aug.output_shape, pad=2)
    assert got.dtype == np.uint8 and got.shape == (5, 6) + aug.output_shape and np.array_equal(got, want)
    assert np.array_equal(imgs, keep)
    plain = compose_loop(imgs, move, a, b, y0, x0, 0 * bh, bw, rgb, aug.output_shape, pad=2)
    assert not np.array_equal(want, plain)  # the boxes did paint


def test_evaluation_augmentation_is_the_movers():
    img = np.random.RandomState(3).randint(1, 256, (6,) + HW, dtype=np.uint8)
    for name in NAMES:
        aug = _make(name)
        got = aug.evaluation_augmentation(img)
        assert np.array_equal(got, aug.move.evaluation_augmentation(img)) and got.shape == (6,) + aug.output_shape
    assert np.array_equal(_make("random_crop+cutout").evaluation_augmentation(img), img[:, 3:31, 3:37])
    assert _make("random_shift+cutout").evaluation_augmentation(img) is img
    centred = _make("translate+cutout").evaluation_augmentation(img)
    assert np.array_equal(centred[:, 4:38, 4:44], img) and int((centred != 0).sum()) == img.size


# ------------------------------------------------------------------------------------------------ ReplayBuffer, host side
@pytest.mark.parametrize("name", ["random_crop+cutout_color", "random_shift+cutout", "translate+cutout_color"])
def test_draw_indices_is_one_index_draw_then_three_times_six_words(name):
    rb = ReplayBuffer((C,) + HW, (2,), 64, B, "cpu", _make(name))
    rb.idx = 40
    np.random.seed(5)
    idxs, offs = rb.draw_indices()
    after = np.random.get_state()
    np.random.seed(5)
    want_idx = np.random.randint(0, 40, size=B)
    per_tensor = [_words(_bare_draws(name, B)) for _ in range(3)]
    assert _same_stream(after, np.random.get_state())
    assert np.array_equal(idxs, want_idx) and offs.shape == (18, B) and offs.dtype == np.int32
    for j in range(3):
        for r in range(6):
            assert np.array_equal(offs[6 * (r // 2) + 2 * j + r % 2], per_tensor[j][r]), (j, r)


def _literal_layout(b, n_step, cut_runs=0):
    n = 2 * b * 8 + 6 * b * 4
    lay = dict(idx=0, offs=2 * b * 8, offs_end=n, aug=None, aug_stride=0, aug_order=None, aug_rng=None)
    if cut_runs:
        lay["cut"] = n
        n += cut_runs * 3 * b * 4
    if n_step > 1:
        lay["next_row"] = n
        n += 8 * b
    lay.update(nbytes=n, tail=n, graph_nbytes=n + 80)
    return lay


@pytest.mark.parametrize("n_step", [1, 3])
def test_block_layout_for_six_words_and_unchanged_for_the_others(n_step):
    kw = dict(n_step=n_step, discount=0.99) if n_step > 1 else {}
    for name in NAMES:
        rb = ReplayBuffer((C,) + HW, (2,), CAP, B, "cpu", _make(name), **kw)
        assert rb.block_layout() == _literal_layout(B, n_step, 4), name
    for name, runs in (("identity", 0), ("random_crop", 0), ("random_shift", 0), ("translate", 0), ("cutout", 2),
                       ("cutout_color", 2), ("color_jiggle", 0), ("noisy_cover", 0), ("random_conv", 0)):
        rb = ReplayBuffer((C,) + HW, (2,), CAP, B, "cpu", curla_amd.make_augmentor(name, HW), **kw)
        assert rb.block_layout() == _literal_layout(B, n_step, runs), name
        assert rb.draw_indices.__func__ is ReplayBuffer.draw_indices
    # the block as the kernel reads it: the move's offsets where crop offsets sit, then y0 | x0 | size | rgb runs of 3B
    rb = ReplayBuffer((C,) + HW, (2,), CAP, B, "cpu", _make(NAMES[1]), **kw)
    lay = rb.block_layout()
    idxs = np.arange(B)[::-1].copy()
    offs = np.arange(18 * B, dtype=np.int32).reshape(18, B)
    host = torch.zeros(lay["nbytes"], dtype=torch.uint8)
    rb._fill_index_block(host, idxs, offs)
    raw = host.numpy()
    assert raw[:16 * B].view(np.int64).tolist() == idxs.tolist() + (idxs + CAP).tolist()
    o32 = raw[16 * B:40 * B].view(np.int32)
    assert o32[:3 * B].tolist() == np.concatenate([offs[0], offs[2], offs[4]]).tolist()
    assert o32[3 * B:].tolist() == np.concatenate([offs[1], offs[3], offs[5]]).tolist()
    c32 = raw[lay["cut"]:lay["cut"] + 48 * B].view(np.int32).reshape(4, 3 * B)
    for k, rows in enumerate(([6, 8, 10], [7, 9, 11], [12, 14, 16], [13, 15, 17])):
        assert c32[k].tolist() == np.concatenate([offs[r] for r in rows]).tolist(), k
    for wrong in (6, 12):
        with pytest.raises(ValueError):
            rb._fill_index_block(host, idxs, offs[:wrong])


@pytest.mark.parametrize("kw", [{}, dict(dedup_frames=True)], ids=["plain", "dedup"])
def test_scratch_holds_frames_of_the_output_size(kw):
    for name in ("random_crop+cutout", "random_shift+cutout", "translate+cutout"):
        rb = ReplayBuffer((C,) + HW, (2,), 64, B, "cpu", _make(name), **kw)
        oh, ow = _out_hw(name)
        frame, oframe = C * HW[0] * HW[1], C * oh * ow
        assert rb._frame == frame and rb._scratch_frame() == oframe and rb.obs_shape == (C,) + HW
        need = 3 * B * oframe + 32
        assert rb._shift_store.shape == (rb.N_SAMPLE_SLOTS, (need + 255) // 256 * 256)
        _lib.set_trace_hook(lambda name, args: None)
        try:
            g = rb.graph_block(0)
        finally:
            _lib.set_trace_hook(None)
        assert g["shift_u8"].numel() == need and len(g["guards"]) == (4 if kw else 2)
        assert all(bool((x == rb.GUARD_BYTE).all()) and x.numel() >= rb.GUARD for x in g["guards"])
        if kw:  # the gathered stacks stay stored-frame sized
            assert g["mb_u8"].numel() == 2 * B * frame + 32 and rb._mb_store.shape[1] == 2 * B * frame + 32
        else:
            assert tuple(rb.obses.shape) == (64,) + HW + (C,)


# ------------------------------------------------------------------------------------------------ launch schedule
def _rb(aug, obs_shape=(C,) + HW, cap=CAP, batch=B, n_add=12, **kw):
    rb = ReplayBuffer(obs_shape, (2,), cap, batch, "cpu", aug, **kw)
    rs = np.random.RandomState(3)
    for _ in range(n_add):
        f = rs.randint(0, 256, obs_shape, dtype=np.uint8)
        rb.add(f, [0.1, -0.2], 0.5, f, False)
    # a CPU buffer has no pinned index slots; stand in for their device addresses so that sampling takes the route
    # of a device buffer (staging kernel) under the trace hook, which computes nothing
    rb._h_index_dev = [4096 * (k + 1) for k in range(rb._n_slots)]
    return rb


def _traced(fn):
    calls = []
    _lib.set_trace_hook(lambda name, args: calls.append((name, args)))
    try:
        out = fn()
    finally:
        _lib.set_trace_hook(None)
    return calls, out


OTHER_SCRATCH = ("curla_random_shift_u8", "curla_cutout_u8", "curla_translate_u8")
FUSED = "curla_move_cutout_u8"


@pytest.mark.parametrize("name", ["random_crop+cutout_color", "random_shift+cutout", "translate+cutout_color"])
def test_one_fused_launch_behind_the_staging_on_plain_storage(name):
    rb = _rb(_make(name, pad=3))
    out_hw, code = _out_hw(name), MOVES[name.split("+")[0]][2]
    calls, sample = _traced(rb.sample_cpc_refs)
    assert [n for n, _ in calls] == ["curla_sample_stage", FUSED]
    (frames, idx, period, move, a, b, pad, y0, x0, size, rgb, n, c, h, w, ho, wo, out, _) = calls[1][1]
    blk, lay = rb._d_index[rb._sample_slot].data_ptr(), rb.block_layout()
    assert frames == rb._both.data_ptr() and idx == blk and period == 2 * B and n == 3 * B and move == code
    assert pad == (3 if code == ops.MOVE_SHIFT else 0)
    assert a == blk + lay["offs"] and b == a + 12 * B
    assert [y0, x0, size, rgb] == [blk + lay["cut"] + 12 * B * k for k in range(4)]
    assert (c, h, w, ho, wo) == (C,) + HW + out_hw
    assert out == rb._shift_store[rb._sample_slot].data_ptr()
    obs, _, _, nxt, _, kw = sample
    for ref, row0 in ((obs, 0), (nxt, B), (kw["obs_pos"], 2 * B)):
        assert ref.src.data_ptr() == out and tuple(ref.src.shape) == (3 * B,) + out_hw + (C,)
        assert ref.is_u8 == 1 and ref.B == B and (ref.Hc, ref.Wc) == (ref.Hs, ref.Ws) == out_hw
        assert ref.idx.tolist() == list(range(row0, row0 + B)) and not ref.h1.any() and not ref.w1.any()
    assert obs.pair[0].B == 2 * B and obs.pair[0].idx.tolist() == list(range(2 * B)) and obs.pair[1] is nxt
    calls, _ = _traced(rb.sample_cpc_refs)  # the next sample goes to the other slot's scratch
    assert calls[1][1][17] == rb._shift_store[rb._sample_slot].data_ptr() != out
    calls, tensors = _traced(rb.sample_cpc)
    assert [n for n, _ in calls] == ["curla_sample_stage", FUSED] + ["curla_crop_nchw"] * 3
    scratch = rb._shift_store[rb._sample_slot].data_ptr()
    assert all(a[0] == scratch and a[2] == rb._shift_zero.data_ptr() == a[3] for nm, a in calls if nm == "curla_crop_nchw")
    assert tuple(tensors[0].shape) == (B, C) + out_hw == tuple(tensors[3].shape) == tuple(tensors[5]["obs_pos"].shape)


def test_on_the_frame_store_the_fused_launch_comes_behind_the_two_gathers():
    rb = _rb(_make("random_crop+cutout_color"), dedup_frames=True)
    calls, _ = _traced(rb.sample_cpc_refs)
    assert [n for n, _ in calls] == ["curla_sample_stage", "curla_gather_stacks", "curla_gather_stacks", FUSED]
    a = calls[-1][1]
    assert a[0] == rb._mb_store[rb._sample_slot].data_ptr() and a[1] is None and a[2] == 2 * B and a[11] == 3 * B
    assert tuple(a[12:17]) == (C,) + HW + CROP and a[3] == ops.MOVE_CROP


def test_rings_in_two_allocations_take_one_fused_launch_per_tensor():
    hw, out_hw = (11, 13), (9, 10)
    aug = curla_amd.make_augmentor("random_crop+cutout", hw, out_hw, min_cut=2, max_cut=4)
    rb = _rb(aug, obs_shape=(3,) + hw, cap=7, batch=4, n_add=5)
    assert (7 * 429) % 4 != 0 and rb._both is None
    calls, _ = _traced(rb.sample_cpc_refs)
    names = [n for n, _ in calls]
    assert names == ["curla_sample_stage"] + [FUSED] * 3 and not set(names) & set(OTHER_SCRATCH)
    moves = [a for n, a in calls if n == FUSED]
    out0 = rb._shift_store[rb._sample_slot].data_ptr()
    blk, lay = rb._d_index[rb._sample_slot].data_ptr(), rb.block_layout()
    assert [a[0] for a in moves] == [rb.obses.data_ptr(), rb.next_obses.data_ptr(), rb.obses.data_ptr()]
    assert [a[1] for a in moves] == [blk] * 3 and all(a[2] == 4 and a[11] == 4 for a in moves)
    assert [a[17] for a in moves] == [out0 + j * 4 * 3 * 9 * 10 for j in range(3)]  # strides of OUTPUT frames
    for j, a in enumerate(moves):
        assert [a[4], a[5]] == [blk + 64 + 16 * (3 * k + j) for k in range(2)]
        assert list(a[7:11]) == [blk + lay["cut"] + 16 * (3 * k + j) for k in range(4)]
    assert not rb.graph_supported()


def test_n_step_composes_inside_the_staging_launch_in_front_of_the_fused_launch():
    rb = _rb(_make("translate+cutout"), n_step=3, discount=0.99)
    calls, _ = _traced(rb.sample_cpc_refs)
    assert [n for n, _ in calls] == ["curla_sample_stage_nstep", FUSED]
    a = calls[1][1]
    assert a[1] == rb._d_index[rb._sample_slot].data_ptr() and a[2] == 2 * B and a[11] == 3 * B


@pytest.mark.parametrize("name", ["identity", "random_crop", "random_shift", "cutout_color", "translate", "color_jiggle"])
def test_the_other_buffers_never_make_the_fused_launch(name):
    rb = _rb(curla_amd.make_augmentor(name, HW))
    calls, _ = _traced(lambda: (rb.sample_cpc_refs(), rb.sample_cpc()))
    names = [n for n, _ in calls]
    assert "curla_sample_stage" in names and FUSED not in names


def test_graph_slot_records_the_fused_launch_behind_staging_and_gathers():
    for dedup in (False, True):
        rb = _rb(_make("random_crop+cutout_color"), dedup_frames=dedup)
        assert rb.graph_supported() is False  # (a CPU buffer; on the device: tests/test_gpu_compose.py)
        _, g = _traced(lambda: rb.graph_block(0))
        before = np.random.get_state()
        calls, (obs, _, _, nxt, _, kw) = _traced(lambda: rb.graph_refs(0))
        assert _same_stream(before, np.random.get_state())
        assert [n for n, _ in calls] == ["curla_sample_stage"] + ["curla_gather_stacks"] * (2 if dedup else 0) + [FUSED]
        a, dev, lay = calls[-1][1], g["dev"].data_ptr(), rb.block_layout()
        assert (a[4], a[5]) == (dev + 16 * B, dev + 28 * B) and (a[2], a[11]) == (2 * B, 3 * B)
        assert list(a[7:11]) == [dev + lay["cut"] + 12 * B * k for k in range(4)]
        assert a[17] == g["shift_u8"].data_ptr() and tuple(a[12:17]) == (C,) + HW + CROP
        assert (a[0], a[1]) == ((g["mb_u8"].data_ptr(), None) if dedup else (rb._both.data_ptr(), dev))
        for ref, row0 in ((obs, 0), (nxt, B), (kw["obs_pos"], 2 * B)):
            assert ref.src.data_ptr() == g["shift_u8"].data_ptr() and ref.is_u8 == 1 and ref.guard is None
            assert (ref.Hc, ref.Wc) == CROP and ref.idx.tolist() == list(range(row0, row0 + B))


def test_ops_move_cutout_checks_shapes_before_any_launch():
    ring = torch.zeros((4, 5, 7, 3), dtype=torch.uint8)
    w = torch.zeros(4, dtype=torch.int32)
    outs = {ops.MOVE_CROP: (4, 4, 6, 3), ops.MOVE_SHIFT: (4, 5, 7, 3), ops.MOVE_TRANSLATE: (4, 8, 9, 3)}
    calls = []
    _lib.set_trace_hook(lambda name, args: calls.append((name, args)))
    try:
        for move, shape in outs.items():
            out = torch.zeros(shape, dtype=torch.uint8)
            ops.move_cutout_u8(ring, None, 4, move, w, w, 2, (w, w, w, w), 4, out)
            assert calls[-1][0] == FUSED and tuple(calls[-1][1][11:17]) == (4, 3, 5, 7) + shape[1:3]
            ops.move_cutout_u8(ring, None, 4, move, w, w, 2, None, 4, out)  # no box: four NULL pointers
            assert calls[-1][1][7:11] == (None,) * 4
        del calls[:]
        ok = torch.zeros(outs[ops.MOVE_SHIFT], dtype=torch.uint8)
        for kw in (dict(move=ops.MOVE_CROP, out=torch.zeros((4, 6, 7, 3), dtype=torch.uint8)),       # taller than the frame
                   dict(move=ops.MOVE_SHIFT, out=torch.zeros((4, 5, 6, 3), dtype=torch.uint8)),      # not the frame's size
                   dict(move=ops.MOVE_TRANSLATE, out=torch.zeros((4, 5, 6, 3), dtype=torch.uint8)),  # narrower canvas
                   dict(move=3), dict(move=-1),                                                      # unknown move
                   dict(out=torch.zeros((4, 5, 7, 4), dtype=torch.uint8)),                           # channel count
                   dict(out=torch.zeros((3, 5, 7, 3), dtype=torch.uint8)),                           # fewer samples than n
                   dict(out=torch.zeros((4, 5, 7, 3), dtype=torch.float32)),                         # dtype
                   dict(a=torch.zeros(3, dtype=torch.int32)), dict(b=torch.zeros(4, dtype=torch.int64)),
                   dict(box=(w, w, w)), dict(box=(w, w, w, torch.zeros(3, dtype=torch.int32))),
                   dict(idx=torch.zeros(3, dtype=torch.int64))):
            args = dict(idx=None, move=ops.MOVE_SHIFT, a=w, b=w, box=(w, w, w, w), out=ok)
            args.update(kw)
            with pytest.raises(_lib.CurlaHipError):
                ops.move_cutout_u8(ring, args["idx"], 4, args["move"], args["a"], args["b"], 2, args["box"], 4, args["out"])
        assert calls == []
    finally:
        _lib.set_trace_hook(None)
    with pytest.raises(_lib.CurlaHipError):  # without the hook a CPU tensor is refused
        ops.move_cutout_u8(ring, None, 4, ops.MOVE_SHIFT, w, w, 2, None, 4, ok)


# ------------------------------------------------------------------------------------------------ agent
def test_batched_acting_accepts_both_frame_sizes():
    frames = np.random.RandomState(4).randint(1, 256, (3, C) + HW, dtype=np.uint8)
    for name, windows in (("random_crop+cutout_color", {CROP: (0, 0), HW: (3, 3)}),
                          ("translate+cutout", {CANVAS: (0, 0), HW: None}), ("random_shift+cutout", {HW: (0, 0)})):
        aug = _make(name)
        curla_amd.set_seed_everywhere(1)
        agent = curla_amd.CurlSacAgent((C,) + aug.output_shape, (2,), "cpu", aug, hidden_dim=64, **HP)
        assert agent._act_windows() == windows
        want = np.stack([aug.evaluation_augmentation(f) for f in frames])
        _lib.set_trace_hook(lambda name, args: None)
        try:
            for x in (frames, list(frames), torch.from_numpy(frames)):
                got, shape, window = agent._act_batch_args(x, None)
                if name.startswith("random_crop"):  # the centre window is cut inside the staging launch
                    assert shape == (3, C) + HW and window == (3, 3)
                else:
                    assert shape == (3, C) + aug.output_shape and window == (0, 0)
                    assert np.array_equal(np.asarray(got if not isinstance(got, list) else np.stack(got)), want)
            same, shape, window = agent._act_batch_args(want, None)
            assert same is want and shape == want.shape and window == (0, 0)
            with pytest.raises(ValueError):
                agent._act_batch_args(np.zeros((3, C, 36, 41), np.uint8), None)
        finally:
            _lib.set_trace_hook(None)


# ------------------------------------------------------------------------------------------------ ABI
def test_header_declares_the_entry_point_and_the_abi_number_stays():
    with open(os.path.join(ROOT, "include", "curla_hip.h")) as f:
        header = f.read()
    m = re.search(r"\bint\s+curla_move_cutout_u8\s*\(([^)]*)\)\s*;", header)
    assert m, "include/curla_hip.h does not declare curla_move_cutout_u8"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == len(_lib.SIGNATURES["curla_move_cutout_u8"]) == 19
    want = ("frames", "idx", "period", "move", "a", "b", "pad", "y0", "x0", "size", "rgb", "n", "C", "H", "W", "Ho", "Wo",
            "out", "stream")
    assert tuple(p.split()[-1].lstrip("*") for p in params) == want
    for p, t in zip(params, _lib.SIGNATURES["curla_move_cutout_u8"]):
        assert ("*" in p) == (t is _lib.vp), p
        if t is not _lib.vp:
            assert p.startswith("int ") and t is _lib.c_int
    assert re.search(r"#define\s+CURLA_ABI_VERSION\s+8\b", header) and _lib.ABI_VERSION == 8
