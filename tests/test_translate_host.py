"""``RandomTranslate`` (RAD's translate: the frame at a random position on a larger black canvas) without a GPU: the
augmentor's API and validation, the order of its NumPy draws, the host restatement against a per-pixel loop, the centred
evaluation form, the replay buffer's draws, unchanged block layout and scratch sizes (the first scratch whose frames are
larger than the stored ones), where the translate launch sits in the launch schedule (trace hook: nothing is computed),
the agent's batched acting arguments and the C ABI's declaration."""
import os
import re

import numpy as np
import pytest
import torch

import curla_amd
from curla_amd import _lib
from curla_amd.utils import ReplayBuffer
from tests.test_host_logic import HP

C, HW, OUT, B, CAP = 9, (34, 40), (42, 48), 8, 32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def translate_loop(imgs, ty, tx, out_hw):
    """The formula of the class docstring, pixel by pixel: (B, C, H, W) -> (B, C, Ho, Wo)."""
    n, c, h, w = imgs.shape
    out = np.empty((n, c) + tuple(out_hw), dtype=imgs.dtype)
    for b in range(n):
        for ch in range(c):
            for y in range(out_hw[0]):
                for x in range(out_hw[1]):
                    inside = 0 <= y - ty[b] < h and 0 <= x - tx[b] < w
                    out[b, ch, y, x] = imgs[b, ch, y - ty[b], x - tx[b]] if inside else 0
    return out


# ------------------------------------------------------------------------------------------------ augmentor API
def test_constructor_validation_and_default_output_shape():
    aug = curla_amd.RandomTranslate(HW)
    assert aug.input_shape == HW and aug.output_shape == (HW[0] + 8, HW[1] + 8)
    assert isinstance(aug, curla_amd.IdentityAugmentation)
    assert not isinstance(aug, (curla_amd.RandomCrop, curla_amd.RandomShift, curla_amd.RandomCutout))
    assert curla_amd.RandomTranslate(HW, OUT).output_shape == OUT
    assert curla_amd.RandomTranslate(list(HW), [np.int64(34), 41]).output_shape == (34, 41)  # no margin in y is allowed
    assert curla_amd.RandomTranslate(HW, HW).output_shape == HW
    for bad_in in ((34,), (3, 34, 40), (34.0, 40), (True, 40), ("34", 40)):
        with pytest.raises(ValueError):
            curla_amd.RandomTranslate(bad_in)
    for bad_out in ((42,), (9, 42, 48), (42.0, 48), (42, True), (42, "48"), (33, 48), (42, 39), (33, 39)):
        with pytest.raises(ValueError):
            curla_amd.RandomTranslate(HW, bad_out)
    from curla_amd.augmentations import RandomTranslate
    assert RandomTranslate is curla_amd.RandomTranslate and "RandomTranslate" in curla_amd.__all__


def test_make_augmentor_builds_it_and_the_other_names_build_what_they_built():
    a = curla_amd.make_augmentor("translate", HW)
    b = curla_amd.make_augmentor("translate", HW, OUT)
    assert type(a) is curla_amd.RandomTranslate and a.output_shape == (42, 48)
    assert type(b) is curla_amd.RandomTranslate and b.output_shape == OUT
    with pytest.raises(ValueError):
        curla_amd.make_augmentor("translate", HW, (30, 48))
    for name, cls, out in (("identity", curla_amd.IdentityAugmentation, HW), ("random_crop", curla_amd.RandomCrop, (29, 34)),
                           ("random_shift", curla_amd.RandomShift, HW), ("cutout", curla_amd.RandomCutout, HW),
                           ("cutout_color", curla_amd.RandomCutout, HW), ("color_jiggle", curla_amd.ColorJiggle, HW),
                           ("noisy_cover", curla_amd.NoisyCover, HW), ("random_conv", curla_amd.RandomConv, HW)):
        aug = curla_amd.make_augmentor(name, HW)
        assert type(aug) is cls and tuple(aug.output_shape) == out
    assert tuple(curla_amd.make_augmentor("random_crop", HW, (28, 30)).output_shape) == (28, 30)
    for unknown in ("translat", "random_translate", "Translate"):
        with pytest.raises(ValueError):
            curla_amd.make_augmentor(unknown, HW)


# ------------------------------------------------------------------------------------------------ draws
def test_draw_offsets_are_two_randint_calls_in_order_and_cover_the_range():
    aug = curla_amd.RandomTranslate(HW, (37, 49))
    n = 4000
    np.random.seed(17)
    ty, tx = aug.draw_offsets(n)
    after = np.random.get_state()
    np.random.seed(17)
    want_ty = np.random.randint(0, 37 - 34 + 1, n)
    want_tx = np.random.randint(0, 49 - 40 + 1, n)
    assert np.array_equal(ty, want_ty) and np.array_equal(tx, want_tx)
    now = np.random.get_state()
    assert np.array_equal(after[1], now[1]) and after[2] == now[2]  # nothing else was drawn
    assert sorted(set(ty.tolist())) == list(range(4)) and sorted(set(tx.tolist())) == list(range(10))
    # no margin in y (Ho == H): only zeros are drawn for it, by the same two calls
    flat = curla_amd.RandomTranslate(HW, (34, 49))
    np.random.seed(17)
    ty, tx = flat.draw_offsets(n)
    after = np.random.get_state()
    np.random.seed(17)
    assert ty.shape == (n,) and not ty.any() and not np.random.randint(0, 1, n).any()
    assert np.array_equal(tx, np.random.randint(0, 10, n))
    now = np.random.get_state()
    assert np.array_equal(after[1], now[1]) and after[2] == now[2]


# ------------------------------------------------------------------------------------------------ host restatement
def test_translate_matches_the_per_pixel_formula():
    n, c, h, w = 2, 6, 5, 7
    out_hw = (8, 9)
    aug = curla_amd.RandomTranslate((h, w), out_hw)
    imgs = np.random.RandomState(1).randint(1, 256, (n, c, h, w), dtype=np.uint8)
    untouched = imgs.copy()
    for ty, tx in (((0, 3), (0, 2)), ((3, 0), (2, 0)), ((0, 3), (2, 0)), ((1, 2), (1, 1))):  # both ends of both ranges
        got = aug.translate(imgs, np.array(ty), np.array(tx))
        assert got.dtype == imgs.dtype and got.shape == (n, c) + out_hw
        assert np.array_equal(got, translate_loop(imgs, ty, tx, out_hw))
        for b in range(n):  # every source pixel is kept, nothing else is set
            assert np.array_equal(got[b, :, ty[b]:ty[b] + h, tx[b]:tx[b] + w], imgs[b])
            assert int((got[b] != 0).sum()) == imgs[b].size
    assert np.array_equal(imgs, untouched)


def test_training_augmentation_draws_and_translates_on_the_host():
    aug = curla_amd.RandomTranslate((9, 11), (13, 12))
    imgs = np.random.RandomState(2).randint(1, 256, (6, 6, 9, 11), dtype=np.uint8)
    np.random.seed(23)
    out = aug.training_augmentation(imgs)
    np.random.seed(23)
    ty = np.random.randint(0, 5, 6)
    tx = np.random.randint(0, 2, 6)
    assert out.shape == (6, 6, 13, 12) and np.array_equal(out, translate_loop(imgs, ty, tx, (13, 12)))


def test_evaluation_augmentation_centres_and_an_odd_margin_floors():
    aug = curla_amd.RandomTranslate((5, 7), (8, 12))  # margins of 3 (odd) and 5 (odd)
    for dtype in (np.uint8, np.float32):
        img = np.random.RandomState(3).randint(1, 256, (6, 5, 7)).astype(dtype)
        out = aug.evaluation_augmentation(img)
        assert out.shape == (6, 8, 12) and out.dtype == dtype
        assert np.array_equal(out[:, 1:6, 2:9], img)  # top = 3 // 2, left = 5 // 2
        assert int((out != 0).sum()) == img.size
        assert np.array_equal(out, aug.translate(img[None], [1], [2])[0])
    full = np.ones((6, 8, 12), np.uint8)
    assert aug.evaluation_augmentation(full) is full  # already of the canvas size: returned unchanged
    even = curla_amd.RandomTranslate((5, 7))
    assert np.array_equal(even.evaluation_augmentation(img)[:, 4:9, 4:11], img)


# ------------------------------------------------------------------------------------------------ ReplayBuffer, host side
def _pair(**kw):
    """A translate buffer and a random_shift buffer of the same construction."""
    return (ReplayBuffer((C,) + HW, (2,), 64, B, "cpu", curla_amd.RandomTranslate(HW, OUT), **kw),
            ReplayBuffer((C,) + HW, (2,), 64, B, "cpu", curla_amd.RandomShift(HW), **kw))


def test_draw_indices_is_one_index_draw_then_three_pairs_in_range():
    rb, shift = _pair()
    rb.idx = shift.idx = 40
    np.random.seed(5)
    idxs, offs = rb.draw_indices()
    after = np.random.get_state()
    np.random.seed(5)
    want = [np.random.randint(0, 40, size=B)]
    for _ in range(3):  # obs, next_obs, pos: ty then tx
        want += [np.random.randint(0, OUT[0] - HW[0] + 1, B), np.random.randint(0, OUT[1] - HW[1] + 1, B)]
    now = np.random.get_state()
    assert np.array_equal(after[1], now[1]) and after[2] == now[2]
    assert np.array_equal(idxs, want[0]) and offs.shape == (6, B) and offs.dtype == np.int32
    for j in range(6):
        assert np.array_equal(offs[j], want[1 + j]), j
    assert offs.min() >= 0 and offs[[0, 2, 4]].max() <= OUT[0] - HW[0] and offs[[1, 3, 5]].max() <= OUT[1] - HW[1]
    assert offs.any()
    # the same seed draws the same indices for the shift buffer (its offsets have another range)
    np.random.seed(5)
    assert np.array_equal(shift.draw_indices()[0], idxs)


@pytest.mark.parametrize("kw", [{}, dict(n_step=3, discount=0.99), dict(dedup_frames=True)], ids=["plain", "n_step", "dedup"])
def test_block_layout_is_the_shifts_and_the_scratch_has_output_frames(kw):
    rb, shift = _pair(**kw)
    assert rb.block_layout() == shift.block_layout() and "cut" not in rb.block_layout()
    out_frame, frame = C * OUT[0] * OUT[1], C * HW[0] * HW[1]
    assert rb._frame == frame == shift._frame and rb._scratch_frame() == out_frame and shift._scratch_frame() == frame
    assert rb.obs_shape == (C,) + HW
    need = 3 * B * out_frame + 32
    assert rb._shift_store.shape[0] == rb.N_SAMPLE_SLOTS
    assert rb._shift_store.shape[1] == (need + 255) // 256 * 256 and rb._shift_store.stride(0) % 256 == 0
    assert shift._shift_store.shape[1] == (3 * B * frame + 32 + 255) // 256 * 256  # ... and the shift's is what it was
    _lib.set_trace_hook(lambda name, args: None)
    try:
        g, gs = rb.graph_block(0), shift.graph_block(0)
    finally:
        _lib.set_trace_hook(None)
    assert g["shift_u8"].numel() == need and gs["shift_u8"].numel() == 3 * B * frame + 32
    assert len(g["guards"]) == (4 if kw.get("dedup_frames") else 2)
    assert all(bool((x == rb.GUARD_BYTE).all()) and x.numel() >= rb.GUARD for x in g["guards"])
    if kw.get("dedup_frames"):  # the gathered stacks stay stored-frame sized
        assert g["mb_u8"].numel() == 2 * B * frame + 32 and rb._mb_store.shape[1] == 2 * B * frame + 32
    else:  # the stored rings stay (C, H, W)
        assert tuple(rb.obses.shape) == (64,) + HW + (C,) == tuple(rb.next_obses.shape)


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


def _no_other_scratch_launch(names):
    assert "curla_random_shift_u8" not in names and "curla_cutout_u8" not in names


def test_one_translate_launch_behind_the_staging_on_plain_storage():
    rb = _rb(curla_amd.RandomTranslate(HW, OUT))
    calls, sample = _traced(rb.sample_cpc_refs)
    names = [n for n, _ in calls]
    assert names == ["curla_sample_stage", "curla_translate_u8"]
    _no_other_scratch_launch(names)
    frames, idx, period, ty, tx, n, c, h, w, ho, wo, out, _ = calls[1][1]
    blk = rb._d_index[rb._sample_slot]
    assert frames == rb._both.data_ptr() and idx == blk.data_ptr() and period == 2 * B and n == 3 * B
    assert ty == blk.data_ptr() + 16 * B and tx == ty + 4 * 3 * B
    assert (c, h, w, ho, wo) == (C,) + HW + OUT
    assert out == rb._shift_store[rb._sample_slot].data_ptr()
    # the handles: an ordinary uint8 ring of 3B rows of the OUTPUT size over the scratch, zero offsets, nothing to crop
    obs, _, _, nxt, _, kw = sample
    for ref, row0 in ((obs, 0), (nxt, B), (kw["obs_pos"], 2 * B)):
        assert ref.src.data_ptr() == out and tuple(ref.src.shape) == (3 * B,) + OUT + (C,)
        assert ref.is_u8 == 1 and ref.B == B and (ref.Hc, ref.Wc) == (ref.Hs, ref.Ws) == OUT
        assert ref.idx.tolist() == list(range(row0, row0 + B)) and not ref.h1.any() and not ref.w1.any()
    assert obs.pair[0].B == 2 * B and obs.pair[0].idx.tolist() == list(range(2 * B)) and obs.pair[1] is nxt
    # the next sample goes to the other slot's scratch
    calls, _ = _traced(rb.sample_cpc_refs)
    assert calls[1][1][11] == rb._shift_store[rb._sample_slot].data_ptr() != out
    # sample_cpc(): the same launch, then one crop_nchw per tensor from the scratch with zero offsets, to (Ho, Wo)
    calls, tensors = _traced(rb.sample_cpc)
    names = [n for n, _ in calls]
    assert names == ["curla_sample_stage", "curla_translate_u8"] + ["curla_crop_nchw"] * 3
    scratch = rb._shift_store[rb._sample_slot].data_ptr()
    assert all(a[0] == scratch and a[2] == rb._shift_zero.data_ptr() == a[3] for nm, a in calls if nm == "curla_crop_nchw")
    assert tuple(tensors[0].shape) == (B, C) + OUT == tuple(tensors[3].shape) == tuple(tensors[5]["obs_pos"].shape)


def test_on_the_frame_store_the_translate_comes_behind_the_two_gathers():
    rb = _rb(curla_amd.RandomTranslate(HW, OUT), dedup_frames=True)
    calls, _ = _traced(rb.sample_cpc_refs)
    names = [n for n, _ in calls]
    assert names == ["curla_sample_stage", "curla_gather_stacks", "curla_gather_stacks", "curla_translate_u8"]
    a = calls[-1][1]
    assert a[0] == rb._mb_store[rb._sample_slot].data_ptr() and a[1] is None and a[2] == 2 * B and a[5] == 3 * B
    assert tuple(a[6:11]) == (C,) + HW + OUT


def test_rings_in_two_allocations_take_one_launch_per_tensor():
    hw, out_hw = (11, 13), (15, 14)
    rb = _rb(curla_amd.RandomTranslate(hw, out_hw), obs_shape=(3,) + hw, cap=7, batch=4, n_add=5)
    assert (7 * 429) % 4 != 0 and rb._both is None  # no dword-aligned second ring
    calls, _ = _traced(rb.sample_cpc_refs)
    names = [n for n, _ in calls]
    assert names == ["curla_sample_stage"] + ["curla_translate_u8"] * 3
    _no_other_scratch_launch(names)
    moves = [a for n, a in calls if n == "curla_translate_u8"]
    out0 = rb._shift_store[rb._sample_slot].data_ptr()
    blk = rb._d_index[rb._sample_slot].data_ptr()
    assert [a[0] for a in moves] == [rb.obses.data_ptr(), rb.next_obses.data_ptr(), rb.obses.data_ptr()]
    assert [a[1] for a in moves] == [blk, blk, blk]
    assert [a[11] for a in moves] == [out0 + j * 4 * 3 * 15 * 14 for j in range(3)]  # strides of OUTPUT frames
    assert [a[3] for a in moves] == [blk + 16 * 4 + 4 * 4 * j for j in range(3)]
    assert [a[4] for a in moves] == [blk + 16 * 4 + 4 * 4 * (3 + j) for j in range(3)]
    assert all(a[2] == 4 and a[5] == 4 for a in moves)
    assert not rb.graph_supported()


def test_n_step_composes_inside_the_staging_launch_in_front_of_the_translate():
    rb = _rb(curla_amd.RandomTranslate(HW, OUT), n_step=3, discount=0.99)
    calls, _ = _traced(rb.sample_cpc_refs)
    assert [n for n, _ in calls] == ["curla_sample_stage_nstep", "curla_translate_u8"]
    a = calls[1][1]
    assert a[1] == rb._d_index[rb._sample_slot].data_ptr() and a[2] == 2 * B and a[5] == 3 * B


@pytest.mark.parametrize("name", ["identity", "random_crop", "random_shift", "cutout_color", "color_jiggle", "noisy_cover"])
def test_the_other_buffers_never_launch_a_translate(name):
    aug = curla_amd.make_augmentor(name, HW, (28, 34) if name == "random_crop" else None)
    rb = _rb(aug)
    calls, _ = _traced(lambda: (rb.sample_cpc_refs(), rb.sample_cpc()))
    names = [n for n, _ in calls]
    assert "curla_sample_stage" in names and "curla_translate_u8" not in names
    assert hasattr(rb, "_shift_store") == (name in ("random_shift", "cutout_color")) and not isinstance(rb.augmentor, curla_amd.RandomTranslate)
    if hasattr(rb, "_shift_store"):  # the scratch of a shift / cutout keeps frames of the stored size
        assert rb._scratch_frame() == rb._frame
        assert rb._shift_store.shape[1] == (3 * B * rb._frame + 32 + 255) // 256 * 256


def test_graph_slot_records_the_translate_behind_staging_and_gathers():
    for dedup in (False, True):
        rb = _rb(curla_amd.RandomTranslate(HW, OUT), dedup_frames=dedup)
        _, g = _traced(lambda: rb.graph_block(0))
        before = np.random.get_state()
        calls, (obs, _, _, nxt, _, kw) = _traced(lambda: rb.graph_refs(0))
        now = np.random.get_state()
        assert np.array_equal(before[1], now[1]) and before[2] == now[2]
        assert [n for n, _ in calls] == ["curla_sample_stage"] + ["curla_gather_stacks"] * (2 if dedup else 0) + ["curla_translate_u8"]
        a = calls[-1][1]
        dev = g["dev"].data_ptr()
        assert (a[3], a[4]) == (dev + 16 * B, dev + 28 * B) and (a[2], a[5]) == (2 * B, 3 * B)
        assert a[11] == g["shift_u8"].data_ptr() and tuple(a[6:11]) == (C,) + HW + OUT
        assert (a[0], a[1]) == ((g["mb_u8"].data_ptr(), None) if dedup else (rb._both.data_ptr(), dev))
        for ref, row0 in ((obs, 0), (nxt, B), (kw["obs_pos"], 2 * B)):
            assert ref.src.data_ptr() == g["shift_u8"].data_ptr() and ref.is_u8 == 1 and ref.guard is None
            assert (ref.Hc, ref.Wc) == OUT and ref.idx.tolist() == list(range(row0, row0 + B))


def test_ops_translate_checks_shapes_before_any_launch():
    from curla_amd import ops
    ring = torch.zeros((4, 5, 7, 3), dtype=torch.uint8)
    off = torch.zeros(4, dtype=torch.int32)
    out = torch.zeros((4, 8, 9, 3), dtype=torch.uint8)
    calls = []
    _lib.set_trace_hook(lambda name, args: calls.append((name, args)))
    try:
        ops.translate_u8(ring, None, 4, off, off, 4, out)
        assert calls[-1][0] == "curla_translate_u8" and tuple(calls[-1][1][5:11]) == (4, 3, 5, 7, 8, 9)
        del calls[:]
        for bad in (dict(out=torch.zeros((4, 4, 9, 3), dtype=torch.uint8)),      # a canvas lower than the frame
                    dict(out=torch.zeros((4, 8, 6, 3), dtype=torch.uint8)),      # ... narrower
                    dict(out=torch.zeros((4, 8, 9, 4), dtype=torch.uint8)),      # another channel count
                    dict(out=torch.zeros((3, 8, 9, 3), dtype=torch.uint8)),      # fewer samples than n
                    dict(out=torch.zeros((4, 8, 9, 3), dtype=torch.float32)),    # dtype
                    dict(ty=torch.zeros(3, dtype=torch.int32)),                  # too few offsets
                    dict(tx=torch.zeros(4, dtype=torch.int64)),                  # dtype
                    dict(idx=torch.zeros(3, dtype=torch.int64)),                 # too few rows for the period
                    dict(idx=torch.zeros(4, dtype=torch.int32))):
            kw = dict(idx=None, ty=off, tx=off, out=out)
            kw.update(bad)
            with pytest.raises(_lib.CurlaHipError):
                ops.translate_u8(ring, kw["idx"], 4, kw["ty"], kw["tx"], 4, kw["out"])
        assert calls == []
    finally:
        _lib.set_trace_hook(None)
    with pytest.raises(_lib.CurlaHipError):  # without the hook a CPU tensor is refused
        ops.translate_u8(ring, None, 4, off, off, 4, out)


# ------------------------------------------------------------------------------------------------ agent
def test_batched_acting_accepts_both_sizes_and_names_them():
    aug = curla_amd.RandomTranslate(HW, OUT)
    curla_amd.set_seed_everywhere(1)
    agent = curla_amd.CurlSacAgent((C,) + OUT, (2,), "cpu", aug, hidden_dim=64, **HP)
    assert agent._act_windows() == {OUT: (0, 0), HW: None}
    frames = np.random.RandomState(4).randint(1, 256, (3, C) + HW, dtype=np.uint8)
    want = np.stack([aug.evaluation_augmentation(f) for f in frames])
    _lib.set_trace_hook(lambda name, args: None)
    try:
        for x in (frames, list(frames), torch.from_numpy(frames), frames.astype(np.float32)):
            got, shape, window = agent._act_batch_args(x, None)
            assert shape == (3, C) + OUT and window == (0, 0)
            assert np.array_equal(np.asarray(got), want) and np.asarray(got).dtype == np.asarray(x[0]).dtype
        same, shape, window = agent._act_batch_args(want, None)
        assert same is want and shape == want.shape and window == (0, 0)
        with pytest.raises(ValueError) as e:
            agent._act_batch_args(np.zeros((3, C, 36, 40), np.uint8), None)
        assert str(OUT) in str(e.value) and str(HW) in str(e.value)
    finally:
        _lib.set_trace_hook(None)
    # an odd margin floors like evaluation_augmentation; other augmentations accept what they accepted
    odd = curla_amd.CurlSacAgent((C, 37, 45), (2,), "cpu", curla_amd.RandomTranslate(HW, (37, 45)), hidden_dim=64, **HP)
    assert odd._act_windows() == {(37, 45): (0, 0), HW: None}
    # margins of 0 and 1: the frame sits at (0, 0) of a larger canvas, and is still centred, not taken for a window
    for out_hw in ((35, 40), (34, 41), (35, 41)):
        aug1 = curla_amd.RandomTranslate(HW, out_hw)
        tight = curla_amd.CurlSacAgent((C,) + out_hw, (2,), "cpu", aug1, hidden_dim=64, **HP)
        assert tight._act_windows() == {out_hw: (0, 0), HW: None}
        want1 = np.stack([aug1.evaluation_augmentation(f) for f in frames])
        assert want1.shape == (3, C) + out_hw and np.array_equal(want1[:, :, :34, :40], frames)
        _lib.set_trace_hook(lambda name, args: None)
        try:
            for x in (frames, list(frames), torch.from_numpy(frames), frames.astype(np.float32)):
                got, shape, window = tight._act_batch_args(x, None)
                assert shape == (3, C) + out_hw and window == (0, 0) and np.array_equal(np.asarray(got), want1)
        finally:
            _lib.set_trace_hook(None)
    same = curla_amd.CurlSacAgent((C,) + HW, (2,), "cpu", curla_amd.RandomTranslate(HW, HW), hidden_dim=64, **HP)
    assert same._act_windows() == {HW: (0, 0)}
    crop = curla_amd.CurlSacAgent((C, 28, 34), (2,), "cpu", curla_amd.RandomCrop(HW, (28, 34)), hidden_dim=64, **HP)
    assert crop._act_windows() == {(28, 34): (0, 0), HW: (3, 3)}
    shift = curla_amd.CurlSacAgent((C,) + HW, (2,), "cpu", curla_amd.RandomShift(HW), hidden_dim=64, **HP)
    assert shift._act_windows() == {HW: (0, 0)}


def test_enable_update_graphs_refusal_names_the_augmentation():
    """(The refusal itself needs the device, tests/test_gpu_translate.py; its text is the agent's.)"""
    import inspect
    text = inspect.getsource(curla_amd.CurlSacAgent.enable_update_graphs)
    assert re.search(r"RandomShift, RandomCutout, RandomTranslate or identity", text)


# ------------------------------------------------------------------------------------------------ ABI
def test_header_declares_the_entry_point_and_the_abi_number_stays():
    with open(os.path.join(ROOT, "include", "curla_hip.h")) as f:
        header = f.read()
    m = re.search(r"\bint\s+curla_translate_u8\s*\(([^)]*)\)\s*;", header)
    assert m, "include/curla_hip.h does not declare curla_translate_u8"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == len(_lib.SIGNATURES["curla_translate_u8"]) == 13
    want = ("frames", "idx", "period", "ty", "tx", "n", "C", "H", "W", "Ho", "Wo", "out", "stream")
    assert tuple(p.split()[-1].lstrip("*") for p in params) == want
    for p, t in zip(params, _lib.SIGNATURES["curla_translate_u8"]):
        assert ("*" in p) == (t is _lib.vp), p
        if t is not _lib.vp:
            assert p.startswith("int ") and t is _lib.c_int
    assert re.search(r"#define\s+CURLA_ABI_VERSION\s+8\b", header) and _lib.ABI_VERSION == 8
