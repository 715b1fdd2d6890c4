"""``RandomCutout`` (RAD's cutout / cutout-color: one box per sample painted black or in one random colour) without a
GPU: the augmentor's API, the order of its NumPy draws, the host restatement against a per-pixel loop, the minibatch
block's layout (unchanged for every other augmentor), where the cutout launch sits in the launch schedule (trace hook:
nothing is computed) and the C ABI's declaration."""
import os
import re

import numpy as np
import pytest
import torch

import curla_amd
from curla_amd import _lib
from curla_amd.utils import ReplayBuffer

C, HW, B, CAP = 9, (34, 40), 8, 32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cut_loop(imgs, y0, x0, bh, bw, rgb):
    """The restatement, pixel by pixel: (B, C, H, W) in and out; rgb (B, 3) or None = black."""
    out = imgs.copy()
    n, c, h, w = imgs.shape
    for b in range(n):
        for ch in range(c):
            for y in range(h):
                for x in range(w):
                    if y0[b] <= y < y0[b] + bh[b] and x0[b] <= x < x0[b] + bw[b]:
                        out[b, ch, y, x] = 0 if rgb is None else rgb[b][ch % 3]
    return out


# ------------------------------------------------------------------------------------------------ augmentor API
def test_augmentor_api_and_validation():
    aug = curla_amd.RandomCutout(HW)
    assert (aug.min_cut, aug.max_cut, aug.color) == (10, 30, False)
    assert aug.input_shape == HW and aug.output_shape == HW
    assert isinstance(aug, curla_amd.IdentityAugmentation) and not isinstance(aug, (curla_amd.RandomCrop, curla_amd.RandomShift))
    img = np.random.RandomState(0).randint(0, 256, (C,) + HW, dtype=np.uint8)
    assert aug.evaluation_augmentation(img) is img
    assert curla_amd.RandomCutout(HW, 1, 34, True).color is True  # max_cut == min(H, W) is allowed
    for kw in (dict(min_cut=True), dict(max_cut=True), dict(min_cut=2.0), dict(max_cut=12.5), dict(min_cut=0),
               dict(min_cut=-1), dict(min_cut=12, max_cut=11), dict(max_cut=35), dict(min_cut="3"), dict(max_cut=None)):
        with pytest.raises(ValueError):
            curla_amd.RandomCutout(HW, **kw)
    with pytest.raises(ValueError):
        curla_amd.make_augmentor("cutout", HW, max_cut=41)


def test_make_augmentor_names_and_keyword_only_parameters():
    a = curla_amd.make_augmentor("cutout", HW)
    b = curla_amd.make_augmentor("cutout_color", HW, min_cut=3, max_cut=7)
    assert type(a) is curla_amd.RandomCutout and (a.min_cut, a.max_cut, a.color) == (10, 30, False)
    assert type(b) is curla_amd.RandomCutout and (b.min_cut, b.max_cut, b.color) == (3, 7, True)
    from curla_amd.augmentations import RandomCutout
    assert RandomCutout is curla_amd.RandomCutout and "RandomCutout" in curla_amd.__all__
    with pytest.raises(TypeError):
        curla_amd.make_augmentor("cutout", HW, None, 4, 3, 7)  # pad, min_cut, max_cut are keyword-only
    # the existing names build what they built
    assert curla_amd.make_augmentor("random_shift", HW, pad=2).pad == 2
    assert tuple(curla_amd.make_augmentor("random_crop", HW, (28, 30)).output_shape) == (28, 30)
    with pytest.raises(ValueError):
        curla_amd.make_augmentor("cutout_colour", HW)


# ------------------------------------------------------------------------------------------------ draws
@pytest.mark.parametrize("color", [False, True])
def test_draw_boxes_consumes_the_stream_in_the_stated_order(color):
    h, w = HW
    aug = curla_amd.RandomCutout(HW, min_cut=3, max_cut=30, color=color)
    n = 3000
    np.random.seed(17)
    y0, x0, bh, bw, rgb = aug.draw_boxes(n)
    after = np.random.get_state()
    np.random.seed(17)
    want_bh = np.random.randint(3, 31, n)
    want_bw = np.random.randint(3, 31, n)
    want_y0 = np.random.randint(0, h - want_bh + 1)
    want_x0 = np.random.randint(0, w - want_bw + 1)
    if color:
        want_rgb = np.random.randint(0, 256, (n, 3))
        assert rgb.shape == (n, 3) and np.array_equal(rgb, want_rgb) and rgb.min() == 0 and rgb.max() == 255
    else:
        assert rgb is None  # nothing drawn for it: the stream stands where four draws leave it
    now = np.random.get_state()
    assert np.array_equal(after[1], now[1]) and after[2] == now[2]
    for got, want in ((bh, want_bh), (bw, want_bw), (y0, want_y0), (x0, want_x0)):
        assert got.shape == (n,) and np.array_equal(got, want)
    # always inside the frame, and the whole range of sizes and of positions at a given size occurs
    assert bh.min() == 3 and bh.max() == 30 and bw.min() == 3 and bw.max() == 30
    assert (y0 >= 0).all() and (y0 + bh <= h).all() and (x0 >= 0).all() and (x0 + bw <= w).all()
    assert (y0 + bh == h).any() and (x0 + bw == w).any() and (y0 == 0).any() and (x0 == 0).any()


def test_draw_indices_is_one_index_draw_then_three_box_draws():
    h, w = HW
    for color in (False, True):
        rb = ReplayBuffer((C,) + HW, (2,), 64, B, "cpu", curla_amd.RandomCutout(HW, 4, 12, color))
        rb.idx = 40
        np.random.seed(5)
        idxs, offs = rb.draw_indices()
        after = np.random.get_state()
        np.random.seed(5)
        assert np.array_equal(idxs, np.random.randint(0, 40, size=B))
        assert offs.shape == (12, B) and offs.dtype == np.int32
        for j in range(3):
            bh = np.random.randint(4, 13, B)
            bw = np.random.randint(4, 13, B)
            y0 = np.random.randint(0, h - bh + 1)
            x0 = np.random.randint(0, w - bw + 1)
            assert np.array_equal(offs[2 * j], y0) and np.array_equal(offs[2 * j + 1], x0)
            assert np.array_equal(offs[6 + 2 * j], bh | (bw << 16))
            if color:
                rgb = np.random.randint(0, 256, (B, 3))
                assert np.array_equal(offs[6 + 2 * j + 1], rgb[:, 0] | (rgb[:, 1] << 8) | (rgb[:, 2] << 16))
            else:
                assert not offs[6 + 2 * j + 1].any()
        now = np.random.get_state()
        assert np.array_equal(after[1], now[1]) and after[2] == now[2]
    # every other augmentor still returns six rows
    for name in ("identity", "random_crop", "random_shift", "color_jiggle", "noisy_cover"):
        other = ReplayBuffer((C,) + HW, (2,), 64, B, "cpu", curla_amd.make_augmentor(name, HW))
        other.idx = 40
        assert other.draw_indices()[1].shape == (6, B)


# ------------------------------------------------------------------------------------------------ host restatement
def test_cut_matches_the_per_pixel_loop():
    n, c, h, w = 3, 6, 5, 7
    rs = np.random.RandomState(1)
    imgs = rs.randint(0, 256, (n, c, h, w), dtype=np.uint8)
    untouched = imgs.copy()
    boxes = [  # (y0, x0, bh, bw) per sample
        [(0, 0, 5, 7), (0, 0, 1, 1), (0, 6, 1, 1)],      # the full frame, 1x1 at two corners
        [(4, 0, 1, 1), (4, 6, 1, 1), (1, 2, 3, 4)],      # 1x1 at the other two corners, an inner box
        [(2, 0, 2, 7), (0, 3, 5, 2), (3, 5, 2, 2)],      # full width, full height, the bottom-right corner
    ]
    for case in boxes:
        y0, x0, bh, bw = (np.array(v) for v in zip(*case))
        rgb = rs.randint(0, 256, (n, 3))
        for colours in (None, rgb):
            got = curla_amd.RandomCutout.cut(imgs, y0, x0, bh, bw, colours)
            assert got.dtype == imgs.dtype and got.shape == imgs.shape
            assert np.array_equal(got, cut_loop(imgs, y0, x0, bh, bw, colours))
    full = curla_amd.RandomCutout.cut(imgs, [0] * n, [0] * n, [h] * n, [w] * n, rgb)
    assert all((full[b, ch] == rgb[b, ch % 3]).all() for b in range(n) for ch in range(c))
    assert not np.array_equal(imgs, full) and np.array_equal(imgs, untouched)  # the argument is left alone


def test_training_augmentation_draws_and_cuts_on_the_host():
    aug = curla_amd.RandomCutout((9, 11), 2, 5, color=True)
    imgs = np.random.RandomState(2).randint(0, 256, (6, 6, 9, 11), dtype=np.uint8)
    np.random.seed(23)
    out = aug.training_augmentation(imgs)
    np.random.seed(23)
    y0, x0, bh, bw, rgb = aug.draw_boxes(6)
    assert np.array_equal(out, cut_loop(imgs, y0, x0, bh, bw, rgb)) and not np.array_equal(out, imgs)


# ------------------------------------------------------------------------------------------------ block layout
def _literal_layout(b, n_step, aug=None, k=3):
    """What block_layout() returned before RandomCutout, from B."""
    n = 2 * b * 8 + 6 * b * 4
    lay = dict(idx=0, offs=2 * b * 8, offs_end=n, aug=None, aug_stride=0, aug_order=None, aug_rng=None)
    if aug == "color_jiggle":
        lay.update(aug=n, aug_stride=16 * b * k + 16, aug_order=16 * b * k)
        n += 3 * (16 * b * k + 16)
    elif aug == "noisy_cover":
        lay.update(aug=n, aug_stride=32, aug_rng=16)
        n += 96
    if n_step > 1:
        lay["next_row"] = n
        n += 8 * b
    lay.update(nbytes=n, tail=n, graph_nbytes=n + 80)
    return lay


@pytest.mark.parametrize("n_step", [1, 3])
def test_block_layout_of_the_other_augmentors_is_what_it_was(n_step):
    kw = dict(n_step=n_step, discount=0.99) if n_step > 1 else {}
    for name, staged in (("identity", False), ("random_crop", False), ("random_shift", False), ("color_jiggle", True),
                         ("noisy_cover", True)):
        rb = ReplayBuffer((C,) + HW, (2,), CAP, B, "cpu", curla_amd.make_augmentor(name, HW), **kw)
        if staged:  # (a CPU buffer cannot be constructed with staged NoisyCover: the flag is what block_layout reads)
            rb.staged_aug = True
        assert rb.block_layout() == _literal_layout(B, n_step, name if staged else None), name
        assert "cut" not in rb.block_layout()


@pytest.mark.parametrize("n_step", [1, 3])
def test_block_layout_of_a_cutout_appends_the_cut_section(n_step):
    kw = dict(n_step=n_step, discount=0.99) if n_step > 1 else {}
    rb = ReplayBuffer((C,) + HW, (2,), CAP, B, "cpu", curla_amd.make_augmentor("cutout_color", HW), **kw)
    lay = rb.block_layout()
    base = _literal_layout(B, 1)
    assert lay["cut"] == lay["offs_end"] == base["offs_end"] == 40 * B and lay["idx"] == 0 and lay["offs"] == 16 * B
    end = lay["cut"] + 2 * 3 * B * 4
    if n_step > 1:
        assert lay["next_row"] == end and lay["nbytes"] == end + 8 * B
    else:
        assert "next_row" not in lay and lay["nbytes"] == end
    assert lay["nbytes"] % 8 == 0 and lay["tail"] == lay["nbytes"] and lay["graph_nbytes"] == lay["nbytes"] + rb.GRAPH_TAIL
    # the block as the kernels read it: offsets where crop offsets sit, then the sizes and the colours as runs of 3B
    idxs = np.arange(B)[::-1].copy()
    offs = np.arange(12 * B, dtype=np.int32).reshape(12, B)
    host = torch.zeros(lay["nbytes"], dtype=torch.uint8)
    rb._fill_index_block(host, idxs, offs)
    raw = host.numpy()
    assert raw[:16 * B].view(np.int64).tolist() == idxs.tolist() + (idxs + CAP).tolist()
    o32 = raw[16 * B:40 * B].view(np.int32)
    assert o32[:3 * B].tolist() == np.concatenate([offs[0], offs[2], offs[4]]).tolist()
    assert o32[3 * B:].tolist() == np.concatenate([offs[1], offs[3], offs[5]]).tolist()
    c32 = raw[lay["cut"]:end].view(np.int32)
    assert c32[:3 * B].tolist() == np.concatenate([offs[6], offs[8], offs[10]]).tolist()
    assert c32[3 * B:].tolist() == np.concatenate([offs[7], offs[9], offs[11]]).tolist()
    with pytest.raises(ValueError):
        rb._fill_index_block(host, idxs, offs[:6])


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


def test_one_cutout_launch_behind_the_staging_on_plain_storage():
    rb = _rb(curla_amd.make_augmentor("cutout_color", HW))
    calls, sample = _traced(rb.sample_cpc_refs)
    assert [n for n, _ in calls] == ["curla_sample_stage", "curla_cutout_u8"]
    frames, idx, period, y0, x0, size, rgb, n, c, h, w, out, _ = calls[1][1]
    blk = rb._d_index[rb._sample_slot]
    lay = rb.block_layout()
    assert frames == rb._both.data_ptr() and idx == blk.data_ptr() and period == 2 * B and n == 3 * B
    assert y0 == blk.data_ptr() + lay["offs"] and x0 == y0 + 4 * 3 * B
    assert size == blk.data_ptr() + lay["cut"] and rgb == size + 4 * 3 * B
    assert (c, h, w) == (C,) + HW
    assert out == rb._shift_store[rb._sample_slot].data_ptr() and rb._shift_store.stride(0) % 256 == 0
    assert rb._shift_store.shape[0] == rb.N_SAMPLE_SLOTS and rb._shift_store.shape[1] >= 3 * B * C * HW[0] * HW[1] + 32
    # the handles: an ordinary uint8 ring of 3B rows over the scratch, zero offsets, the pair over the first 2B
    obs, _, _, nxt, _, kw = sample
    for ref, row0 in ((obs, 0), (nxt, B), (kw["obs_pos"], 2 * B)):
        assert ref.src.data_ptr() == out and ref.is_u8 == 1 and ref.B == B and (ref.Hc, ref.Wc) == HW
        assert ref.idx.tolist() == list(range(row0, row0 + B)) and not ref.h1.any() and not ref.w1.any()
    assert obs.pair[0].B == 2 * B and obs.pair[0].idx.tolist() == list(range(2 * B)) and obs.pair[1] is nxt
    # the next sample goes to the other slot's scratch
    calls, _ = _traced(rb.sample_cpc_refs)
    assert calls[1][1][11] == rb._shift_store[rb._sample_slot].data_ptr() != out
    # sample_cpc(): the same launch, then one crop_nchw per tensor from the scratch with zero offsets
    calls, _ = _traced(rb.sample_cpc)
    names = [n for n, _ in calls]
    assert names == ["curla_sample_stage", "curla_cutout_u8"] + ["curla_crop_nchw"] * 3
    scratch = rb._shift_store[rb._sample_slot].data_ptr()
    assert all(a[0] == scratch and a[2] == rb._shift_zero.data_ptr() == a[3] for nm, a in calls if nm == "curla_crop_nchw")


def test_on_the_frame_store_the_cutout_comes_behind_the_two_gathers():
    rb = _rb(curla_amd.make_augmentor("cutout", HW), dedup_frames=True)
    calls, _ = _traced(rb.sample_cpc_refs)
    assert [n for n, _ in calls] == ["curla_sample_stage", "curla_gather_stacks", "curla_gather_stacks", "curla_cutout_u8"]
    a = calls[-1][1]
    assert a[0] == rb._mb_store[rb._sample_slot].data_ptr() and a[1] is None and a[2] == 2 * B and a[7] == 3 * B


def test_rings_in_two_allocations_take_one_launch_per_tensor():
    hw = (11, 13)
    aug = curla_amd.make_augmentor("cutout_color", hw, min_cut=2, max_cut=5)
    rb = _rb(aug, obs_shape=(3,) + hw, cap=7, batch=4, n_add=5)  # 7 * 429 bytes: no dword-aligned second ring
    assert (7 * 429) % 4 != 0 and rb._both is None
    calls, _ = _traced(rb.sample_cpc_refs)
    cuts = [a for n, a in calls if n == "curla_cutout_u8"]
    assert [n for n, _ in calls] == ["curla_sample_stage"] + ["curla_cutout_u8"] * 3
    out0 = rb._shift_store[rb._sample_slot].data_ptr()
    blk = rb._d_index[rb._sample_slot].data_ptr()
    lay = rb.block_layout()
    assert [a[0] for a in cuts] == [rb.obses.data_ptr(), rb.next_obses.data_ptr(), rb.obses.data_ptr()]
    assert [a[1] for a in cuts] == [blk, blk, blk]  # (1-step: next_obs at the sampled rows)
    assert [a[11] for a in cuts] == [out0 + j * 4 * 429 for j in range(3)]
    assert [a[3] for a in cuts] == [blk + lay["offs"] + 4 * 4 * j for j in range(3)]
    assert [a[5] for a in cuts] == [blk + lay["cut"] + 4 * 4 * j for j in range(3)]
    assert [a[6] for a in cuts] == [blk + lay["cut"] + 4 * 4 * (3 + j) for j in range(3)]
    assert all(a[2] == 4 and a[7] == 4 for a in cuts)
    assert not rb.graph_supported()


def test_n_step_composes_inside_the_staging_launch_in_front_of_the_cutout():
    rb = _rb(curla_amd.make_augmentor("cutout_color", HW), n_step=3, discount=0.99)
    calls, _ = _traced(rb.sample_cpc_refs)
    assert [n for n, _ in calls] == ["curla_sample_stage_nstep", "curla_cutout_u8"]
    lay = rb.block_layout()
    assert calls[0][1][3] == lay["next_row"] == lay["cut"] + 24 * B and calls[0][1][2] == lay["nbytes"]
    a = calls[1][1]
    assert a[1] == rb._d_index[rb._sample_slot].data_ptr() and a[2] == 2 * B and a[7] == 3 * B


@pytest.mark.parametrize("name", ["identity", "random_crop", "random_shift", "color_jiggle", "noisy_cover"])
def test_the_other_buffers_never_launch_a_cutout(name):
    aug = curla_amd.make_augmentor(name, HW, (28, 34) if name == "random_crop" else None)
    rb = _rb(aug)
    calls, _ = _traced(lambda: (rb.sample_cpc_refs(), rb.sample_cpc()))
    names = [n for n, _ in calls]
    assert "curla_sample_stage" in names and "curla_cutout_u8" not in names
    assert hasattr(rb, "_shift_store") == (name == "random_shift")
    assert all("shift_u8" in s for s in rb._sample_slots) == (name == "random_shift")


def test_graph_slot_records_the_cutout_behind_staging_and_gathers():
    for dedup in (False, True):
        rb = _rb(curla_amd.make_augmentor("cutout_color", HW), dedup_frames=dedup)
        frame = C * HW[0] * HW[1]
        _, g = _traced(lambda: rb.graph_block(0))
        assert g["shift_u8"].numel() == 3 * B * frame + 32 and not g["shift_u8"].any()
        assert len(g["guards"]) == (4 if dedup else 2)
        assert all(bool((x == rb.GUARD_BYTE).all()) and x.numel() >= rb.GUARD for x in g["guards"])
        before = np.random.get_state()
        calls, _ = _traced(lambda: rb.graph_refs(0))
        now = np.random.get_state()
        assert np.array_equal(before[1], now[1]) and before[2] == now[2]
        assert [n for n, _ in calls] == ["curla_sample_stage"] + ["curla_gather_stacks"] * (2 if dedup else 0) + ["curla_cutout_u8"]
        a = calls[-1][1]
        dev, lay = g["dev"].data_ptr(), rb.block_layout()
        assert (a[3], a[4], a[5], a[6]) == (dev + 16 * B, dev + 28 * B, dev + lay["cut"], dev + lay["cut"] + 12 * B)
        assert (a[2], a[7]) == (2 * B, 3 * B) and a[11] == g["shift_u8"].data_ptr()
        assert (a[0], a[1]) == ((g["mb_u8"].data_ptr(), None) if dedup else (rb._both.data_ptr(), dev))
        assert g["host"].numel() == lay["graph_nbytes"]


# ------------------------------------------------------------------------------------------------ ABI
def test_header_declares_the_entry_point_and_the_abi_number_stays():
    with open(os.path.join(ROOT, "include", "curla_hip.h")) as f:
        header = f.read()
    m = re.search(r"\bint\s+curla_cutout_u8\s*\(([^)]*)\)\s*;", header)
    assert m, "include/curla_hip.h does not declare curla_cutout_u8"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == len(_lib.SIGNATURES["curla_cutout_u8"]) == 13
    want = ("frames", "idx", "period", "y0", "x0", "size", "rgb", "n", "C", "H", "W", "out", "stream")
    assert tuple(p.split()[-1].lstrip("*") for p in params) == want
    for p, t in zip(params, _lib.SIGNATURES["curla_cutout_u8"]):
        assert ("*" in p) == (t is _lib.vp), p
        if t is not _lib.vp:
            assert p.startswith("int ") and t is _lib.c_int
    assert re.search(r"#define\s+CURLA_ABI_VERSION\s+8\b", header) and _lib.ABI_VERSION == 8
