"""``RandomAffine`` (rotate, zoom and sub-pixel shift on the uint8 path) without a GPU: the augmentor's API and validation,
the order of its NumPy draws, its words against the formula, the host restatement ``warp`` against the independent one of
tests/_affine_ref.py and against slicing, ``np.rot90``, ``RandomShift.shift`` and the half-pixel average, ``make_augmentor``,
``Compose`` refusing it, where its launch sits in the launch schedule (trace hook: nothing is computed) and the C ABI's
declaration."""
import os
import re

import numpy as np
import pytest
import torch

import curla_amd
from curla_amd import _lib
from tests._affine_ref import GARBAGE, IDENTITY, affine_nhwc, affine_pixel, kernel_word_sets, words_of, wrap32
from tests.test_translate_host import _rb, _traced

C, HW, B = 9, (34, 40), 8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRIES = [(8, 8, 9), (7, 7, 3), (5, 7, 3)]  # (H, W, C)
W180, W90 = [-65536, 0, 458752, 0, -65536, 458752], [0, -65536, 458752, 65536, 0, 0]  # on (8, 8)


def _same_stream(a, b):
    return np.array_equal(a[1], b[1]) and a[2] == b[2]


def _imgs(geo, n, seed=0):
    H, W, Cc = geo
    return np.random.RandomState(seed + H * W + Cc).randint(0, 256, (n, Cc, H, W), dtype=np.uint8)


def _warp_ref(imgs, words, fill):
    """tests/_affine_ref.py on (B, C, H, W), words [6][B]."""
    nhwc = np.ascontiguousarray(imgs.transpose(0, 2, 3, 1))
    return affine_nhwc(nhwc, np.asarray(words, dtype=object).T.tolist(), 1 if fill == "edge" else 0).transpose(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------ augmentor API
def test_constructor_defaults_refusals_and_exports():
    aug = curla_amd.RandomAffine(HW)
    assert (aug.degrees, aug.scale, aug.translate, aug.fill, aug.p) == (10.0, (0.9, 1.1), 0.05, "edge", 1.0)
    assert aug.input_shape == HW == aug.output_shape and isinstance(aug, curla_amd.IdentityAugmentation)
    assert (aug.sample_kind, aug.index_rows) == ("scratch", 6)
    assert not isinstance(aug, (curla_amd.RandomShift, curla_amd.RandomRotate, curla_amd.Compose))
    a = curla_amd.RandomAffine([np.int64(34), 40], 180, [1, np.float32(2.0)], 0.5, "zero", 0)
    assert (a.input_shape, a.degrees, a.scale, a.translate, a.fill, a.p) == ((34, 40), 180.0, (1.0, 2.0), 0.5, "zero", 0.0)
    assert curla_amd.RandomAffine(HW, 0, (1, 1), 0).degrees == 0.0
    for bad_shape in ((34,), (3, 34, 40), (34.0, 40), (True, 40), ("34", 40)):
        with pytest.raises(ValueError):
            curla_amd.RandomAffine(bad_shape)
    for bad in (dict(degrees=-1), dict(degrees=180.5), dict(degrees=float("nan")), dict(degrees=float("inf")),
                dict(degrees=True), dict(degrees="10"), dict(degrees=None), dict(degrees=(5, 10)),
                dict(scale=1.0), dict(scale=(1.0,)), dict(scale=(0.9, 1.0, 1.1)), dict(scale=(0.0, 1.0)),
                dict(scale=(-0.5, 1.0)), dict(scale=(1.1, 0.9)), dict(scale=(0.9, float("inf"))),
                dict(scale=(float("nan"), 1.0)), dict(scale=(True, 1.0)), dict(scale=("0.9", 1.1)), dict(scale="ab"),
                dict(scale=None),
                dict(translate=-0.01), dict(translate=0.51), dict(translate=float("nan")), dict(translate=True),
                dict(translate="0.1"), dict(translate=None),
                dict(fill="reflect"), dict(fill="Edge"), dict(fill=1), dict(fill=None), dict(fill=True),
                dict(p=-0.1), dict(p=1.5), dict(p=True), dict(p="1"), dict(p=None), dict(p=float("nan"))):
        with pytest.raises(ValueError):
            curla_amd.RandomAffine(HW, **bad)
    from curla_amd.augmentations import RandomAffine
    assert RandomAffine is curla_amd.RandomAffine and "RandomAffine" in curla_amd.__all__


def test_the_wrap_bound():
    """65536 (g (H + W) (1.5 + translate) + max(H, W) / 2 + 1) < 2^31 with g = 1 / scale[0]."""
    curla_amd.RandomAffine((84, 84))
    curla_amd.RandomAffine((1024, 1024), scale=(0.25, 1.0))
    with pytest.raises(ValueError):
        curla_amd.RandomAffine((4096, 4096), scale=(0.1, 1))
    # the bound is sufficient: at its extremes the words and every source coordinate of the frame stay inside 32 bits
    aug = curla_amd.RandomAffine((1024, 1024), 180, (0.25, 1.0), 0.5)
    for th in np.deg2rad([0, 45, 135, 180, -45, -135]):
        for ty, tx in ((512, 512), (-512, -512), (512, -512)):
            m = [int(v) for v in aug.words(th, 0.25, ty, tx)[:, 0]]
            for y, x in ((0, 0), (0, 1023), (1023, 0), (1023, 1023)):
                for a, b, c in (m[:3], m[3:]):
                    assert -2 ** 31 <= a * x + b * y + c < 2 ** 31


def test_evaluation_is_the_identity():
    img = _imgs((5, 7, 3), 1)[0]
    assert curla_amd.RandomAffine((5, 7)).evaluation_augmentation(img) is img


def test_make_augmentor_builds_it():
    a = curla_amd.make_augmentor("affine", HW)
    assert type(a) is curla_amd.RandomAffine
    assert (a.degrees, a.scale, a.translate, a.fill, a.p) == (10.0, (0.9, 1.1), 0.05, "edge", 1.0)
    b = curla_amd.make_augmentor("affine", HW, degrees=25, scale=(0.5, 2), translate=0.2, fill="zero", p=0.25)
    assert (b.degrees, b.scale, b.translate, b.fill, b.p) == (25.0, (0.5, 2.0), 0.2, "zero", 0.25)
    with pytest.raises(TypeError):
        curla_amd.make_augmentor("affine", HW, None, 25)  # the new arguments are keyword-only
    with pytest.raises(ValueError):
        curla_amd.make_augmentor("affine", HW, degrees=-3)
    for unknown in ("Affine", "random_affine", "affine+cutout", "rotate+affine"):
        with pytest.raises(ValueError):
            curla_amd.make_augmentor(unknown, HW)
    assert type(curla_amd.make_augmentor("rotate", HW, p=0.5)) is curla_amd.RandomRotate  # p still means theirs


def test_compose_refuses_it_as_a_mover():
    with pytest.raises(ValueError, match="Compose: move must be a RandomCrop, RandomShift or RandomTranslate"):
        curla_amd.Compose(curla_amd.RandomAffine(HW), curla_amd.RandomCutout(HW))


# ------------------------------------------------------------------------------------------------ draws and words
@pytest.mark.parametrize("kw", [dict(), dict(degrees=0, scale=(1, 1), translate=0), dict(p=0.4), dict(p=0.0)])
def test_five_draws_in_the_stated_order_whatever_the_parameters(kw):
    hw, n = (20, 30), 16
    aug = curla_amd.RandomAffine(hw, **kw)
    np.random.seed(4)
    theta, s, ty, tx, keep = aug.draw_params(n)
    after = np.random.get_state()
    np.random.seed(4)
    deg = np.random.uniform(-aug.degrees, aug.degrees, n)
    s_ = np.random.uniform(aug.scale[0], aug.scale[1], n)
    ty_ = np.random.uniform(-aug.translate * 20, aug.translate * 20, n)
    tx_ = np.random.uniform(-aug.translate * 30, aug.translate * 30, n)
    keep_ = np.random.rand(n) < aug.p
    assert _same_stream(after, np.random.get_state())
    assert np.array_equal(theta, np.deg2rad(deg)) and np.array_equal(s, s_) and np.array_equal(ty, ty_)
    assert np.array_equal(tx, tx_) and np.array_equal(keep, keep_) and keep.dtype == bool
    np.random.seed(4)
    words = aug.draw_index_words(n)
    assert _same_stream(after, np.random.get_state())
    assert len(words) == 6 and all(w.shape == (n,) and w.dtype == np.int32 for w in words)
    m = aug.words(theta, s, ty, tx)
    for k in range(6):
        assert np.array_equal(words[k], np.where(keep, m[k], IDENTITY[k]))
    if aug.p == 0.0 or aug.degrees == 0.0:
        assert all((words[k] == IDENTITY[k]).all() for k in range(6))
    elif aug.p == 1.0:
        assert not any((words[k] == IDENTITY[k]).all() for k in range(6))
    else:
        ident = np.all([words[k] == IDENTITY[k] for k in range(6)], axis=0)
        assert np.array_equal(ident, ~keep) and 0 < ident.sum() < n


def test_words_are_the_formula():
    hw = (20, 30)
    aug = curla_amd.RandomAffine(hw)
    rs = np.random.RandomState(1)
    theta, s = rs.uniform(-np.pi, np.pi, 40), rs.uniform(0.3, 3.0, 40)
    ty, tx = rs.uniform(-10, 10, 40), rs.uniform(-15, 15, 40)
    m = aug.words(theta, s, ty, tx)
    assert m.shape == (6, 40) and m.dtype == np.int32
    for i in range(40):
        a, b = np.cos(theta[i]) / s[i], -np.sin(theta[i]) / s[i]
        cx, cy = (30 - 1) / 2, (20 - 1) / 2
        ux, uy = cx + tx[i], cy + ty[i]
        want = [np.rint(65536 * a), np.rint(65536 * b), np.rint(65536 * (cx - a * ux - b * uy)),
                np.rint(-65536 * b), np.rint(65536 * a), np.rint(65536 * (cy + b * ux - a * uy))]
        assert m[:, i].tolist() == [int(v) for v in want]
        assert m[:, i].tolist() == list(words_of(20, 30, np.rad2deg(theta[i]), s[i], ty[i], tx[i]))
    # the neutral parameters are the identity words exactly, on any frame; scalars are taken as one sample
    for shape in ((8, 8), (5, 7), (84, 84), (90, 160)):
        assert curla_amd.RandomAffine(shape).words(0.0, 1.0, 0.0, 0.0)[:, 0].tolist() == list(IDENTITY)
    sq = curla_amd.RandomAffine((8, 8))
    assert sq.words(np.pi, 1, 0, 0)[:, 0].tolist() == W180
    assert sq.words(np.pi / 2, 1, 0, 0)[:, 0].tolist() == W90
    assert sq.words(-np.pi / 2, 1, 0, 0)[:, 0].tolist() == [0, 65536, 0, -65536, 0, 458752]
    np.random.seed(2)
    ident = curla_amd.RandomAffine((8, 8), 0, (1, 1), 0).draw_index_words(5)
    assert [w.tolist() for w in ident] == [[v] * 5 for v in IDENTITY]


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("fill", ["edge", "zero"])
@pytest.mark.parametrize("geo", GEOMETRIES, ids=["%dx%dx%d" % g for g in GEOMETRIES])
def test_warp_is_the_independent_restatement(geo, fill):
    H, W, Cc = geo
    sets = [w for _, w in kernel_word_sets(H, W)]
    imgs = _imgs(geo, len(sets))
    words = np.array(sets, dtype=np.int64).T
    aug = curla_amd.RandomAffine((H, W), fill=fill)
    got = aug.warp(imgs, words)
    assert got.dtype == np.uint8 and got.shape == imgs.shape
    assert np.array_equal(got, _warp_ref(imgs, words, fill))
    assert np.array_equal(got, aug.warp(imgs, [w.astype(np.int32) for w in words]))  # int32 rows, as the block carries them
    # ... and the vectorised helper is the formula pixel by pixel, in Python integers
    nhwc = np.ascontiguousarray(imgs.transpose(0, 2, 3, 1))
    for s in range(len(sets)):
        for y in range(H):
            for x in range(W):
                assert got[s, :, y, x].tolist() == affine_pixel(nhwc[s], sets[s], fill == "edge", y, x), (s, y, x)
    assert np.array_equal(got[-3], aug.warp(imgs[-3:-2], np.array(GARBAGE, dtype=np.int64).reshape(6, 1))[0])


@pytest.mark.parametrize("geo", GEOMETRIES, ids=["%dx%dx%d" % g for g in GEOMETRIES])
def test_warp_equals_the_exact_maps_it_contains(geo):
    H, W, Cc = geo
    imgs = _imgs(geo, 3, seed=5)
    col = lambda w: np.array(w, dtype=np.int64).reshape(6, 1).repeat(3, axis=1)  # noqa: E731
    for fill in ("edge", "zero"):
        aug = curla_amd.RandomAffine((H, W), fill=fill)
        assert np.array_equal(aug.warp(imgs, col(IDENTITY)), imgs)
        assert np.array_equal(aug.warp(imgs, aug.words(np.pi, 1, 0, 0).repeat(3, axis=1)), imgs[..., ::-1, ::-1])
        if H == W:
            for k, th in ((1, np.pi / 2), (3, -np.pi / 2)):
                assert np.array_equal(aug.warp(imgs, aug.words(th, 1, 0, 0).repeat(3, axis=1)),
                                      np.rot90(imgs, k, axes=(2, 3)))
    # an integer translation is RandomShift's shift (edge) and the same with zeros shifted in (zero)
    pad = 3
    shift = curla_amd.RandomShift((H, W), pad)
    dy, dx = np.array([0, 5, 2]), np.array([6, 1, 3])
    words = curla_amd.RandomAffine((H, W)).words(0.0, 1.0, -(dy - pad), -(dx - pad))
    assert words[2].tolist() == ((dx - pad) * 65536).tolist() and words[5].tolist() == ((dy - pad) * 65536).tolist()
    assert np.array_equal(curla_amd.RandomAffine((H, W)).warp(imgs, words), shift.shift(imgs, dy, dx))
    zero = np.zeros_like(imgs)
    for b in range(3):
        oy, ox = int(dy[b]) - pad, int(dx[b]) - pad
        for y in range(H):
            for x in range(W):
                if 0 <= y + oy < H and 0 <= x + ox < W:
                    zero[b, :, y, x] = imgs[b, :, y + oy, x + ox]
    assert np.array_equal(curla_amd.RandomAffine((H, W), fill="zero").warp(imgs, words), zero)
    assert not np.array_equal(zero, shift.shift(imgs, dy, dx))
    # half a pixel to the right: the rounded mean of neighbours, the last column its own under edge fill
    half = curla_amd.RandomAffine((H, W)).warp(imgs, col((65536, 0, 0x8000, 0, 65536, 0)))
    p = imgs.astype(np.int64)
    nxt = np.concatenate([p[..., 1:], p[..., -1:]], axis=-1)
    assert np.array_equal(half, (p + nxt + 1) >> 1)
    # a constant image stays constant under edge fill, whatever the words; under zero fill it cannot grow
    const = np.full((3, Cc, H, W), 201, dtype=np.uint8)
    rs = np.random.RandomState(8)
    wild = rs.randint(-2 ** 31, 2 ** 31, (6, 3), dtype=np.int64)
    wild[:, 0] = GARBAGE
    assert np.array_equal(curla_amd.RandomAffine((H, W)).warp(const, wild), const)
    assert int(curla_amd.RandomAffine((H, W), fill="zero").warp(const, wild).max()) <= 201
    # the garbage words give a defined result, the same for words that differ by multiples of 2^32
    g = curla_amd.RandomAffine((H, W)).warp(imgs[:1], np.array(GARBAGE, dtype=np.int64).reshape(6, 1))
    g2 = curla_amd.RandomAffine((H, W)).warp(imgs[:1], (np.array(GARBAGE, dtype=np.int64) + 2 ** 32).reshape(6, 1))
    assert g.shape == imgs[:1].shape and g.dtype == np.uint8 and np.array_equal(g, g2)
    assert wrap32(2 ** 31) == -2 ** 31 and wrap32(-2 ** 31 - 1) == 2 ** 31 - 1 and wrap32(-1) == -1


def test_training_augmentation_is_draw_words_warp():
    imgs = _imgs((7, 7, 3), 6, seed=9)
    aug = curla_amd.RandomAffine((7, 7), 30, (0.8, 1.3), 0.1, "zero", 0.5)
    np.random.seed(3)
    out = aug.training_augmentation(imgs)
    after = np.random.get_state()
    np.random.seed(3)
    theta, s, ty, tx, keep = aug.draw_params(6)
    assert _same_stream(after, np.random.get_state())
    words = np.where(keep, aug.words(theta, s, ty, tx), np.array(IDENTITY)[:, None])
    assert np.array_equal(out, aug.warp(imgs, words)) and 0 < keep.sum() < 6
    assert np.array_equal(out[~keep], imgs[~keep]) and not np.array_equal(out[keep], imgs[keep])


# ------------------------------------------------------------------------------------------------ launch schedule
def test_one_launch_behind_the_staging_on_plain_storage():
    rb = _rb(curla_amd.make_augmentor("affine", HW, fill="zero"))
    calls, sample = _traced(rb.sample_cpc_refs)
    assert [n for n, _ in calls] == ["curla_sample_stage", "curla_affine_u8"]
    frames, idx, period, m00, m01, m02, m10, m11, m12, fill, n, c, h, w, out, _ = calls[1][1]
    blk, lay = rb._d_index[rb._sample_slot].data_ptr(), rb.block_layout()
    assert frames == rb._both.data_ptr() and idx == blk and period == 2 * B and n == 3 * B and fill == 0
    assert (m00, m01) == (blk + lay["offs"], blk + lay["offs"] + 12 * B)
    assert [m02, m10, m11, m12] == [blk + lay["cut"] + 12 * B * k for k in range(4)]
    assert (c, h, w) == (C,) + HW and out == rb._shift_store[rb._sample_slot].data_ptr()
    assert rb._scratch_frame() == rb._frame
    obs, _, _, nxt, _, kw = sample
    for ref, row0 in ((obs, 0), (nxt, B), (kw["obs_pos"], 2 * B)):
        assert ref.src.data_ptr() == out and tuple(ref.src.shape) == (3 * B,) + HW + (C,)
        assert ref.is_u8 == 1 and ref.B == B and (ref.Hc, ref.Wc) == (ref.Hs, ref.Ws) == HW
        assert ref.idx.tolist() == list(range(row0, row0 + B)) and not ref.h1.any() and not ref.w1.any()
    calls, tensors = _traced(rb.sample_cpc)
    assert [n for n, _ in calls] == ["curla_sample_stage", "curla_affine_u8"] + ["curla_crop_nchw"] * 3
    assert tuple(tensors[0].shape) == (B, C) + HW == tuple(tensors[5]["obs_pos"].shape)
    assert _traced(_rb(curla_amd.RandomAffine(HW)).sample_cpc_refs)[0][1][1][9] == 1  # edge fill is 1
    # the block: six words per sample and tensor, the last four as runs of 3B behind the offsets
    n0 = 2 * B * 8 + 6 * B * 4
    assert lay["cut"] == n0 and lay["nbytes"] == n0 + 4 * 3 * B * 4
    assert lay == _rb(curla_amd.make_augmentor("random_shift+cutout", HW)).block_layout()
    assert not rb.graph_supported()  # a CPU buffer


def test_the_other_routes_launch_it_where_the_shift_is_launched():
    rb = _rb(curla_amd.RandomAffine(HW), dedup_frames=True)
    calls, _ = _traced(rb.sample_cpc_refs)
    assert [n for n, _ in calls] == ["curla_sample_stage", "curla_gather_stacks", "curla_gather_stacks", "curla_affine_u8"]
    a = calls[-1][1]
    assert a[0] == rb._mb_store[rb._sample_slot].data_ptr() and a[1] is None and a[2] == 2 * B and a[10] == 3 * B
    rb = _rb(curla_amd.RandomAffine(HW), n_step=3, discount=0.99)
    calls, _ = _traced(rb.sample_cpc_refs)
    assert [n for n, _ in calls] == ["curla_sample_stage_nstep", "curla_affine_u8"]


def test_rings_in_two_allocations_take_one_launch_per_tensor():
    hw = (11, 13)
    rb = _rb(curla_amd.RandomAffine(hw), obs_shape=(3,) + hw, cap=7, batch=4, n_add=5)
    assert (7 * 429) % 4 != 0 and rb._both is None
    calls, _ = _traced(rb.sample_cpc_refs)
    assert [n for n, _ in calls] == ["curla_sample_stage"] + ["curla_affine_u8"] * 3
    moves = [a for n, a in calls if n == "curla_affine_u8"]
    out0 = rb._shift_store[rb._sample_slot].data_ptr()
    blk, lay = rb._d_index[rb._sample_slot].data_ptr(), rb.block_layout()
    assert [a[0] for a in moves] == [rb.obses.data_ptr(), rb.next_obses.data_ptr(), rb.obses.data_ptr()]
    assert [a[1] for a in moves] == [blk] * 3 and all(a[2] == 4 and a[10] == 4 for a in moves)
    assert [a[14] for a in moves] == [out0 + j * 4 * 3 * 11 * 13 for j in range(3)]
    for j, a in enumerate(moves):
        assert [a[3], a[4]] == [blk + 64 + 16 * (3 * k + j) for k in range(2)]
        assert list(a[5:9]) == [blk + lay["cut"] + 16 * (3 * k + j) for k in range(4)]
    assert not rb.graph_supported()


def test_the_words_of_a_draw_reach_the_block_rows():
    """draw_indices: the index draw, then per tensor the class's five calls; word r of tensor j in row 6 (r // 2) + 2 j +
    r % 2 of [18, B]."""
    rb = _rb(curla_amd.RandomAffine(HW, p=0.7))
    rb.idx = 12
    np.random.seed(5)
    idxs, offs = rb.draw_indices()
    after = np.random.get_state()
    np.random.seed(5)
    want_idx = np.random.randint(0, 12, size=B)
    per_tensor = [curla_amd.RandomAffine(HW, p=0.7).draw_index_words(B) for _ in range(3)]
    assert _same_stream(after, np.random.get_state()) and np.array_equal(idxs, want_idx)
    assert offs.shape == (18, B) and offs.dtype == np.int32
    for j in range(3):
        for r in range(6):
            assert np.array_equal(offs[6 * (r // 2) + 2 * j + r % 2], per_tensor[j][r]), (j, r)
    assert not np.array_equal(per_tensor[0][2], per_tensor[1][2])


def test_ops_check_shapes_before_any_launch():
    from curla_amd import ops
    ring = torch.zeros((4, 5, 7, 3), dtype=torch.uint8)
    w = [torch.zeros(4, dtype=torch.int32) for _ in range(6)]
    out = torch.zeros((4, 5, 7, 3), dtype=torch.uint8)
    calls = []
    _lib.set_trace_hook(lambda name, args: calls.append((name, args)))
    try:
        ops.affine_u8(ring, None, 4, w, 1, 4, out)
        assert calls[-1][0] == "curla_affine_u8" and tuple(calls[-1][1][9:14]) == (1, 4, 3, 5, 7)
        del calls[:]
        short, wide = torch.zeros(3, dtype=torch.int32), torch.zeros(4, dtype=torch.int64)
        for bad in (dict(out=torch.zeros((4, 7, 5, 3), dtype=torch.uint8)),     # another frame shape
                    dict(out=torch.zeros((3, 5, 7, 3), dtype=torch.uint8)),     # fewer samples than n
                    dict(out=torch.zeros((4, 5, 7, 3), dtype=torch.float32)),   # dtype
                    dict(w=w[:5]), dict(w=w + w[:1]),                           # not six words
                    dict(w=w[:5] + [short]), dict(w=[wide] + w[1:]),            # too few words; dtype
                    dict(fill=2), dict(fill=-1),
                    dict(idx=torch.zeros(3, dtype=torch.int64)),                # too few rows for the period
                    dict(idx=torch.zeros(4, dtype=torch.int32))):
            kw = dict(idx=None, w=w, out=out, fill=0)
            kw.update(bad)
            with pytest.raises(_lib.CurlaHipError):
                ops.affine_u8(ring, kw["idx"], 4, kw["w"], kw["fill"], 4, kw["out"])
        assert calls == []
    finally:
        _lib.set_trace_hook(None)


def test_graph_texts_name_it():
    import inspect
    for text in (inspect.getsource(curla_amd.CurlSacAgent.enable_update_graphs), curla_amd.ReplayBuffer.graph_supported.__doc__,
                 curla_amd.ReplayBuffer.draw_indices.__doc__):
        assert "RandomAffine" in text


# ------------------------------------------------------------------------------------------------ ABI
def test_header_declares_the_entry_point_and_the_abi_number_stays():
    with open(os.path.join(ROOT, "include", "curla_hip.h")) as f:
        header = f.read()
    m = re.search(r"\bint\s+curla_affine_u8\s*\(([^)]*)\)\s*;", header)
    assert m, "include/curla_hip.h does not declare curla_affine_u8"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == len(_lib.SIGNATURES["curla_affine_u8"]) == 16
    assert tuple(p.split()[-1].lstrip("*") for p in params) == (
        "frames", "idx", "period", "m00", "m01", "m02", "m10", "m11", "m12", "fill", "n", "C", "H", "W", "out", "stream")
    for p, t in zip(params, _lib.SIGNATURES["curla_affine_u8"]):
        assert ("*" in p) == (t is _lib.vp), p
        if t is not _lib.vp:
            assert p.startswith("int ") and t is _lib.c_int
    assert re.search(r"#define\s+CURLA_ABI_VERSION\s+8\b", header) and _lib.ABI_VERSION == 8
