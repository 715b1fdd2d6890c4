"""``RandomFlip``, ``RandomRotate`` and ``RandomGrayscale`` (RAD's flip, rotate and grayscale on the uint8 path) without a
GPU: the augmentors' API and validation, the order of their NumPy draws, the host restatements against ``np.rot90``,
slicing and the integer formula, the dihedral codes, ``make_augmentor``, ``Compose`` refusing them as movers, where their
launches sit in the launch schedule (trace hook: nothing is computed) and the C ABI's declarations."""
import os
import re

import numpy as np
import pytest
import torch

import curla_amd
from curla_amd import _lib
from curla_amd.augmentations import FLIP_X, FLIP_Y, ROT90_CODES, TRANSPOSE, dihedral
from tests.test_translate_host import _rb, _traced

C, HW, SQ, B = 9, (34, 40), (36, 36), 8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = {"flip": ("RandomFlip", 0.5), "rotate": ("RandomRotate", 0.3), "grayscale": ("RandomGrayscale", 0.3)}
KERNEL = {"flip": "curla_dihedral_u8", "rotate": "curla_dihedral_u8", "grayscale": "curla_grayscale_u8"}


def _cls(name):
    return getattr(curla_amd, CLASSES[name][0])


def _stream_untouched_since(state):
    now = np.random.get_state()
    return np.array_equal(state[1], now[1]) and state[2] == now[2]


# ------------------------------------------------------------------------------------------------ augmentor API
@pytest.mark.parametrize("name", list(CLASSES))
def test_constructor_defaults_and_refusals(name):
    cls, p = _cls(name), CLASSES[name][1]
    aug = cls(HW)
    assert aug.input_shape == HW == aug.output_shape and aug.p == p and isinstance(aug.p, float)
    assert isinstance(aug, curla_amd.IdentityAugmentation) and not isinstance(aug, (curla_amd.RandomCrop, curla_amd.RandomShift))
    assert cls(list(HW), 1).p == 1.0 and cls([np.int64(34), 40], np.float32(0.25)).p == 0.25 and cls(HW, 0).p == 0.0
    assert cls([np.int64(34), 40]).input_shape == HW
    for bad_in in ((34,), (3, 34, 40), (34.0, 40), (True, 40), ("34", 40)):
        with pytest.raises(ValueError):
            cls(bad_in)
    for bad_p in (True, False, "0.5", None, -0.01, 1.01, float("nan"), [0.5]):
        with pytest.raises(ValueError):
            cls(HW, bad_p)
    assert cls.__name__ in curla_amd.__all__ and getattr(curla_amd.augmentations, cls.__name__) is cls
    img = np.arange(C * 4 * 5, dtype=np.uint8).reshape(C, 4, 5)
    assert aug.evaluation_augmentation(img) is img  # evaluation is the identity


@pytest.mark.parametrize("name", list(CLASSES))
def test_kind_and_words(name):
    aug = _cls(name)(HW)
    assert aug.sample_kind == "scratch" and aug.index_rows == 2 and callable(aug.scratch_launch)
    np.random.seed(3)
    words = aug.draw_index_words(50)
    assert len(words) == 2 and np.asarray(words[0]).shape == (50,) and not np.any(words[1])  # the second word is 0
    allowed = {"flip": {0, 1}, "rotate": {0, 3}, "grayscale": {0, 1}}[name]  # (34, 40) is not square: 0 or 180 degrees
    assert set(np.asarray(words[0]).tolist()) == allowed


def test_make_augmentor_names_and_p():
    for name, (cls_name, default) in CLASSES.items():
        a = curla_amd.make_augmentor(name, HW)
        assert type(a) is getattr(curla_amd, cls_name) and a.p == default and a.output_shape == HW
        assert curla_amd.make_augmentor(name, HW, p=None).p == default
        assert curla_amd.make_augmentor(name, HW, p=0.75).p == 0.75 and curla_amd.make_augmentor(name, HW, p=0).p == 0.0
        with pytest.raises(ValueError):
            curla_amd.make_augmentor(name, HW, p=1.5)
    assert type(curla_amd.make_augmentor("translate", HW, p=0.2)) is curla_amd.RandomTranslate  # p is theirs alone
    for unknown in ("Flip", "random_flip", "rotation", "gray", "greyscale", "flip+cutout", "rotate+cutout_color",
                    "grayscale+cutout"):
        with pytest.raises(ValueError):
            curla_amd.make_augmentor(unknown, HW)


@pytest.mark.parametrize("name", list(CLASSES))
def test_compose_refuses_them_as_movers(name):
    with pytest.raises(ValueError, match="Compose: move must be"):
        curla_amd.Compose(_cls(name)(HW), curla_amd.RandomCutout(HW))
    with pytest.raises(ValueError, match="Compose: paint must be"):
        curla_amd.Compose(curla_amd.RandomShift(HW), _cls(name)(HW))


# ------------------------------------------------------------------------------------------------ draws
@pytest.mark.parametrize("name", ["flip", "grayscale"])
def test_flags_are_one_rand_call(name):
    aug, n = _cls(name)(HW, 0.4), 3000
    np.random.seed(21)
    flags = aug.draw_flags(n)
    after = np.random.get_state()
    np.random.seed(21)
    want = np.random.rand(n) < 0.4
    assert _stream_untouched_since(after) and flags.dtype == bool and np.array_equal(flags, want)
    assert 0.3 < flags.mean() < 0.5
    np.random.seed(21)
    word0, word1 = aug.draw_index_words(n)
    assert _stream_untouched_since(after) and np.array_equal(word0, want.astype(np.int32)) and not np.any(word1)
    for p, all_set in ((0.0, False), (1.0, True)):  # the call is made whatever p is
        np.random.seed(21)
        f = _cls(name)(HW, p).draw_flags(n)
        assert _stream_untouched_since(after) and f.all() == all_set and f.any() == all_set


@pytest.mark.parametrize("hw", [SQ, HW], ids=["square", "not_square"])
def test_rotate_draws_turns_then_keep_whatever_p_is(hw):
    n = 4000
    for p in (0.3, 0.0, 1.0):
        aug = curla_amd.RandomRotate(hw, p)
        np.random.seed(9)
        k = aug.draw_turns(n)
        after = np.random.get_state()
        np.random.seed(9)
        turns = np.random.randint(0, 4, n) if hw[0] == hw[1] else 2 * np.random.randint(0, 2, n)
        keep = np.random.rand(n) < p
        assert _stream_untouched_since(after)
        assert np.array_equal(k, np.where(keep, turns, 0))
        if p == 1.0:
            assert sorted(set(k.tolist())) == ([0, 1, 2, 3] if hw[0] == hw[1] else [0, 2])
        if p == 0.0:
            assert not k.any()
        np.random.seed(9)
        word0, word1 = aug.draw_index_words(n)
        assert _stream_untouched_since(after) and not np.any(word1)
        assert np.array_equal(word0, np.array([0, 5, 3, 6])[k]) and word0.dtype == np.int32


# ------------------------------------------------------------------------------------------------ host restatements
def test_the_dihedral_codes_are_the_numpy_operations():
    """The table of the codes: 1 = [:, ::-1], 2 = [::-1], 4 = .T, 5 / 3 / 6 = np.rot90 with k = 1 / 2 / 3 over (H, W);
    and the formula of curla_dihedral_u8 pixel by pixel."""
    assert (FLIP_X, FLIP_Y, TRANSPOSE) == (1, 2, 4) and ROT90_CODES == (0, 5, 3, 6)
    img = np.random.RandomState(1).randint(0, 256, (1, 6, 5, 5), dtype=np.uint8)
    plane = lambda code: dihedral(img, [code])[0]  # noqa: E731
    assert np.array_equal(plane(0), img[0])
    assert np.array_equal(plane(1), img[0][:, :, ::-1]) and np.array_equal(plane(2), img[0][:, ::-1])
    assert np.array_equal(plane(4), img[0].transpose(0, 2, 1))
    for k, code in enumerate(ROT90_CODES):
        assert np.array_equal(plane(code), np.rot90(img[0], k, axes=(1, 2))), k
    H = W = 5
    for code in range(8):
        got = plane(code)
        for y in range(H):
            for x in range(W):
                a, b = (x, y) if code & 4 else (y, x)
                assert np.array_equal(got[:, y, x], img[0][:, H - 1 - a if code & 2 else a, W - 1 - b if code & 1 else b])
    wide = np.random.RandomState(2).randint(0, 256, (4, 3, 4, 7), dtype=np.uint8)  # not square: codes 0..3
    got = dihedral(wide, [0, 1, 2, 3])
    assert np.array_equal(got[1], wide[1][:, :, ::-1]) and np.array_equal(got[3], np.rot90(wide[3], 2, axes=(1, 2)))


def test_flip_and_rotate_restatements():
    imgs = np.random.RandomState(3).randint(0, 256, (5, 6, 7, 7), dtype=np.uint8)
    untouched = imgs.copy()
    flags = np.array([True, False, True, False, False])
    got = curla_amd.RandomFlip.flip(imgs, flags)
    assert got.dtype == np.uint8 and got.shape == imgs.shape
    for b in range(5):
        assert np.array_equal(got[b], imgs[b][:, :, ::-1] if flags[b] else imgs[b])
    assert np.array_equal(curla_amd.RandomFlip.flip(got, flags), imgs)  # an involution
    assert np.array_equal(got, dihedral(imgs, flags.astype(int)))
    k = np.array([0, 1, 2, 3, 1])
    rot = curla_amd.RandomRotate.rotate(imgs, k)
    for b in range(5):
        assert np.array_equal(rot[b], np.rot90(imgs[b], k[b], axes=(1, 2)))
    assert np.array_equal(curla_amd.RandomRotate.rotate(rot, (4 - k) % 4), imgs)
    wide = np.random.RandomState(4).randint(0, 256, (2, 3, 4, 9), dtype=np.uint8)
    assert np.array_equal(curla_amd.RandomRotate.rotate(wide, [2, 0]), np.stack([wide[0][:, ::-1, ::-1], wide[1]]))
    assert np.array_equal(imgs, untouched)
    # training_augmentation: the draw, then the restatement
    for aug, fn in ((curla_amd.RandomFlip((7, 7)), lambda a: a.flip(imgs, np.random.rand(5) < 0.5)),
                    (curla_amd.RandomRotate((7, 7), 0.9),
                     lambda a: a.rotate(imgs, (lambda t, keep: np.where(keep, t, 0))(np.random.randint(0, 4, 5),
                                                                                      np.random.rand(5) < 0.9)))):
        np.random.seed(31)
        out = aug.training_augmentation(imgs)
        np.random.seed(31)
        assert np.array_equal(out, fn(aug))


def test_grey_is_the_integer_formula_idempotent_and_keeps_grey_pixels():
    rs = np.random.RandomState(5)
    imgs = rs.randint(0, 256, (4, 6, 5, 7), dtype=np.uint8)
    imgs[0, :, 0, 0] = 255
    imgs[0, :, 0, 1] = 0
    flags = np.array([1, 0, 2, -1])  # any non-zero flag counts
    got = curla_amd.RandomGrayscale.grey(imgs, flags)
    assert got.dtype == np.uint8 and got.shape == imgs.shape and np.array_equal(got[1], imgs[1])
    for b in (0, 2, 3):
        for f in range(2):
            r, g, bl = (imgs[b, 3 * f + j].astype(np.int64) for j in range(3))
            want = (77 * r + 150 * g + 29 * bl + 128) >> 8
            assert want.min() >= 0 and want.max() <= 255
            for j in range(3):
                assert np.array_equal(got[b, 3 * f + j], want)
    assert got[0, 0, 0, 0] == 255 and got[0, 0, 0, 1] == 0
    assert np.array_equal(curla_amd.RandomGrayscale.grey(got, flags), got)  # idempotent
    v = np.arange(256, dtype=np.uint8)
    grey_in = np.broadcast_to(v[None, None, None, :], (1, 3, 1, 256)).copy()  # every (v, v, v)
    assert np.array_equal(curla_amd.RandomGrayscale.grey(grey_in, [1]), grey_in)
    # within 1 of RAD's float mix
    trip = rs.randint(0, 256, (1, 3, 100, 100), dtype=np.uint8)
    rad = 0.2989 * trip[0, 0] + 0.587 * trip[0, 1] + 0.114 * trip[0, 2]
    assert np.abs(curla_amd.RandomGrayscale.grey(trip, [1])[0, 0] - rad).max() < 1.0
    with pytest.raises(ValueError):
        curla_amd.RandomGrayscale.grey(np.zeros((1, 4, 2, 2), np.uint8), [1])
    np.random.seed(6)
    out = curla_amd.RandomGrayscale((5, 7), 0.5).training_augmentation(imgs)
    np.random.seed(6)
    assert np.array_equal(out, curla_amd.RandomGrayscale.grey(imgs, np.random.rand(4) < 0.5))


# ------------------------------------------------------------------------------------------------ launch schedule
@pytest.mark.parametrize("name", list(CLASSES))
def test_one_launch_behind_the_staging_on_plain_storage(name):
    rb = _rb(curla_amd.make_augmentor(name, HW))
    calls, sample = _traced(rb.sample_cpc_refs)
    assert [n for n, _ in calls] == ["curla_sample_stage", KERNEL[name]]
    frames, idx, period, word0, n, c, h, w, out, _ = calls[1][1]
    blk = rb._d_index[rb._sample_slot]
    assert frames == rb._both.data_ptr() and idx == blk.data_ptr() and period == 2 * B and n == 3 * B
    assert word0 == blk.data_ptr() + 16 * B and (c, h, w) == (C,) + HW
    assert out == rb._shift_store[rb._sample_slot].data_ptr() and rb._scratch_frame() == rb._frame
    obs, _, _, nxt, _, kw = sample
    for ref, row0 in ((obs, 0), (nxt, B), (kw["obs_pos"], 2 * B)):
        assert ref.src.data_ptr() == out and tuple(ref.src.shape) == (3 * B,) + HW + (C,)
        assert ref.is_u8 == 1 and ref.B == B and (ref.Hc, ref.Wc) == (ref.Hs, ref.Ws) == HW
        assert ref.idx.tolist() == list(range(row0, row0 + B)) and not ref.h1.any() and not ref.w1.any()
    calls, tensors = _traced(rb.sample_cpc)
    assert [n for n, _ in calls] == ["curla_sample_stage", KERNEL[name]] + ["curla_crop_nchw"] * 3
    assert tuple(tensors[0].shape) == (B, C) + HW == tuple(tensors[5]["obs_pos"].shape)
    assert rb.block_layout() == _rb(curla_amd.RandomShift(HW)).block_layout() and "cut" not in rb.block_layout()


@pytest.mark.parametrize("name", list(CLASSES))
def test_the_other_routes_launch_it_where_the_shift_is_launched(name):
    rb = _rb(curla_amd.make_augmentor(name, HW), dedup_frames=True)
    calls, _ = _traced(rb.sample_cpc_refs)
    assert [n for n, _ in calls] == ["curla_sample_stage", "curla_gather_stacks", "curla_gather_stacks", KERNEL[name]]
    a = calls[-1][1]
    assert a[0] == rb._mb_store[rb._sample_slot].data_ptr() and a[1] is None and a[2] == 2 * B and a[4] == 3 * B
    rb = _rb(curla_amd.make_augmentor(name, HW), n_step=3, discount=0.99)
    calls, _ = _traced(rb.sample_cpc_refs)
    assert [n for n, _ in calls] == ["curla_sample_stage_nstep", KERNEL[name]]


@pytest.mark.parametrize("name", list(CLASSES))
def test_rings_in_two_allocations_take_one_launch_per_tensor(name):
    hw = (11, 13)
    rb = _rb(curla_amd.make_augmentor(name, hw), obs_shape=(3,) + hw, cap=7, batch=4, n_add=5)
    assert (7 * 429) % 4 != 0 and rb._both is None
    calls, _ = _traced(rb.sample_cpc_refs)
    assert [n for n, _ in calls] == ["curla_sample_stage"] + [KERNEL[name]] * 3
    moves = [a for n, a in calls if n == KERNEL[name]]
    out0, blk = rb._shift_store[rb._sample_slot].data_ptr(), rb._d_index[rb._sample_slot].data_ptr()
    assert [a[0] for a in moves] == [rb.obses.data_ptr(), rb.next_obses.data_ptr(), rb.obses.data_ptr()]
    assert [a[1] for a in moves] == [blk, blk, blk] and all(a[2] == 4 and a[4] == 4 for a in moves)
    assert [a[8] for a in moves] == [out0 + j * 4 * 3 * 11 * 13 for j in range(3)]
    assert [a[3] for a in moves] == [blk + 16 * 4 + 4 * 4 * j for j in range(3)]
    assert not rb.graph_supported()


def test_the_words_of_a_draw_reach_the_block_rows():
    """draw_indices: the index draw, then per tensor the class's own calls in its stated order; word 1 stays zero."""
    rb = _rb(curla_amd.RandomRotate(SQ, 0.5), obs_shape=(C,) + SQ)
    rb.idx = 12
    np.random.seed(5)
    idxs, offs = rb.draw_indices()
    after = np.random.get_state()
    np.random.seed(5)
    want_idx = np.random.randint(0, 12, size=B)
    codes = []
    for _ in range(3):
        turns = np.random.randint(0, 4, B)
        keep = np.random.rand(B) < 0.5
        codes.append(np.array([0, 5, 3, 6])[np.where(keep, turns, 0)])
    assert _stream_untouched_since(after) and np.array_equal(idxs, want_idx)
    assert offs.shape == (6, B) and offs.dtype == np.int32
    for j in range(3):
        assert np.array_equal(offs[2 * j], codes[j]) and not offs[2 * j + 1].any()
    assert offs.any()


def test_ops_check_shapes_before_any_launch():
    from curla_amd import ops
    ring = torch.zeros((4, 5, 7, 3), dtype=torch.uint8)
    w = torch.zeros(4, dtype=torch.int32)
    out = torch.zeros((4, 5, 7, 3), dtype=torch.uint8)
    calls = []
    _lib.set_trace_hook(lambda name, args: calls.append((name, args)))
    try:
        for fn, kernel in ((ops.dihedral_u8, "curla_dihedral_u8"), (ops.grayscale_u8, "curla_grayscale_u8")):
            fn(ring, None, 4, w, 4, out)
            assert calls[-1][0] == kernel and tuple(calls[-1][1][4:8]) == (4, 3, 5, 7)
            del calls[:]
            for bad in (dict(out=torch.zeros((4, 7, 5, 3), dtype=torch.uint8)),     # another frame shape
                        dict(out=torch.zeros((3, 5, 7, 3), dtype=torch.uint8)),     # fewer samples than n
                        dict(out=torch.zeros((4, 5, 7, 3), dtype=torch.float32)),   # dtype
                        dict(w=torch.zeros(3, dtype=torch.int32)),                  # too few words
                        dict(w=torch.zeros(4, dtype=torch.int64)),                  # dtype
                        dict(idx=torch.zeros(3, dtype=torch.int64)),                # too few rows for the period
                        dict(idx=torch.zeros(4, dtype=torch.int32))):
                kw = dict(idx=None, w=w, out=out)
                kw.update(bad)
                with pytest.raises(_lib.CurlaHipError):
                    fn(ring, kw["idx"], 4, kw["w"], 4, kw["out"])
            assert calls == []
        ring4, out4 = torch.zeros((4, 5, 7, 4), dtype=torch.uint8), torch.zeros((4, 5, 7, 4), dtype=torch.uint8)
        ops.dihedral_u8(ring4, None, 4, w, 4, out4)  # any C moves ...
        assert len(calls) == 1
        with pytest.raises(_lib.CurlaHipError):      # ... but only RGB triplets are greyed
            ops.grayscale_u8(ring4, None, 4, w, 4, out4)
        assert len(calls) == 1
    finally:
        _lib.set_trace_hook(None)


def test_graph_texts_name_the_three():
    import inspect
    for text in (inspect.getsource(curla_amd.CurlSacAgent.enable_update_graphs), curla_amd.ReplayBuffer.graph_supported.__doc__):
        assert all(n in text for n in ("RandomFlip", "RandomRotate", "RandomGrayscale"))


# ------------------------------------------------------------------------------------------------ ABI
@pytest.mark.parametrize("entry,word", [("curla_dihedral_u8", "code"), ("curla_grayscale_u8", "grey")])
def test_header_declares_the_entry_points_and_the_abi_number_stays(entry, word):
    with open(os.path.join(ROOT, "include", "curla_hip.h")) as f:
        header = f.read()
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % entry, header)
    assert m, "include/curla_hip.h does not declare " + entry
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == len(_lib.SIGNATURES[entry]) == 10
    assert tuple(p.split()[-1].lstrip("*") for p in params) == ("frames", "idx", "period", word, "n", "C", "H", "W", "out", "stream")
    for p, t in zip(params, _lib.SIGNATURES[entry]):
        assert ("*" in p) == (t is _lib.vp), p
        if t is not _lib.vp:
            assert p.startswith("int ") and t is _lib.c_int
    assert re.search(r"#define\s+CURLA_ABI_VERSION\s+8\b", header) and _lib.ABI_VERSION == 8
