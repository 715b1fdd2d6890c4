"""``RandomShift`` (pad by replicated edge pixels, cut a window of the original size at a random offset) without a GPU:
the augmentor's API, the order of its NumPy draws, the host-side augmentation against ``np.pad(mode='edge')``, where the
shift launch sits in an update's launch schedule (trace hook: nothing is computed) and the C ABI's declaration."""
import os
import re

import numpy as np
import pytest
import torch

import curla_amd
from curla_amd import _lib
from curla_amd.utils import ReplayBuffer
from tests.test_host_logic import HP, NullLogger

C, HW, B, CAP = 9, (34, 40), 8, 32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def edge_pad_shift(img, dy, dx, pad):
    """The restatement: (C, H, W) image -> np.pad(HWC, mode='edge')[dy:dy + H, dx:dx + W], back as (C, H, W)."""
    hwc = img.transpose(1, 2, 0)
    h, w = hwc.shape[:2]
    return np.pad(hwc, ((pad, pad), (pad, pad), (0, 0)), mode="edge")[dy:dy + h, dx:dx + w].transpose(2, 0, 1)


# ------------------------------------------------------------------------------------------------ augmentor API
def test_augmentor_api():
    aug = curla_amd.RandomShift(HW)
    assert aug.pad == 4 and aug.input_shape == HW and aug.output_shape == HW
    assert isinstance(aug, curla_amd.IdentityAugmentation) and not isinstance(aug, curla_amd.RandomCrop)
    img = np.random.RandomState(0).randint(0, 256, (C,) + HW, dtype=np.uint8)
    assert aug.evaluation_augmentation(img) is img
    assert curla_amd.RandomShift(HW, pad=0).pad == 0
    for bad in (-1, 2.0, 1.5, "4", None, True):
        with pytest.raises(ValueError):
            curla_amd.RandomShift(HW, pad=bad)
    with pytest.raises(ValueError):
        curla_amd.make_augmentor("random_shift", HW, pad=-3)


@pytest.mark.parametrize("how", ["package", "submodule", "dropin"])
def test_make_augmentor_builds_it_and_the_four_existing_names_build_what_they_built(how):
    if how == "package":
        make = curla_amd.make_augmentor
    elif how == "submodule":
        from curla_amd.augmentations import make_augmentor as make
    else:
        import importlib

        import curla_amd.dropin as dropin
        dropin.install()
        try:
            make = importlib.import_module("augmentations").make_augmentor
            assert importlib.import_module("augmentations").RandomShift is curla_amd.RandomShift
        finally:
            dropin.uninstall()
    a = make("random_shift", HW)
    b = make("random_shift", HW, pad=2)
    assert type(a) is curla_amd.RandomShift and a.pad == 4 and type(b) is curla_amd.RandomShift and b.pad == 2
    with pytest.raises(TypeError):
        make("random_shift", HW, None, 2)  # keyword-only
    for name, cls, out in (("identity", curla_amd.IdentityAugmentation, HW), ("random_crop", curla_amd.RandomCrop, (29, 34)),
                           ("color_jiggle", curla_amd.ColorJiggle, HW), ("noisy_cover", curla_amd.NoisyCover, HW)):
        aug = make(name, HW)
        assert type(aug) is cls and tuple(aug.output_shape) == out
    assert tuple(make("random_crop", HW, (28, 30)).output_shape) == (28, 30)  # positional output_shape as before
    with pytest.raises(ValueError):
        make("random_shif", HW)


# ------------------------------------------------------------------------------------------------ draws
@pytest.mark.parametrize("pad", [0, 1, 4])
def test_draw_offsets_are_two_randint_calls_in_order_and_cover_the_range(pad):
    aug = curla_amd.RandomShift(HW, pad=pad)
    n = 4000
    np.random.seed(17)
    dy, dx = aug.draw_offsets(n)
    after = np.random.get_state()
    np.random.seed(17)
    want_dy = np.random.randint(0, 2 * pad + 1, n)
    want_dx = np.random.randint(0, 2 * pad + 1, n)
    assert np.array_equal(dy, want_dy) and np.array_equal(dx, want_dx)
    now = np.random.get_state()
    assert np.array_equal(after[1], now[1]) and after[2] == now[2]  # nothing else was drawn
    full = list(range(2 * pad + 1))
    assert sorted(set(dy.tolist())) == full and sorted(set(dx.tolist())) == full


def test_draw_indices_is_one_index_draw_then_three_pairs():
    pad = 3
    rb = ReplayBuffer((C,) + HW, (2,), 64, B, "cpu", curla_amd.RandomShift(HW, pad=pad))
    rb.idx = 40
    np.random.seed(5)
    idxs, offs = rb.draw_indices()
    np.random.seed(5)
    want = [np.random.randint(0, 40, size=B)] + [np.random.randint(0, 2 * pad + 1, B) for _ in range(6)]
    assert np.array_equal(idxs, want[0])
    assert offs.shape == (6, B) and offs.dtype == np.int32
    for j in range(6):  # dy, dx of obs; dy, dx of next_obs; dy, dx of pos
        assert np.array_equal(offs[j], want[1 + j]), j
    assert offs.max() <= 2 * pad and offs.min() >= 0 and offs.any()
    # a full buffer draws over the capacity; an object that is none of the known classes is still refused
    rb.full = True
    np.random.seed(6)
    idxs, _ = rb.draw_indices()
    np.random.seed(6)
    assert np.array_equal(idxs, np.random.randint(0, 64, size=B))

    class Other(curla_amd.IdentityAugmentation):
        pass
    other = ReplayBuffer((C,) + HW, (2,), 64, B, "cpu", Other(HW))
    other.idx = 40
    with pytest.raises(NotImplementedError):
        other.draw_indices()


def test_index_block_carries_the_offsets_as_runs_of_3B():
    """The block layout is RandomCrop's: behind idx [2B] int64 the dy rows of obs, next_obs, pos are ONE int32 run of
    3B, the dx rows the next -- what one shift launch of 3B samples reads."""
    rb = ReplayBuffer((C,) + HW, (2,), CAP, B, "cpu", curla_amd.RandomShift(HW, pad=2))
    assert rb.block_layout() == ReplayBuffer((C,) + HW, (2,), CAP, B, "cpu", curla_amd.RandomCrop(HW, (28, 34))).block_layout()
    idxs = np.arange(B)[::-1].copy()
    offs = np.arange(6 * B, dtype=np.int32).reshape(6, B)
    host = torch.zeros(rb.block_layout()["nbytes"], dtype=torch.uint8)
    rb._fill_index_block(host, idxs, offs)
    raw = host.numpy()
    assert raw[:16 * B].view(np.int64).tolist() == idxs.tolist() + (idxs + CAP).tolist()
    o32 = raw[16 * B:].view(np.int32)
    assert o32[:3 * B].tolist() == np.concatenate([offs[0], offs[2], offs[4]]).tolist()
    assert o32[3 * B:].tolist() == np.concatenate([offs[1], offs[3], offs[5]]).tolist()


# ------------------------------------------------------------------------------------------------ host augmentation
@pytest.mark.parametrize("pad", [0, 3, 13])
def test_training_augmentation_is_the_edge_pad_restatement(pad):
    h, w = 9, 11  # (pad = 13 is larger than both sides)
    aug = curla_amd.RandomShift((h, w), pad=pad)
    imgs = np.random.RandomState(pad).randint(0, 256, (40, 6, h, w), dtype=np.uint8)
    np.random.seed(23)
    out = aug.training_augmentation(imgs)
    np.random.seed(23)
    dy = np.random.randint(0, 2 * pad + 1, 40)
    dx = np.random.randint(0, 2 * pad + 1, 40)
    assert out.shape == imgs.shape and out.dtype == imgs.dtype
    for b in range(40):
        assert np.array_equal(out[b], edge_pad_shift(imgs[b], dy[b], dx[b], pad)), b
    if pad == 0:
        assert np.array_equal(out, imgs)
    else:
        assert not np.array_equal(out, imgs)
    # the formula of the issue, element by element, on one sample
    b = 7
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    want = imgs[b][:, np.clip(y + dy[b] - pad, 0, h - 1), np.clip(x + dx[b] - pad, 0, w - 1)]
    assert np.array_equal(out[b], want)


# ------------------------------------------------------------------------------------------------ launch schedule
def _rb(aug, **kw):
    rb = ReplayBuffer((C,) + HW, (2,), CAP, B, "cpu", aug, **kw)
    rs = np.random.RandomState(3)
    for _ in range(12):
        f = rs.randint(0, 256, (C,) + HW, dtype=np.uint8)
        rb.add(f, [0.1, -0.2], 0.5, f, False)
    # a CPU buffer has no pinned index slots; stand in for their device addresses so that sampling takes the route
    # of a device buffer (staging kernel) under the trace hook, which computes nothing
    rb._h_index_dev = [4096 * (k + 1) for k in range(rb._n_slots)]
    return rb


def _agent(aug):
    curla_amd.set_seed_everywhere(1)
    return curla_amd.CurlSacAgent((C,) + tuple(aug.output_shape), (2,), "cpu", aug, hidden_dim=64, **HP)


def _traced_update(aug, **kw):
    agent, rb = _agent(aug), _rb(aug, **kw)
    calls = []
    _lib.set_trace_hook(lambda name, args: calls.append((name, args)))
    try:
        agent.update(rb, NullLogger(), 0)
    finally:
        _lib.set_trace_hook(None)
    return calls, rb


def test_one_shift_launch_behind_the_staging_on_plain_storage():
    calls, rb = _traced_update(curla_amd.RandomShift(HW, pad=3))
    names = [n for n, _ in calls]
    assert names.count("curla_random_shift_u8") == 1 and names.count("curla_sample_stage") == 1
    at = names.index("curla_random_shift_u8")
    assert names[at - 1] == "curla_sample_stage" and names[:at].count("curla_sample_stage") == 1
    assert not any(n.startswith("curla_conv") for n in names[:at])  # in front of everything that reads pixels
    frames, idx, period, dy, dx, pad, n, c, h, w, out, _ = calls[at][1]
    blk = rb._d_index[rb._sample_slot]
    assert frames == rb._both.data_ptr() and idx == blk.data_ptr() and period == 2 * B
    assert dy == blk.data_ptr() + 16 * B and dx == dy + 4 * 3 * B
    assert (pad, n, c, h, w) == (3, 3 * B, C) + HW
    assert out == rb._shift_store[rb._sample_slot].data_ptr()
    # downstream the update reads the scratch as an ordinary uint8 ring: rows 0..3B-1, zero offsets
    first = [a for nm, a in calls if nm == "curla_conv1_fwd2"]
    assert first and all(a[0] == out for a in first)
    assert first[0][1] == rb._shift_rows.data_ptr() and first[0][2] == rb._shift_zero.data_ptr() == first[0][3]
    assert first[0][7] == 2 * B  # (obs | next_obs) as one minibatch of 2B
    assert rb._shift_rows.tolist() == list(range(3 * B)) and not rb._shift_zero.any()
    assert rb._shift_store.shape[0] == rb.N_SAMPLE_SLOTS and rb._shift_store.shape[1] >= 3 * B * C * HW[0] * HW[1] + 32
    # the next sample goes to the other slot's scratch
    _lib.set_trace_hook(lambda name, args: calls.append((name, args)))
    try:
        del calls[:]
        rb.sample_cpc_refs()
    finally:
        _lib.set_trace_hook(None)
    (again,) = [a for nm, a in calls if nm == "curla_random_shift_u8"]
    assert again[10] == rb._shift_store[rb._sample_slot].data_ptr() != out


def test_on_the_frame_store_the_shift_comes_behind_the_two_gathers():
    calls, rb = _traced_update(curla_amd.RandomShift(HW, pad=3), dedup_frames=True)
    names = [n for n, _ in calls]
    assert names.count("curla_random_shift_u8") == 1 and names.count("curla_gather_stacks") == 2
    at = names.index("curla_random_shift_u8")
    assert names[at - 3:at] == ["curla_sample_stage", "curla_gather_stacks", "curla_gather_stacks"]
    a = calls[at][1]
    assert a[0] == rb._mb_store[rb._sample_slot].data_ptr() and a[1] is None and a[2] == 2 * B and a[6] == 3 * B


def test_rings_in_two_allocations_take_one_launch_per_tensor():
    hw = (11, 13)
    aug = curla_amd.RandomShift(hw, pad=2)
    rb = ReplayBuffer((3,) + hw, (2,), 7, 4, "cpu", aug)   # 7 * 429 bytes: the second ring would not start on a dword
    assert rb._both is None
    f = np.zeros((3,) + hw, np.uint8)
    for _ in range(5):
        rb.add(f, [0, 0], 0.0, f, False)
    calls = []
    _lib.set_trace_hook(lambda name, args: calls.append((name, args)))
    try:
        rb.sample_cpc_refs()
    finally:
        _lib.set_trace_hook(None)
    shifts = [a for n, a in calls if n == "curla_random_shift_u8"]
    assert len(shifts) == 3
    out0 = rb._shift_store[rb._sample_slot].data_ptr()
    assert [a[0] for a in shifts] == [rb.obses.data_ptr(), rb.next_obses.data_ptr(), rb.obses.data_ptr()]
    assert [a[10] for a in shifts] == [out0 + j * 4 * 429 for j in range(3)]
    assert all(a[2] == 4 and a[6] == 4 for a in shifts)
    assert not rb.graph_supported()


@pytest.mark.parametrize("name", ["random_crop", "identity"])
def test_the_other_uint8_buffers_launch_no_shift_and_own_no_scratch(name):
    aug = curla_amd.make_augmentor(name, HW, (28, 34) if name == "random_crop" else None)
    calls, rb = _traced_update(aug)
    assert "curla_sample_stage" in [n for n, _ in calls]
    assert not [n for n, _ in calls if n == "curla_random_shift_u8"]
    assert not hasattr(rb, "_shift_store")


def test_graph_slot_records_the_shift_behind_staging_and_gathers():
    """graph_block / graph_refs on the trace hook: the slot owns a guarded 3B-frame buffer, graph_refs launches the
    staging kernel, (frame store) the two gathers and ONE shift that reads its offsets from the slot's device block,
    without a host draw, and hands out ring handles into that buffer."""
    for dedup in (False, True):
        rb = _rb(curla_amd.RandomShift(HW, pad=4), dedup_frames=dedup)
        frame = C * HW[0] * HW[1]
        _lib.set_trace_hook(lambda name, args: None)
        try:
            g = rb.graph_block(0)
        finally:
            _lib.set_trace_hook(None)
        assert g["shift_u8"].numel() == 3 * B * frame + 32 and not g["shift_u8"].any()
        assert len(g["guards"]) == (4 if dedup else 2)
        assert all(bool((x == rb.GUARD_BYTE).all()) and x.numel() >= rb.GUARD for x in g["guards"])
        before = np.random.get_state()
        calls = []
        _lib.set_trace_hook(lambda name, args: calls.append((name, args)))
        try:
            obs, _, _, nxt, _, kw = rb.graph_refs(0)
        finally:
            _lib.set_trace_hook(None)
        now = np.random.get_state()
        assert np.array_equal(before[1], now[1]) and before[2] == now[2]
        names = [n for n, _ in calls]
        assert names == ["curla_sample_stage"] + ["curla_gather_stacks"] * (2 if dedup else 0) + ["curla_random_shift_u8"]
        a = calls[-1][1]
        dev = g["dev"].data_ptr()
        assert a[3] == dev + 16 * B and a[4] == dev + 16 * B + 12 * B and (a[2], a[5], a[6]) == (2 * B, 4, 3 * B)
        assert a[10] == g["shift_u8"].data_ptr()
        assert (a[0], a[1]) == ((g["mb_u8"].data_ptr(), None) if dedup else (rb._both.data_ptr(), dev))
        for ref, row0 in ((obs, 0), (nxt, B), (kw["obs_pos"], 2 * B)):
            assert ref.src.data_ptr() == g["shift_u8"].data_ptr() and ref.is_u8 == 1 and ref.guard is None
            assert ref.idx.tolist() == list(range(row0, row0 + B)) and not ref.h1.any() and not ref.w1.any()
        assert obs.pair[0].B == 2 * B and obs.pair[0].idx.tolist() == list(range(2 * B)) and obs.pair[1] is nxt


# ------------------------------------------------------------------------------------------------ ABI
def test_header_declares_the_entry_point_and_the_abi_number_stays():
    with open(os.path.join(ROOT, "include", "curla_hip.h")) as f:
        header = f.read()
    m = re.search(r"\bint\s+curla_random_shift_u8\s*\(([^)]*)\)\s*;", header)
    assert m, "include/curla_hip.h does not declare curla_random_shift_u8"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == len(_lib.SIGNATURES["curla_random_shift_u8"]) == 12
    want = ("frames", "idx", "period", "dy", "dx", "pad", "n", "C", "H", "W", "out", "stream")
    assert tuple(p.split()[-1].lstrip("*") for p in params) == want
    for p, t in zip(params, _lib.SIGNATURES["curla_random_shift_u8"]):
        assert ("*" in p) == (t is _lib.vp), p
    assert re.search(r"#define\s+CURLA_ABI_VERSION\s+8\b", header) and _lib.ABI_VERSION == 8
    assert "beyond the reference" in header
