"""``RandomConv`` (the random 3x3, 3 -> 3 channel convolution of RAD / "Network Randomization") without a GPU: the NumPy
statement of the formula against hand-computed values, the order and number of the host's draws, validation, and -- on
the launch-trace hook, where nothing is computed -- the ``staged_aug=True`` block layout and what a sample launches."""
import math

import numpy as np
import pytest
import torch

import curla_amd
from curla_amd import _lib
from curla_amd.augmentations import RandomConv
from curla_amd.utils import ReplayBuffer

C, HW, CAP = 9, (12, 10), 32
SCALE = math.sqrt(2 / 54)


@pytest.fixture
def trace():
    calls = []
    _lib.set_trace_hook(lambda name, args: calls.append((name, args)))
    yield calls
    _lib.set_trace_hook(None)


def _one_hot(co, ci, ky, kx):
    w = np.zeros((3, 3, 3, 3), dtype=np.float32)
    w[co, ci, ky, kx] = 1.0
    return w


def _identity():
    return sum(_one_hot(c, c, 1, 1) for c in range(3))


def _moved(plane, dy, dx):
    """out[y][x] = plane[y + dy][x + dx], zeros shifted in."""
    h, w = plane.shape
    out = np.zeros_like(plane)
    for y in range(h):
        for x in range(w):
            if 0 <= y + dy < h and 0 <= x + dx < w:
                out[y, x] = plane[y + dy, x + dx]
    return out


# ------------------------------------------------------------------------------------------------ 1. conv
def test_conv_on_a_1x1_frame_only_the_centre_taps_count():
    x = np.array([[[[2.0]], [[3.0]], [[5.0]], [[7.0]], [[11.0]], [[13.0]]]])  # (1, 6, 1, 1): two frames
    w = np.arange(81, dtype=np.float64).reshape(1, 3, 3, 3, 3) + 1.0
    got = RandomConv.conv(x, w)
    assert got.shape == (1, 6, 1, 1) and got.dtype == np.float64
    centre = w[0, :, :, 1, 1]  # [co][ci]
    for f, rgb in enumerate(([2.0, 3.0, 5.0], [7.0, 11.0, 13.0])):
        for co in range(3):
            assert got[0, 3 * f + co, 0, 0] == sum(centre[co, ci] * rgb[ci] for ci in range(3))
    # by hand: w[0][ci][1][1] is entry 9 ci + 4 of 1..81, so co = 0 of frame 0 is 5 * 2 + 14 * 3 + 23 * 5
    assert centre[0].tolist() == [5.0, 14.0, 23.0] and got[0, 0, 0, 0] == 167.0


def test_conv_with_each_of_the_81_one_hot_filters_moves_one_channel():
    """w[co][ci][ky][kx] = 1 alone: out[co] is in[ci] moved by (ky - 1, kx - 1) with zeros shifted in, the other two output
    channels are 0 -- in every frame of the stack.  Pins correlation (no flip), the channel order and the zero padding."""
    rs = np.random.RandomState(1)
    x = rs.randint(1, 256, (1, 6, 2, 3)).astype(np.uint8)
    for co in range(3):
        for ci in range(3):
            for ky in range(3):
                for kx in range(3):
                    got = RandomConv.conv(x, _one_hot(co, ci, ky, kx)[None])
                    for f in range(2):
                        for o in range(3):
                            want = _moved(x[0, 3 * f + ci].astype(np.float64), ky - 1, kx - 1) if o == co else 0.0
                            assert np.array_equal(got[0, 3 * f + o], want + np.zeros((2, 3))), (co, ci, ky, kx, f, o)
    # one of them by hand: the tap above-left (ky = kx = 0) of channel 2 into channel 0
    got = RandomConv.conv(x, _one_hot(0, 2, 0, 0)[None])[0, 0]
    assert got.tolist() == [[0.0, 0.0, 0.0], [0.0, float(x[0, 2, 0, 0]), float(x[0, 2, 0, 1])]]


def test_conv_takes_per_sample_weights_and_the_identity_returns_the_input():
    rs = np.random.RandomState(2)
    x = rs.randint(0, 256, (3, 9, 4, 5)).astype(np.uint8)
    w = np.stack([_identity(), _one_hot(1, 0, 1, 1), 2.0 * _identity()])
    got = RandomConv.conv(x, w.reshape(3, 81))  # (B, 81) is accepted too
    assert np.array_equal(got[0], x[0]) and np.array_equal(got[2], 2.0 * x[2])
    assert np.array_equal(got[1, 1::3], x[1, 0::3]) and not got[1, 0::3].any() and not got[1, 2::3].any()


# ------------------------------------------------------------------------------------------------ 2. draw_weights
@pytest.mark.parametrize("seed", [0, 7])
def test_draw_weights_is_one_scaled_randn_when_p_is_one(seed):
    aug = RandomConv(HW)
    torch.manual_seed(seed)
    w = aug.draw_weights(5)
    after = torch.get_rng_state()
    assert w.shape == (5, 3, 3, 3, 3) and w.dtype == torch.float32
    torch.manual_seed(seed)
    want = torch.randn(5, 3, 3, 3, 3) * SCALE
    assert torch.equal(w, want)
    assert torch.equal(after, torch.get_rng_state())  # exactly that one draw was consumed


def test_draw_weights_with_p_zero_is_all_identity():
    torch.manual_seed(3)
    w = RandomConv(HW, p=0).draw_weights(6)
    assert w.dtype == torch.float32 and all(np.array_equal(w[i].numpy(), _identity()) for i in range(6))
    assert torch.equal(RandomConv.identity_filter(), torch.from_numpy(_identity()))


def test_draw_weights_with_p_between_replaces_exactly_the_rows_that_lose_the_second_draw():
    n = 40
    torch.manual_seed(4)
    w = RandomConv(HW, p=0.6).draw_weights(n)
    after = torch.get_rng_state()
    torch.manual_seed(4)
    drawn = torch.randn(n, 3, 3, 3, 3) * SCALE
    keep = torch.rand(n) < 0.6
    assert torch.equal(after, torch.get_rng_state())  # randn, then rand: nothing else
    assert 0 < int(keep.sum()) < n
    for i in range(n):
        assert torch.equal(w[i], drawn[i] if keep[i] else torch.from_numpy(_identity())), i


# ------------------------------------------------------------------------------------------------ 3. validation
@pytest.mark.parametrize("p", [True, False, -0.01, 1.5, "1", None, float("nan")])
def test_constructor_refuses_a_p_that_is_no_probability(p):
    with pytest.raises(ValueError, match="RandomConv: p"):
        RandomConv(HW, p)
    with pytest.raises(ValueError, match="RandomConv: p"):
        curla_amd.make_augmentor("random_conv", HW, conv_p=p)


def test_constructor_and_make_augmentor():
    with pytest.raises(AssertionError):  # (IdentityAugmentation's own check, as for every augmentation)
        RandomConv((9, 84, 84))
    a = curla_amd.make_augmentor("random_conv", (84, 84))
    assert type(a) is RandomConv is curla_amd.RandomConv and "RandomConv" in curla_amd.__all__
    assert a.output_shape == (84, 84) == a.input_shape and a.p == 1.0
    assert curla_amd.make_augmentor("random_conv", (84, 84), conv_p=0.25).p == 0.25
    assert RandomConv(HW, p=1).p == 1.0 and RandomConv(HW, p=np.float32(0.5)).p == 0.5
    with pytest.raises(TypeError):
        curla_amd.make_augmentor("random_conv", HW, None, 0.5)  # conv_p is keyword-only
    img = np.arange(24).reshape(6, 2, 2)
    assert a.evaluation_augmentation(img) is img
    with pytest.raises(RuntimeError, match="HIP device only"):  # no CPU path
        RandomConv((2, 2)).training_augmentation(torch.zeros(1, 6, 2, 2))


# ------------------------------------------------------------------------------------------------ 4. the buffer
def _rb(B, **kw):
    rb = ReplayBuffer((C,) + HW, (2,), CAP, B, "cpu", RandomConv(HW), **kw)
    rs = np.random.RandomState(3)
    for _ in range(12):
        f = rs.randint(0, 256, (C,) + HW, dtype=np.uint8)
        rb.add(f, [0.1, -0.2], 0.5, f, False)
    return rb


@pytest.mark.parametrize("B", [4, 5])
def test_block_layout_offsets_alignment_and_fill(B):
    """Three runs of float [B][81] behind the offsets, each 4-byte aligned, the stride padded (odd B) so that nbytes
    stays a multiple of 8; an unstaged buffer keeps the plain block."""
    base = 2 * B * 8 + 6 * B * 4
    plain = _rb(B).block_layout()
    assert plain["nbytes"] == base and plain["aug"] is None and "aug_weights" not in plain
    rb = _rb(B, staged_aug=True)
    assert rb.staged_aug
    lay = rb.block_layout()
    stride = 324 * B + (4 if B % 2 else 0)
    assert (lay["aug"], lay["aug_stride"], lay["aug_weights"]) == (base, stride, 324 * B)
    assert lay["aug_order"] is None and lay["aug_rng"] is None
    assert lay["nbytes"] == base + 3 * stride == rb._h_index.shape[1] == rb._d_index.shape[1]
    assert lay["nbytes"] % 8 == 0 and lay["tail"] == lay["nbytes"] and lay["graph_nbytes"] == lay["nbytes"] + 80
    assert all((lay["aug"] + j * stride) % 4 == 0 for j in range(3))
    torch.manual_seed(1)
    drawn = rb.draw_aug()
    torch.manual_seed(1)
    assert len(drawn) == 3 and all(torch.equal(d, torch.randn(B, 3, 3, 3, 3) * SCALE) for d in drawn)  # obs, next_obs, pos
    assert not torch.equal(drawn[0], drawn[2])
    host = torch.full((lay["graph_nbytes"],), 0xEE, dtype=torch.uint8)
    rb._fill_aug(host, drawn)
    raw = host.numpy()
    for j, w in enumerate(drawn):
        a = base + j * stride
        assert np.array_equal(raw[a:a + 324 * B].view(np.float32).reshape(B, 3, 3, 3, 3), w.numpy())
        assert (raw[a + 324 * B:a + stride] == 0xEE).all()  # the padding is nobody's
        # ... and _aug_args reads the same run back as the [B, 81] tensor the kernel takes
        assert torch.equal(rb._aug_args(host, j), w.reshape(B, 81)) and rb._aug_args(host, j).data_ptr() == host.data_ptr() + a
    assert (raw[:base] == 0xEE).all() and (raw[lay["tail"]:] == 0xEE).all()


def test_draw_indices_gives_zero_offsets_and_consumes_numpy_only():
    rb = _rb(4)
    np.random.seed(5)
    torch.manual_seed(5)
    t0 = torch.get_rng_state()
    idxs, offs = rb.draw_indices()
    assert offs.shape == (6, 4) and not offs.any() and idxs.shape == (4,)
    assert torch.equal(t0, torch.get_rng_state())
    np.random.seed(5)
    assert np.array_equal(idxs, np.random.randint(0, 12, size=4))


@pytest.mark.parametrize("dedup", [False, True])
def test_staged_sample_launches_the_staging_kernel_then_three_convolutions_on_the_block(trace, dedup):
    B = 4
    rb = _rb(B, staged_aug=True, dedup_frames=dedup)
    lay = rb.block_layout()
    del trace[:]
    torch.manual_seed(2)
    np.random.seed(2)
    obs, _, _, nxt, _, kw = rb.sample_cpc_refs()
    names = [n for n, _ in trace]
    gathers = ["curla_gather_stacks"] * 2 if dedup else []
    # (a buffer without pinned slots stages its block with a copy and gathers the scalars from the device block's
    # indices; the staging KERNEL of a pinned block is the first launch of test_graph_slot_... below)
    assert names == ["curla_gather_transition_scalars"] + gathers + ["curla_random_conv"] * 3
    dev = rb._sample_slots[rb._sample_slot]["dev"]
    assert trace[0][1][1] == dev.data_ptr() and dev.numel() == lay["nbytes"]
    convs = [a for n, a in trace if n == "curla_random_conv"]
    frame = C * HW[0] * HW[1]
    for j, a in enumerate(convs):
        assert a[2] == dev.data_ptr() + lay["aug"] + j * lay["aug_stride"]  # the tensor's run inside the device block
        assert a[3:7] == (B, C, HW[0], HW[1]) and len(a) == 9
        if dedup:  # the gathered stacks, rows 0..B-1
            mb = rb._sample_slots[rb._sample_slot]["mb_u8"]
            assert a[0] == mb.data_ptr() + (frame * B if j == 1 else 0) and a[1] is None
        else:      # the rings at the sampled rows
            assert a[0] == (rb.next_obses if j == 1 else rb.obses).data_ptr() and a[1] == dev.data_ptr()
    # obs and next_obs are the two halves of one [2B] float tensor, pos a tensor of its own
    assert convs[1][7] == convs[0][7] + 4 * B * frame and convs[2][7] not in (convs[0][7], convs[1][7])
    assert obs.src.data_ptr() == convs[0][7] and nxt.src.data_ptr() == convs[1][7] and kw["obs_pos"].src.data_ptr() == convs[2][7]
    assert obs.pair[0].B == 2 * B and obs.pair[0].src.data_ptr() == convs[0][7]


def _states():
    s = np.random.get_state()
    return torch.get_rng_state().clone(), (s[1].copy(), s[2], s[3], s[4])


def _same(a, b):
    return torch.equal(a[0], b[0]) and np.array_equal(a[1][0], b[1][0]) and a[1][1:] == b[1][1:]


@pytest.mark.parametrize("p", [1.0, 0.5])
def test_staged_and_unstaged_buffers_consume_the_host_streams_alike(trace, p):
    """indices (NumPy), then the weights of obs, next_obs, pos (torch's CPU generator): the same draws in the same order,
    and the same kernels, whether the weights travel in the block or in a pinned block of their own per tensor."""
    ends, launches, weights = [], [], []
    for staged in (False, True):
        aug = RandomConv(HW, p)
        rb = ReplayBuffer((C,) + HW, (2,), CAP, 4, "cpu", aug, staged_aug=staged)
        f = np.zeros((C,) + HW, dtype=np.uint8)
        for _ in range(12):
            rb.add(f, [0.1, -0.2], 0.5, f, False)
        seen = []
        real = aug.draw_weights
        aug.draw_weights = lambda n, real=real, seen=seen: (seen.append(real(n)), seen[-1])[1]
        torch.manual_seed(11)
        np.random.seed(11)
        del trace[:]
        rb.sample_cpc_refs()
        rb.sample_cpc()
        ends.append(_states())
        launches.append([n for n, _ in trace])
        weights.append(seen)
    assert _same(*ends)
    assert launches[0].count("curla_random_conv") == 6
    assert [n for n in launches[0] if n != "curla_nhwc_to_nchw"] == [n for n in launches[1] if n != "curla_nhwc_to_nchw"]
    assert len(weights[0]) == len(weights[1]) == 6 and all(torch.equal(a, b) for a, b in zip(*weights))
    torch.manual_seed(11)
    np.random.seed(11)
    assert not _same(ends[0], _states())  # ... and the streams did move


def test_graph_slot_launches_three_convolutions_into_its_guarded_buffers(trace):
    B = 4
    rb = _rb(B, staged_aug=True)
    lay = rb.block_layout()
    g = rb.graph_block(0)
    assert g["host"].numel() == g["dev"].numel() == lay["graph_nbytes"]
    np.random.seed(4)
    torch.manual_seed(4)
    idxs, offs = rb.draw_indices()
    drawn = rb.draw_aug()
    rb.graph_write(0, idxs, offs, bytes(range(80)), drawn)
    raw = g["host"].numpy()
    assert raw[lay["tail"]:].tobytes() == bytes(range(80))
    assert np.array_equal(raw[lay["aug"]:lay["aug"] + 324 * B].view(np.float32), drawn[0].numpy().reshape(-1))
    before = _states()
    del trace[:]
    rb.graph_refs(0)
    assert _same(before, _states())  # nothing is drawn while a graph is captured
    assert [n for n, _ in trace] == ["curla_sample_stage"] + ["curla_random_conv"] * 3
    outs = [g["both_f32"].data_ptr(), g["both_f32"][B:].data_ptr(), g["pos_f32"].data_ptr()]
    for j, (_, a) in enumerate(trace[1:]):
        assert a[2] == g["dev"].data_ptr() + lay["aug"] + j * lay["aug_stride"] and a[7] == outs[j]
