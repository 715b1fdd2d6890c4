"""Host side of ``ReplayBuffer(..., staged_aug=True)`` and of the update graphs that build on it, without a GPU (the
launch-trace hook: nothing is computed): the order of the host's random draws, the layout of the extended minibatch
block, what a graph slot launches and from where, and that a capture that raises leaves every random stream alone."""
import contextlib

import numpy as np
import pytest
import torch

import curla_amd
from curla_amd import _lib
from curla_amd.utils import ReplayBuffer
from tests.test_host_logic import HP, NullLogger

C, HW, B, CAP = 9, (34, 40), 8, 32
N_EL = B * C * HW[0] * HW[1]


class FakeDeviceGenerator:
    """Stands in for the HIP device's torch generator (seed + Philox offset) where there is no device."""

    def __init__(self, seed=0xDEADBEEF12345, offset=40):
        self.seed, self.offset = seed, offset

    def get_offset(self):
        return self.offset

    def set_offset(self, v):
        self.offset = int(v)

    def initial_seed(self):
        return self.seed


@pytest.fixture
def fake_gen(monkeypatch):
    gen = FakeDeviceGenerator()
    monkeypatch.setattr(ReplayBuffer, "_noise_generator", lambda self: gen)
    return gen


@pytest.fixture
def trace():
    calls = []
    _lib.set_trace_hook(lambda name, args: calls.append((name, args)))
    yield calls
    _lib.set_trace_hook(None)


def _rb(aug, **kw):
    rb = ReplayBuffer((C,) + HW, (2,), CAP, B, "cpu", aug, **kw)
    rs = np.random.RandomState(3)
    for _ in range(12):
        f = rs.randint(0, 256, (C,) + HW, dtype=np.uint8)
        rb.add(f, [0.1, -0.2], 0.5, f, False)
    return rb


def _states():
    s = np.random.get_state()
    return torch.get_rng_state().clone(), (s[1].copy(), s[2], s[3], s[4])


def _same(a, b):
    return torch.equal(a[0], b[0]) and np.array_equal(a[1][0], b[1][0]) and a[1][1:] == b[1][1:]


def test_staged_color_jiggle_consumes_the_host_streams_like_the_default_buffer(trace):
    ends, launches = [], []
    for staged in (False, True):
        aug = curla_amd.ColorJiggle(HW)
        rb = _rb(aug, staged_aug=staged)
        torch.manual_seed(11)
        np.random.seed(11)
        del trace[:]
        for _ in range(3):
            rb.sample_cpc_refs()
        ends.append(_states())
        launches.append([n for n, _ in trace])
    assert _same(*ends)
    assert launches[0] == launches[1] and launches[0].count("curla_color_jiggle") == 9  # same kernels, same order
    # ... and the streams did move
    torch.manual_seed(11)
    np.random.seed(11)
    assert not _same(ends[0], _states())


def test_staged_noisy_cover_draw_order_and_counter_ranges(trace, fake_gen):
    """NumPy (indices, then three colours per tensor) is consumed as by the default buffer; the default buffer's
    torch.randn is replaced by three counter ranges of ceil(n / 4) taken from the device generator, consecutive and
    disjoint, and torch's CPU generator is not touched."""
    ends = []
    for staged in (False, True):
        aug = curla_amd.NoisyCover(HW)
        rb = _rb(aug, staged_aug=staged)
        torch.manual_seed(12)
        np.random.seed(12)
        before = _states()
        del trace[:]
        rb.sample_cpc_refs()
        ends.append(_states())
    assert np.array_equal(ends[0][1][0], ends[1][1][0]) and ends[0][1][1:] == ends[1][1][1:]
    assert torch.equal(ends[1][0], before[0])  # staged: no host normal draw
    cnt = (N_EL + 3) // 4
    assert fake_gen.offset == 40 + 3 * 4 * cnt
    launched = [a for n, a in trace if n == "curla_noisy_cover_rng"]
    assert len(launched) == 3 and not [n for n, _ in trace if n == "curla_noisy_cover"]
    np.random.seed(12)
    np.random.randint(0, 12, size=B)
    fake_gen.offset = 400
    draws = rb.draw_aug()
    assert [d[2] for d in draws] == [100, 100 + cnt, 100 + 2 * cnt]  # [ctr, ctr + cnt) disjoint, back to back
    assert all(d[1] == fake_gen.seed for d in draws) and all(len(d[0]) == 3 for d in draws)


def test_staged_noisy_cover_needs_a_generator_with_an_offset():
    with pytest.raises(ValueError, match="offset"):
        ReplayBuffer((C,) + HW, (2,), CAP, B, "cpu", curla_amd.NoisyCover(HW), staged_aug=True)
    # the default buffer does not care, and staged_aug means nothing to the uint8 augmentations
    assert not ReplayBuffer((C,) + HW, (2,), CAP, B, "cpu", curla_amd.NoisyCover(HW)).staged_aug
    assert not ReplayBuffer((C,) + HW, (2,), CAP, B, "cpu", curla_amd.RandomCrop(HW, (28, 34)), staged_aug=True).staged_aug


def test_block_layout_offsets_alignment_and_sizes(fake_gen):
    base = 2 * B * 8 + 6 * B * 4
    plain = _rb(curla_amd.RandomCrop(HW, (28, 34)))
    lay = plain.block_layout()
    assert lay["nbytes"] == base == plain._h_index.shape[1] and lay["aug"] is None
    assert lay["tail"] == base and lay["graph_nbytes"] == base + ReplayBuffer.GRAPH_TAIL == base + 80
    # an unstaged float buffer keeps the plain block: nothing changes for it
    assert _rb(curla_amd.ColorJiggle(HW)).block_layout() == lay

    cj = _rb(curla_amd.ColorJiggle(HW), staged_aug=True)
    lay = cj.block_layout()
    k = C // 3
    assert lay["aug"] == base and lay["aug_order"] == 16 * B * k and lay["aug_stride"] == 16 * B * k + 16
    assert lay["nbytes"] == base + 3 * (16 * B * k + 16) == cj._h_index.shape[1] == cj._d_index.shape[1]
    assert lay["tail"] == lay["nbytes"] and lay["tail"] % 8 == 0 and lay["graph_nbytes"] == lay["nbytes"] + 80
    torch.manual_seed(1)
    aug = cj.draw_aug()
    host = torch.zeros(lay["graph_nbytes"], dtype=torch.uint8)
    cj._fill_aug(host, aug)
    raw = host.numpy()
    for j, (params, order) in enumerate(aug):
        a = base + j * lay["aug_stride"]
        assert np.array_equal(raw[a:a + 16 * B * k].view(np.float32).reshape(B * k, 4), params.numpy())
        assert np.array_equal(raw[a + 16 * B * k:a + lay["aug_stride"]].view(np.int32), order.numpy())
        assert sorted(order.tolist()) == [0, 1, 2, 3]
    assert not raw[:base].any() and not raw[lay["tail"]:].any()  # indices and the control tail are not this call's

    nc = _rb(curla_amd.NoisyCover(HW), staged_aug=True)
    lay = nc.block_layout()
    assert (lay["aug"], lay["aug_stride"], lay["aug_rng"]) == (base, 32, 16)
    assert lay["nbytes"] == base + 96 == nc._h_index.shape[1] and lay["graph_nbytes"] == base + 96 + 80
    fake_gen.offset = 2 ** 40 + 8
    np.random.seed(2)
    aug = nc.draw_aug()
    host = torch.zeros(lay["graph_nbytes"], dtype=torch.uint8)
    nc._fill_aug(host, aug)
    raw = host.numpy()
    cnt = (N_EL + 3) // 4
    for j, (colors, seed, ctr) in enumerate(aug):
        a = base + 32 * j
        assert (a + 16) % 8 == 0  # the u64 pair is 8-byte aligned inside an 8-byte aligned block
        assert raw[a:a + 12].view(np.float32).tolist() == [float(c) for c in colors]
        assert raw[a + 16:a + 32].view(np.uint64).tolist() == [fake_gen.seed, 2 ** 38 + 2 + j * cnt] == [seed, ctr]


def test_graph_slot_block_and_launches(trace, fake_gen):
    """graph_block / graph_write / graph_refs on the trace hook: the slot's block has the layout's size, graph_write
    fills indices, parameters and tail, and graph_refs launches -- without a single host draw -- the staging kernel,
    the two stack gathers (de-duplicated store) and the three augmentation kernels, each reading ITS parameters from
    the device copy of the block and writing into the slot's own guarded buffers."""
    for aug, kernel in ((curla_amd.ColorJiggle(HW), "curla_color_jiggle"), (curla_amd.NoisyCover(HW), "curla_noisy_cover_rng")):
        rb = _rb(aug, staged_aug=True, dedup_frames=True)
        lay = rb.block_layout()
        g = rb.graph_block(0)
        assert g["host"].numel() == g["dev"].numel() == lay["graph_nbytes"] and g["tail"] == lay["tail"]
        assert rb.graph_block(0) is g and rb.graph_block(1) is not g
        assert len(g["guards"]) == 5 and all(bool((x == rb.GUARD_BYTE).all()) and x.numel() >= rb.GUARD for x in g["guards"])
        assert g["both_f32"].shape == (2 * B,) + HW + (C,) and g["pos_f32"].shape == (B,) + HW + (C,)
        # every buffer starts right behind a guard, a multiple of 256 bytes into its (device-aligned) allocation
        for buf, first, guard in ((g["mb_u8"], 0, 0), (g["both_f32"], 2, 2), (g["pos_f32"], 2, 3)):
            assert buf.data_ptr() == g["guards"][guard].data_ptr() + g["guards"][guard].numel()
            assert (buf.data_ptr() - g["guards"][first].data_ptr()) % 256 == 0
        assert g["mb_u8"].data_ptr() - g["guards"][0].data_ptr() == rb.GUARD
        np.random.seed(4)
        idxs, offs = rb.draw_indices()
        drawn = rb.draw_aug()
        tail = bytes(range(80))
        rb.graph_write(0, idxs, offs, tail, drawn)
        raw = g["host"].numpy()
        assert raw[:8 * B].view(np.int64).tolist() == idxs.tolist()
        assert raw[lay["tail"]:].tobytes() == tail
        assert raw[lay["aug"]:lay["tail"]].any()
        before = _states(), fake_gen.offset
        del trace[:]
        refs = rb.graph_refs(0)
        assert _same(before[0], _states()) and fake_gen.offset == before[1]
        names = [n for n, _ in trace]
        assert names == ["curla_sample_stage", "curla_gather_stacks", "curla_gather_stacks", kernel, kernel, kernel]
        stage = trace[0][1]
        assert stage[1] == g["dev"].data_ptr() and stage[2] == lay["graph_nbytes"]
        dev0 = g["dev"].data_ptr()
        outs = [g["both_f32"].data_ptr(), g["both_f32"][B:].data_ptr(), g["pos_f32"].data_ptr()]
        srcs = [g["mb_u8"].data_ptr(), g["mb_u8"].data_ptr() + B * C * HW[0] * HW[1], g["mb_u8"].data_ptr()]
        for j, (_, a) in enumerate(trace[3:]):
            at = dev0 + lay["aug"] + j * lay["aug_stride"]
            assert a[0] == srcs[j] and a[1] is None  # the gathered stacks, rows 0..B-1
            if kernel == "curla_color_jiggle":
                assert (a[2], a[3], a[8]) == (at, at + lay["aug_order"], outs[j])
            else:
                assert a[5] == at + 16 and a[9] == at and (a[3], a[4]) == (0, 0)  # rng_dev, colors_dev; nothing by value
                assert a[2] == 10.0 and a[16] == outs[j] and a[17] is None
        obs, _, _, nxt, _, kw = refs
        assert obs.src.data_ptr() == outs[0] and nxt.src.data_ptr() == outs[1] and kw["obs_pos"].src.data_ptr() == outs[2]
        assert obs.pair[0].src.data_ptr() == outs[0] and obs.pair[0].B == 2 * B


def test_a_capture_that_raises_leaves_all_three_random_streams_alone(trace, fake_gen, monkeypatch):
    """An update whose graph capture fails half way (the hook raises at the 12th launch of the capture, after the
    staging and cover launches and part of the critic phase have been recorded) runs eagerly instead -- from exactly the stream positions
    (NumPy, torch's CPU generator, the device generator) the update started at."""
    aug = curla_amd.NoisyCover(HW)
    curla_amd.set_seed_everywhere(1)
    agent = curla_amd.CurlSacAgent((C,) + HW, (2,), "cpu", aug, hidden_dim=64, **{**HP, "log_interval": 1000})
    rb = _rb(aug, staged_aug=True)

    class FakeGraph:
        def replay(self):
            raise AssertionError("nothing was captured")
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    monkeypatch.setattr(torch.cuda, "CUDAGraph", FakeGraph)
    monkeypatch.setattr(torch.cuda, "graph", lambda *a, **k: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(torch.cuda, "default_generators", (fake_gen,), raising=False)
    # what enable_update_graphs sets up (it refuses a CPU agent before anything else)
    agent._graphs, agent._graph_rb, agent._graph_warm, agent._graph_depth = {}, rb, 0, 2
    agent._graph_seen, agent._graph_key_at_capture = {}, None

    seen = {"in_capture": 0}

    def hook(name, args):
        if agent._graph_cap is not None:
            seen["in_capture"] += 1
            if seen["in_capture"] == 12:
                raise RuntimeError("injected capture failure")
    _lib.set_trace_hook(hook)
    at_eager_entry = []
    real_eager = agent._update_eager
    monkeypatch.setattr(agent, "_update_eager", lambda *a, **k: (at_eager_entry.append((_states(), fake_gen.offset)),
                                                                 real_eager(*a, **k))[1])
    torch.manual_seed(21)
    np.random.seed(21)
    start = _states(), fake_gen.offset
    with pytest.warns(RuntimeWarning, match="injected capture failure"):
        agent.update(rb, NullLogger(), 1)
    assert seen["in_capture"] == 12                     # the capture got well past the minibatch kernels
    assert len(at_eager_entry) == 1
    assert _same(at_eager_entry[0][0], start[0]) and at_eager_entry[0][1] == start[1]
    assert agent._graph_cap is None and agent._graphs[agent._graph_kind(1)][0]["graph"] is None
    # the eager update that followed did draw: indices and colours from NumPy, the three tensors' noise ranges
    # (a CPU agent's policy noise comes from torch's CPU generator: not counted here)
    assert not np.array_equal(_states()[1][0], start[0][1][0])
    assert fake_gen.offset == start[1] + 3 * 4 * ((N_EL + 3) // 4)


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
def test_sampling_bounds_hold_for_numpys_own_normals(seed):
    """The two bounds tests/test_gpu_graph_aug.py puts on the in-kernel noise -- |mean| <= 6 std / sqrt(n) and
    |s / std - 1| <= 6 / sqrt(2 n), six standard errors of a normal sample's mean and standard deviation -- checked on
    NumPy's own normals at the same n and std before they are relied on."""
    n, std = 1_806_250, 10.0
    x = np.random.RandomState(seed).standard_normal(n) * std
    assert abs(x.mean()) <= 6 * std / np.sqrt(n)
    assert abs(x.std(ddof=1) / std - 1) <= 6 / np.sqrt(2 * n)
