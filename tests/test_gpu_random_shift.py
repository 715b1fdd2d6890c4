"""``RandomShift`` on the device: ``curla_random_shift_u8`` against the NumPy edge-pad restatement, the replay buffer's
routes (plain storage in one and in two allocations, the de-duplicated frame store, ``sample_cpc``), a whole update
against the update of host-shifted pixels, and update graphs.  Everything is bit for bit (``torch.equal``): the kernel
only moves bytes and the update downstream of it is the existing uint8-ring update."""
import collections

import numpy as np
import pytest
import torch

from tests.test_gpu_agent import HP, NullLogger
from tests.test_gpu_graph_aug import _episode, _run, _state

pytestmark = pytest.mark.gpu

GUARD, GUARD_BYTE = 256, 0xA5


def shifted(frames_hwc, dy, dx, pad):
    """The restatement, per sample: np.pad(in, ((pad, pad), (pad, pad), (0, 0)), mode='edge')[dy:dy + H, dx:dx + W]."""
    n, h, w, _ = frames_hwc.shape
    out = np.empty_like(frames_hwc)
    for s in range(n):
        padded = np.pad(frames_hwc[s], ((pad, pad), (pad, pad), (0, 0)), mode="edge")
        out[s] = padded[dy[s]:dy[s] + h, dx[s]:dx[s] + w]
    return out


def forced_offsets(pad, n, seed):
    """(dy, dx) of n samples: the four corners of the offset range, the centre (a pure copy), then random ones."""
    rs = np.random.RandomState(seed)
    first = [(0, 0), (2 * pad, 2 * pad), (0, 2 * pad), (2 * pad, 0), (pad, pad)]
    rest = [tuple(rs.randint(0, 2 * pad + 1, 2)) for _ in range(max(0, n - len(first)))]
    both = np.array((first + rest)[:n], dtype=np.int32).reshape(n, 2)
    return both[:, 0].copy(), both[:, 1].copy()


# ------------------------------------------------------------------------------------------------ 1. the kernel
GEOMETRIES = [
    (11, 13, 3, 2, 5),    # frame of 429 bytes: the byte path everywhere
    (40, 44, 9, 4, 7),    # 15840 = 16 x 990 bytes, but rows of 396: 16-byte groups straddle rows
    (20, 20, 12, 4, 4),   # rows of 240 bytes = 15 whole groups: the fast path proper
    (9, 7, 6, 8, 3),      # pad larger than the image: clamping on every side
]


@pytest.mark.parametrize("H,W,C,pad,n", GEOMETRIES)
def test_kernel_equals_the_edge_pad_restatement(H, W, C, pad, n):
    """Rows: unordered, repeated, from both halves of a double ring; read with a period shorter than n and without an
    index (rows s % period).  Offsets: all four corners and the centre over the launches of a geometry.  The output sits
    between guard bytes, on and off the 16-byte grid."""
    from curla_amd import ops
    cap = 6
    frame = H * W * C
    rs = np.random.RandomState(H * W + C)
    host = rs.randint(0, 256, (2 * cap, H, W, C), dtype=np.uint8)
    store = torch.zeros(2 * cap * frame + 32, dtype=torch.uint8, device="cuda")
    ring = store[:2 * cap * frame].view(2 * cap, H, W, C)
    ring.copy_(torch.from_numpy(host))
    launches = -(-5 // n) + 1
    all_dy, all_dx = forced_offsets(pad, launches * n, 7)
    seen = set()
    for k in range(launches):
        dy, dx = all_dy[k * n:(k + 1) * n], all_dx[k * n:(k + 1) * n]
        seen |= set(zip(dy.tolist(), dx.tolist()))
        d_dy, d_dx = torch.from_numpy(dy).cuda(), torch.from_numpy(dx).cuda()
        period = max(1, n - 2)
        rows = rs.randint(0, 2 * cap, size=period)
        rows[0] = cap + 1 + k          # the second (next_obs) half of the double ring
        if period > 2:
            rows[-1] = rows[1]         # a repeat
        cases = [(torch.from_numpy(rows.astype(np.int64)).cuda(), period, rows[np.arange(n) % period]),
                 (None, n, np.arange(n)),
                 (None, period, np.arange(n) % period)]
        for idx, per, src_rows in cases:
            want = torch.from_numpy(shifted(host[src_rows], dy, dx, pad))
            for lead in (0, 3):  # out on a 16-byte boundary (torch allocations are), and 3 bytes off it
                buf = torch.full((GUARD + lead + n * frame + GUARD,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
                out = buf[GUARD + lead:GUARD + lead + n * frame].view(n, H, W, C)
                assert (out.data_ptr() % 16 == 0) == (lead == 0)
                ops.random_shift_u8(ring, idx, per, d_dy, d_dx, pad, n, out)
                got = buf.cpu()
                assert torch.equal(got[GUARD + lead:GUARD + lead + n * frame].view(n, H, W, C), want), (k, per, lead)
                assert bool((got[:GUARD + lead] == GUARD_BYTE).all()) and bool((got[GUARD + lead + n * frame:] == GUARD_BYTE).all())
    assert {(0, 0), (2 * pad, 2 * pad), (0, 2 * pad), (2 * pad, 0), (pad, pad)} <= seen
    assert not bool(store[-32:].any())  # the ring's slack: never written
    # (pad, pad) is a pure copy
    one = torch.empty((1, H, W, C), dtype=torch.uint8, device="cuda")
    p = torch.full((1,), pad, dtype=torch.int32, device="cuda")
    ops.random_shift_u8(ring, torch.tensor([cap + 2], device="cuda"), 1, p, p, pad, 1, one)
    assert torch.equal(one[0], ring[cap + 2])


def test_kernel_refuses_bad_arguments_before_any_launch():
    from curla_amd import _lib
    lib = _lib.load()
    ring = torch.zeros(4 * 4 * 3 + 32, dtype=torch.uint8, device="cuda")
    off = torch.zeros(4, dtype=torch.int32, device="cuda")
    out = torch.zeros(4 * 4 * 3, dtype=torch.uint8, device="cuda")
    args = lambda period, pad, n: (ring.data_ptr(), None, period, off.data_ptr(), off.data_ptr(), pad, n, 3, 4, 4,  # noqa: E731
                                   out.data_ptr(), None)
    assert lib.curla_random_shift_u8(*args(1, -1, 1)) == -1
    assert lib.curla_random_shift_u8(*args(0, 1, 1)) == -1
    assert lib.curla_random_shift_u8(*args(1, 1, 0)) == -1
    assert lib.curla_random_shift_u8(*args(1, 2 ** 29, 1)) == -3
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. buffer routes
def _filled(in_hw, C, capacity, B, pad=4, dedup=False, n_fill=60, cls=None):
    import curla_amd
    aug = curla_amd.make_augmentor("random_shift", in_hw, pad=pad)
    rb = (cls or curla_amd.ReplayBuffer)((C,) + in_hw, (2,), capacity, B, torch.device("cuda"), aug, dedup_frames=dedup)
    ep = _episode(n_fill, C // 3, in_hw, 6)
    rb.add_batch(*ep)
    return rb, ep


def _injected(B, n_fill, pad, seed):
    rs = np.random.RandomState(seed)
    idxs = rs.randint(0, n_fill, size=B)
    idxs[1] = idxs[0]  # a repeat
    offs = np.empty((6, B), dtype=np.int32)
    for j in range(3):
        offs[2 * j], offs[2 * j + 1] = forced_offsets(pad, B, seed + j)
        offs[2 * j], offs[2 * j + 1] = np.roll(offs[2 * j], j), np.roll(offs[2 * j + 1], j)
    return idxs, offs


def _restated(ep, idxs, offs, pad):
    """(obs | next_obs | pos) of the minibatch as uint8 [3B, H, W, C], each tensor with its own offsets."""
    obs, nxt = ep[0][idxs].transpose(0, 2, 3, 1), ep[3][idxs].transpose(0, 2, 3, 1)
    return np.concatenate([shifted(obs, offs[0], offs[1], pad), shifted(nxt, offs[2], offs[3], pad),
                           shifted(obs, offs[4], offs[5], pad)])


def _check_refs(rb, sample, want, B):
    obs, act, rew, nxt, nd, kw = sample
    scratch = obs.src
    assert scratch.dtype == torch.uint8 and tuple(scratch.shape) == tuple(want.shape)
    assert torch.equal(scratch.cpu(), torch.from_numpy(want))
    for ref, row0 in ((obs, 0), (nxt, B), (kw["obs_pos"], 2 * B)):
        assert ref.src.data_ptr() == scratch.data_ptr() and ref.is_u8 == 1 and ref.B == B
        assert ref.idx.tolist() == list(range(row0, row0 + B)) and not bool(ref.h1.any()) and not bool(ref.w1.any())
        assert (ref.Hc, ref.Wc) == (ref.Hs, ref.Ws) == tuple(rb.obs_shape[1:])
        ref.check()
    pair, second = obs.pair
    assert second is nxt and pair.B == 2 * B and pair.idx.tolist() == list(range(2 * B)) and not bool(pair.h1.any())
    assert kw["obs_anchor"] is obs


@pytest.mark.parametrize("route", ["plain", "dedup", "two_allocations"])
def test_buffer_routes_give_the_restated_bytes(route):
    B, pad = 8, 4
    if route == "two_allocations":
        in_hw, C, cap = (11, 13), 3, 61  # 61 * 429 bytes: the next_obs ring would not start on a dword
    else:
        in_hw, C, cap = (40, 44), 9, 64
    rb, ep = _filled(in_hw, C, cap, B, pad, dedup=route == "dedup")
    if route != "dedup":  # (the frame store has no rings: its stacks are gathered per minibatch)
        assert (rb._both is None) == (route == "two_allocations")
    idxs, offs = _injected(B, 60, pad, 11)
    want = _restated(ep, idxs, offs, pad)
    sample = rb.sample_cpc_refs((idxs, offs))
    _check_refs(rb, sample, want, B)
    assert torch.equal(sample[1].cpu(), torch.from_numpy(ep[1][idxs]))
    assert torch.equal(sample[2].cpu().flatten(), torch.from_numpy(ep[2][idxs]))
    assert torch.equal(sample[4].cpu().flatten(), torch.from_numpy(1.0 - ep[4][idxs].astype(np.float32)))
    # the slack behind the scratch is never written, and a second sample lives in the other slot
    assert not bool(rb._shift_store[rb._sample_slot][3 * B * rb._frame:].any())
    idxs2, offs2 = _injected(B, 60, pad, 12)
    sample2 = rb.sample_cpc_refs((idxs2, offs2))
    _check_refs(rb, sample2, _restated(ep, idxs2, offs2, pad), B)
    assert sample2[0].src.data_ptr() != sample[0].src.data_ptr()
    assert torch.equal(sample[0].src.cpu(), torch.from_numpy(want))  # the first one is still intact
    # sample_cpc(): the reference contract, float NCHW in [0, 255], from the same scratch
    o, _, _, nx, _, kw = rb.sample_cpc((idxs, offs))
    want_f = torch.from_numpy(want.transpose(0, 3, 1, 2).astype(np.float32))
    for t, j in ((o, 0), (nx, 1), (kw["obs_pos"], 2)):
        assert t.dtype == torch.float32 and tuple(t.shape) == (B, C) + in_hw
        assert torch.equal(t.cpu(), want_f[j * B:(j + 1) * B])
    assert kw["obs_anchor"] is o


def test_scratch_is_counted_and_other_buffers_have_none():
    import curla_amd
    rb, _ = _filled((40, 44), 9, 64, 8)
    assert rb._shift_store.shape[0] == rb.N_SAMPLE_SLOTS and rb._shift_store.shape[1] >= 3 * 8 * rb._frame + 32
    assert rb._shift_store.data_ptr() % 256 == 0 and rb._shift_store.stride(0) % 256 == 0
    other = curla_amd.ReplayBuffer((9, 40, 44), (2,), 64, 8, torch.device("cuda"), curla_amd.RandomCrop((40, 44), (32, 36)))
    assert not hasattr(other, "_shift_store")


# ------------------------------------------------------------------------------------------------ 3. a whole update
class _HostShiftedBuffer:
    """Stands in for a replay buffer: hands out, per call, ring handles of the structure ``ReplayBuffer`` returns for
    a RandomShift (rows 0..3B-1, zero offsets, the pair over the first 2B) over a device tensor that holds frames
    shifted ON THE HOST with NumPy (+ the 32 bytes of slack), plus the transitions' scalars."""

    def __init__(self, batches, B, hw):
        self.batch_size, self.hw = B, hw
        self.batches = collections.deque(batches)
        self.rows = torch.arange(3 * B, dtype=torch.int64, device="cuda")
        self.zero = torch.zeros(3 * B, dtype=torch.int32, device="cuda")
        self.alive = []

    def sample_cpc_refs(self):
        from curla_amd import ops
        pixels, act, rew, nd = self.batches.popleft()
        B, hw, ar, z = self.batch_size, self.hw, self.rows, self.zero
        store = torch.zeros(pixels.size + 32, dtype=torch.uint8, device="cuda")
        ring = store[:pixels.size].view(pixels.shape)
        ring.copy_(torch.from_numpy(pixels))
        self.alive.append(store)
        obs, nxt, pos = (ops.ObsRef.from_ring(ring, ar[j * B:(j + 1) * B], z[:B], z[:B], B, hw) for j in range(3))
        obs.pair = (ops.ObsRef.from_ring(ring, ar[:2 * B], z[:2 * B], z[:2 * B], 2 * B, hw), nxt)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()  # noqa: E731
        return obs, dev(act), dev(rew).view(B, 1), nxt, dev(nd).view(B, 1), dict(obs_anchor=obs, obs_pos=pos,
                                                                               time_anchor=None, time_pos=None)


def _agent(seed, in_hw, C):
    import curla_amd
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    np.random.seed(seed)
    aug = curla_amd.make_augmentor("random_shift", in_hw)
    return curla_amd.CurlSacAgent((C,) + in_hw, (2,), torch.device("cuda"), aug, hidden_dim=64, **HP)


def test_an_update_is_the_update_of_the_shifted_pixels():
    """Steps 0, 1, 2 (critic + actor + target update, critic + CURL, ...) from a random_shift buffer with injected
    draws, against the same agent fed frames shifted with NumPy: parameters, targets, Adam moments, log_alpha and the
    device generator end bit-identical."""
    import curla_amd
    B, in_hw, C, pad, n_fill = 64, (40, 44), 9, 4, 400
    draws = [_injected(B, n_fill, pad, 30 + s) for s in range(3)]

    class Injected(curla_amd.ReplayBuffer):
        queue = collections.deque(draws)

        def draw_indices(self):
            return self.queue.popleft()

    agent_a = _agent(5, in_hw, C)
    rb, ep = _filled(in_hw, C, 512, B, pad, n_fill=n_fill, cls=Injected)
    for step in range(3):
        agent_a.update(rb, NullLogger(), step)
    torch.cuda.synchronize()
    assert not Injected.queue
    state_a = _state(agent_a, rb)

    agent_b = _agent(5, in_hw, C)
    batches = [(_restated(ep, i, o, pad), ep[1][i], ep[2][i], 1.0 - ep[4][i].astype(np.float32)) for i, o in draws]
    stand_in = _HostShiftedBuffer(batches, B, in_hw)
    for step in range(3):
        agent_b.update(stand_in, NullLogger(), step)
    torch.cuda.synchronize()
    state_b = _state(agent_b, stand_in)
    for k in state_a:
        assert torch.equal(state_a[k], state_b[k]), k
    assert float(state_a["critic_steps"][0]) == 3 and float(state_a["actor_steps"][0]) == 2
    # ... and the shift did matter: the same draws with zero shift end somewhere else
    agent_c = _agent(5, in_hw, C)
    centre = np.full((6, B), pad, dtype=np.int32)
    plain = _HostShiftedBuffer([(_restated(ep, i, centre, pad), ep[1][i], ep[2][i], 1.0 - ep[4][i].astype(np.float32))
                                for i, _ in draws], B, in_hw)
    for step in range(3):
        agent_c.update(plain, NullLogger(), step)
    torch.cuda.synchronize()
    assert not torch.equal(_state(agent_c, plain)["critic"], state_a["critic"])


# ------------------------------------------------------------------------------------------------ 4. update graphs
@pytest.mark.parametrize("dedup", [False, True], ids=["random_shift", "random_shift+dedup"])
def test_graph_replay_is_the_eager_update_bit_for_bit(dedup):
    """The protocol of tests/test_gpu_graph_aug.py: 14 mixed steps with log_interval 5 (0, 5, 10 log and run eagerly;
    1, 2 warm up; 3, 4, 6, 7 capture; 8, 9, 11, 12, 13 replay)."""
    setup = dict(aug="random_shift", dedup_frames=dedup)
    eager, calls_e, logs_e, _, _ = _run(False, **setup)
    graph, calls_g, logs_g, agent, rb = _run(True, **setup)
    replayed = [8, 9, 11, 12, 13]
    assert all(sum(calls_e[s].values()) > 15 for s in range(14))
    assert all(calls_e[s].get("curla_random_shift_u8") == 1 and calls_e[s].get("curla_sample_stage") == 1 for s in range(14))
    assert all(calls_e[s].get("curla_gather_stacks", 0) == (2 if dedup else 0) for s in range(14))
    assert [sum(calls_g[s].values()) for s in replayed] == [0] * len(replayed), calls_g
    assert all(sum(calls_g[s].values()) > 15 for s in (0, 1, 2, 3, 4, 5, 6, 7, 10)), calls_g
    assert len(agent._graphs) == 2 and all(len(r) == 2 and all(g["graph"] is not None for g in r)
                                           for r in agent._graphs.values())
    assert logs_e == logs_g
    for k in eager:
        assert torch.equal(eager[k], graph[k]), k
    assert float(eager["critic_steps"][0]) == 14 and float(eager["actor_steps"][0]) == 7
    blocks = rb._graph_blocks
    B, frame = rb.batch_size, rb._frame
    assert len(blocks) == 4
    for g in blocks.values():
        assert len(g["guards"]) == (4 if dedup else 2)
        for guard in g["guards"]:
            assert guard.numel() >= rb.GUARD and bool((guard == rb.GUARD_BYTE).all())
        assert g["shift_u8"].numel() == 3 * B * frame + 32
        assert bool(g["shift_u8"][:3 * B * frame].any()) and not bool(g["shift_u8"][-32:].any())
        if dedup:
            assert not bool(g["mb_u8"][-32:].any())


def test_rings_in_two_allocations_are_refused_by_enable_update_graphs():
    rb, _ = _filled((11, 13), 3, 61, 8)
    assert rb._both is None and not rb.graph_supported()
    agent = _agent(1, (40, 44), 9)
    with pytest.raises(ValueError, match="RandomShift.*both rings in one allocation"):
        agent.enable_update_graphs(rb)
    assert _filled((40, 44), 9, 64, 8)[0].graph_supported() and _filled((40, 44), 9, 64, 8, dedup=True)[0].graph_supported()


# ------------------------------------------------------------------------------------------------ 5. non-interference
@pytest.mark.parametrize("aug", ["random_crop", "identity"])
def test_other_uint8_buffers_launch_what_they_launched(aug):
    """One seeded update from a random_crop / identity buffer: no shift launch, and the per-kernel launch counters are
    those of a second, identically built buffer and agent (nothing RandomShift added depends on state it left)."""
    counts = []
    for _ in range(2):
        _, per_step, _, _, rb = _run(False, steps=1, aug=aug)
        assert not hasattr(rb, "_shift_store")
        counts.append(per_step[0])
    assert counts[0].get("curla_random_shift_u8", 0) == 0
    assert counts[0] == counts[1] and sum(counts[0].values()) == sum(counts[1].values()) > 15
    assert counts[0]["curla_sample_stage"] == 1
