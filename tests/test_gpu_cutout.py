"""``RandomCutout`` on the device: ``curla_cutout_u8`` against a NumPy restatement of its clamp-and-paint rule, the replay
buffer's routes (plain ring, frame store, rings in two allocations, n-step, ``sample_cpc``), a whole update against the
update of frames cut on the host, and update graphs.  Everything is bit for bit (``torch.equal``): the kernel only moves
and paints bytes and the update downstream of it is the existing uint8-ring update."""
import collections

import numpy as np
import pytest
import torch

from tests.test_gpu_agent import HP, NullLogger
from tests.test_gpu_graph_aug import _episode, _run, _state
from tests.test_gpu_random_shift import _HostShiftedBuffer

pytestmark = pytest.mark.gpu

GUARD, GUARD_BYTE = 256, 0xA5


def cut_nhwc(frames, y0, x0, size, rgb):
    """The restatement on uint8 [n, H, W, C], with the kernel's clamp rule: y0c = clamp(y0, 0, H), bhc = clamp(bh, 0,
    H - y0c), likewise in x; size = bh | bw << 16, rgb = r | g << 8 | b << 16 (top byte ignored)."""
    out = frames.copy()
    n, H, W, C = frames.shape
    for s in range(n):
        yc, xc = min(max(int(y0[s]), 0), H), min(max(int(x0[s]), 0), W)
        bh, bw = min(int(size[s]) & 0xFFFF, H - yc), min((int(size[s]) >> 16) & 0xFFFF, W - xc)
        for c in range(C):
            out[s, yc:yc + bh, xc:xc + bw, c] = (int(rgb[s]) >> (8 * (c % 3))) & 0xFF
    return out


def _edge_boxes(H, W, C):
    """A one-row box whose first byte is the last byte of a 16-byte group, and one whose last byte is the first byte of
    a group (byte offsets inside the frame); None where the geometry has no such box."""
    rb, first, last = W * C, None, None
    for y in range(1, H):
        for x in range(W):
            if first is None and (y * rb + x * C) % 16 == 15:
                first = (y, x, 1, min(2, W - x))
            if last is None and (y * rb + (x + 1) * C - 1) % 16 == 0:
                last = (y, max(0, x - 1), 1, x + 1 - max(0, x - 1))
    return first, last


def _boxes(H, W, C, few=False):
    first, last = _edge_boxes(H, W, C)
    boxes = [b for b in (first, last) if b is not None]
    boxes += [(1, 0, 2, W),                       # full row width: the fill runs on across rows
              (-3, 1, 5, 2),                      # negative y0: clamped to 0, the height stays
              (1, 1, 0x7FFF, 0x7FFF),             # sizes far outside: clamped to the frame's remainder
              (H - 1, W - 1, 1, 1)]               # 1x1 in the last corner
    if not few:
        boxes += [(2, 1, 0, 3),                   # empty
                  (0, 0, H, W),                   # the full frame
                  (0, 0, 1, 1), (0, W - 1, 1, 1), (H - 1, 0, 1, 1),
                  (H + 2, 0, 3, 3),               # y0 > H: nothing
                  (1, -2, 2, 0x7FFF),             # negative x0 and a width outside
                  (H // 2, W // 3, 2, 3)]
    return boxes, (first is not None, last is not None)


GEOMETRIES = [
    (5, 7, 3, False),      # frame of 105 bytes: every group byte-wise
    (8, 8, 9, False),      # 576 = 36 groups, rows of 72 bytes: groups straddle rows
    (12, 20, 9, False),    # rows of 180 bytes
    (6, 8, 4, False),      # C not a multiple of 3: the colour goes by c % 3 all the same
    (84, 84, 9, True),     # the training geometry, n = 6
]


@pytest.mark.parametrize("H,W,C,few", GEOMETRIES)
def test_kernel_equals_the_restatement(H, W, C, few):
    from curla_amd import ops
    frame = H * W * C
    boxes, (has_first, has_last) = _boxes(H, W, C, few)
    if frame % 16 == 0 and C == 9:
        assert has_first and has_last
    n = len(boxes)
    assert not few or n == 6
    rows_in_ring = n + 3
    rs = np.random.RandomState(H * W + C)
    host = rs.randint(0, 256, (rows_in_ring, H, W, C), dtype=np.uint8)
    store = torch.zeros(rows_in_ring * frame + 32, dtype=torch.uint8, device="cuda")
    ring = store[:rows_in_ring * frame].view(rows_in_ring, H, W, C)
    ring.copy_(torch.from_numpy(host))
    y0 = np.array([b[0] for b in boxes], dtype=np.int32)
    x0 = np.array([b[1] for b in boxes], dtype=np.int32)
    size = np.array([b[2] | (b[3] << 16) for b in boxes], dtype=np.int32)
    rgb = rs.randint(0, 2 ** 31, n).astype(np.int32)  # (a non-zero top byte: ignored)
    rgb[0] = 0x00FF01
    d = [torch.from_numpy(a).cuda() for a in (y0, x0, size, rgb)]
    period = max(1, n - 2)
    rows = rs.randint(0, rows_in_ring, size=period)
    if period > 2:
        rows[-1] = rows[1]  # a repeat
    cases = [(torch.from_numpy(rows.astype(np.int64)).cuda(), period, rows[np.arange(n) % period]),
             (None, n, np.arange(n)),
             (None, period, np.arange(n) % period)]
    for idx, per, src_rows in cases:
        want = torch.from_numpy(cut_nhwc(host[src_rows], y0, x0, size, rgb))
        for lead in (0, 1):  # out on a 16-byte boundary, and one byte off it (no vector path)
            buf = torch.full((GUARD + lead + n * frame + GUARD,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
            out = buf[GUARD + lead:GUARD + lead + n * frame].view(n, H, W, C)
            assert (out.data_ptr() % 16 == 0) == (lead == 0)
            ops.cutout_u8(ring, idx, per, *d, n, out)
            got = buf.cpu()
            assert torch.equal(got[GUARD + lead:GUARD + lead + n * frame].view(n, H, W, C), want), (per, lead)
            assert bool((got[:GUARD + lead] == GUARD_BYTE).all()) and bool((got[GUARD + lead + n * frame:] == GUARD_BYTE).all())
    assert torch.equal(ring.cpu(), torch.from_numpy(host)) and not bool(store[-32:].any())  # the source is only read
    # the colour goes by c % 3 across the stack, and the restatement did paint something
    s = boxes.index((1, 0, 2, W))  # the full-row-width box
    painted = want[s, 1:3].reshape(-1, C)
    for c in range(C):
        assert bool((painted[:, c] == ((int(rgb[s]) >> (8 * (c % 3))) & 0xFF)).all())


def test_kernel_refuses_bad_arguments_before_any_launch():
    from curla_amd import _lib
    lib = _lib.load()
    ring = torch.zeros(4 * 4 * 3 + 32, dtype=torch.uint8, device="cuda")
    w = torch.zeros(8, dtype=torch.int32, device="cuda")
    out = torch.zeros(4 * 4 * 3, dtype=torch.uint8, device="cuda")
    P = w.data_ptr()

    def rc(frames=ring.data_ptr(), period=1, y0=P, x0=P, size=P, rgb=P, n=1, chw=(3, 4, 4), o=out.data_ptr()):
        return lib.curla_cutout_u8(frames, None, period, y0, x0, size, rgb, n, *chw, o, None)
    assert rc(frames=None) == -1 and rc(y0=None) == -1 and rc(o=None) == -1
    assert rc(x0=None) == -1 and rc(size=None) == -1 and rc(rgb=None) == -1
    assert rc(n=0) == -1 and rc(period=0) == -1 and rc(chw=(0, 4, 4)) == -1
    assert rc(size=P + 2) == -1                      # a misaligned size pointer
    assert rc(chw=(3, 2 ** 15, 2 ** 15)) == -3       # H W C = 3 * 2^30: over the 32-bit frame limit
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. buffer routes
MIN_CUT, MAX_CUT = 2, 6


def _filled(in_hw=(12, 12), C=9, capacity=40, B=4, n_fill=30, name="cutout_color", cls=None, **kw):
    import curla_amd
    aug = curla_amd.make_augmentor(name, in_hw, min_cut=MIN_CUT, max_cut=MAX_CUT)
    rb = (cls or curla_amd.ReplayBuffer)((C,) + in_hw, (2,), capacity, B, torch.device("cuda"), aug, **kw)
    ep = _episode(n_fill, C // 3, in_hw, 6)
    rb.add_batch(*ep)
    return rb, ep


def _injected(rb, n_fill, seed):
    """(idxs, offs [12, B]) with a repeated row and boxes drawn by the augmentor from a private seed."""
    B = rb.batch_size
    keep = np.random.get_state()
    np.random.seed(seed)
    idxs = np.random.randint(0, n_fill, size=B)
    idxs[1] = idxs[0]
    offs = np.zeros((12, B), dtype=np.int32)
    for j in range(3):
        y0, x0, bh, bw, rgb = rb.augmentor.draw_boxes(B)
        offs[2 * j], offs[2 * j + 1], offs[6 + 2 * j] = y0, x0, bh | (bw << 16)
        if rgb is not None:
            offs[7 + 2 * j] = rgb[:, 0] | (rgb[:, 1] << 8) | (rgb[:, 2] << 16)
    np.random.set_state(keep)
    return idxs, offs


def _restated(ep, idxs, offs, next_rows=None):
    """(obs | next_obs | pos) as uint8 [3B, H, W, C] through ``RandomCutout.cut`` of the stored (B, C, H, W) stacks."""
    import curla_amd
    next_rows = idxs if next_rows is None else next_rows
    outs = []
    for j, stacks in enumerate((ep[0][idxs], ep[3][next_rows], ep[0][idxs])):
        size, colour = offs[6 + 2 * j], offs[7 + 2 * j]
        rgb = np.stack([colour & 0xFF, (colour >> 8) & 0xFF, (colour >> 16) & 0xFF], 1)
        outs.append(curla_amd.RandomCutout.cut(stacks, offs[2 * j], offs[2 * j + 1], size & 0xFFFF, size >> 16, rgb))
    return np.concatenate(outs).transpose(0, 2, 3, 1)


def _check_refs(rb, sample, want):
    B = rb.batch_size
    obs, _, _, nxt, _, kw = sample
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


@pytest.mark.parametrize("route", ["plain", "dedup", "two_allocations", "n_step"])
@pytest.mark.parametrize("name", ["cutout", "cutout_color"])
def test_buffer_routes_give_the_restated_bytes(route, name):
    """Capacity 40, B = 4, obs 9x12x12, boxes of 2..6 pixels.  (A frame of 9x12x12 bytes puts the second ring on a dword
    at any capacity, so the two-allocation route runs at 3x11x13 and capacity 41.)"""
    kw = dict(dedup_frames=True) if route == "dedup" else dict(n_step=3, discount=0.99) if route == "n_step" else {}
    geo = dict(in_hw=(11, 13), C=3, capacity=41) if route == "two_allocations" else {}
    rb, ep = _filled(name=name, **geo, **kw)
    B, n_fill = rb.batch_size, 30
    if route != "dedup":
        assert (rb._both is None) == (route == "two_allocations")
    assert rb._shift_store.data_ptr() % 256 == 0 and rb._shift_store.stride(0) % 256 == 0
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
    for seed, injected in ((11, True), (12, True), (13, False)):
        if injected:
            idxs, offs = _injected(rb, n_fill, seed)
            sample = rb.sample_cpc_refs((idxs, offs))
        else:  # freshly drawn: the buffer's own draw, re-derived with bare NumPy calls in the stated order
            np.random.seed(seed)
            sample = rb.sample_cpc_refs()
            np.random.seed(seed)
            idxs = np.random.randint(0, n_fill, size=B)
            offs = np.zeros((12, B), dtype=np.int32)
            for j in range(3):
                bh = np.random.randint(MIN_CUT, MAX_CUT + 1, B)
                bw = np.random.randint(MIN_CUT, MAX_CUT + 1, B)
                offs[2 * j] = np.random.randint(0, rb.obs_shape[1] - bh + 1)
                offs[2 * j + 1] = np.random.randint(0, rb.obs_shape[2] - bw + 1)
                offs[6 + 2 * j] = bh | (bw << 16)
                if name == "cutout_color":
                    rgb = np.random.randint(0, 256, (B, 3))
                    offs[7 + 2 * j] = rgb[:, 0] | (rgb[:, 1] << 8) | (rgb[:, 2] << 16)
        assert (name == "cutout_color") == bool(offs[[7, 9, 11]].any())
        last = next_of(idxs)
        if route == "n_step" and seed == 11:
            assert (last != idxs).any()
        want = _restated(ep, idxs, offs, last)
        _check_refs(rb, sample, want)
        assert torch.equal(sample[1].cpu(), torch.from_numpy(ep[1][idxs]))
        assert not bool(rb._shift_store[rb._sample_slot][3 * B * rb._frame:].any())  # the slack is never written
    assert bool((want != _restated(ep, idxs, np.zeros_like(offs), last)).any())  # (the boxes did change pixels)
    # sample_cpc(): the reference contract, float NCHW in [0, 255], the same values
    o, _, _, nx, _, kwargs = rb.sample_cpc((idxs, offs))
    want_f = torch.from_numpy(want.transpose(0, 3, 1, 2).astype(np.float32))
    for t, j in ((o, 0), (nx, 1), (kwargs["obs_pos"], 2)):
        assert t.dtype == torch.float32 and tuple(t.shape) == (B,) + rb.obs_shape
        assert torch.equal(t.cpu(), want_f[j * B:(j + 1) * B])


# ------------------------------------------------------------------------------------------------ 3. a whole update
def _agent(seed, in_hw, C, name="cutout_color"):
    import curla_amd
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    np.random.seed(seed)
    aug = curla_amd.make_augmentor(name, in_hw, min_cut=4, max_cut=12)
    return curla_amd.CurlSacAgent((C,) + in_hw, (2,), torch.device("cuda"), aug, hidden_dim=64, **HP)


def test_an_update_is_the_update_of_the_host_cut_pixels():
    """Steps 0, 1, 2 from a cutout_color buffer with injected draws against the same agent fed frames cut with NumPy
    (handles of the same structure over a host-made ring): the logged losses, the gradient buffers, parameters, targets,
    Adam moments, log_alpha and the device generator end bit-identical."""
    import curla_amd
    B, in_hw, C, n_fill = 32, (40, 44), 9, 200
    aug = curla_amd.make_augmentor("cutout_color", in_hw, min_cut=4, max_cut=12)
    ep = _episode(n_fill, C // 3, in_hw, 6)

    class Injected(curla_amd.ReplayBuffer):
        queue = collections.deque()

        def draw_indices(self):
            return self.queue.popleft()

    rb = Injected((C,) + in_hw, (2,), 256, B, torch.device("cuda"), aug)
    rb.add_batch(*ep)
    draws = [_injected(rb, n_fill, 30 + s) for s in range(3)]
    Injected.queue.extend(draws)
    runs = []
    batches = [(_restated(ep, i, o), ep[1][i], ep[2][i], 1.0 - ep[4][i].astype(np.float32)) for i, o in draws]
    plain = [(_restated(ep, i, np.zeros_like(o)), ep[1][i], ep[2][i], 1.0 - ep[4][i].astype(np.float32)) for i, o in draws]
    for source in (rb, _HostShiftedBuffer(batches, B, in_hw), _HostShiftedBuffer(plain, B, in_hw)):
        agent, L = _agent(5, in_hw, C), NullLogger()
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
@pytest.mark.parametrize("dedup", [False, True], ids=["cutout_color", "cutout_color+dedup"])
def test_graph_replay_is_the_eager_update_bit_for_bit(dedup):
    """The protocol of tests/test_gpu_graph_aug.py: 14 mixed steps with log_interval 5 (0, 5, 10 log and run eagerly;
    1, 2 warm up; 3, 4, 6, 7 capture; 8, 9, 11, 12, 13 replay); the state compared includes NumPy's stream, torch's CPU
    generator and the device generator.  Then ``max_cut`` is edited: the next step is still a replay, and the minibatch
    it left in its graph slot is the host restatement of the new, smaller boxes."""
    import curla_amd.ops as ops_mod
    from curla_amd import _lib
    setup = dict(aug="cutout_color", dedup_frames=dedup)
    eager, calls_e, logs_e, _, _ = _run(False, **setup)
    graph, calls_g, logs_g, agent, rb = _run(True, **setup)
    replayed = [8, 9, 11, 12, 13]
    assert all(calls_e[s].get("curla_cutout_u8") == 1 and calls_e[s].get("curla_sample_stage") == 1 for s in range(14))
    assert all(calls_e[s].get("curla_gather_stacks", 0) == (2 if dedup else 0) for s in range(14))
    assert [sum(calls_g[s].values()) for s in replayed] == [0] * len(replayed), calls_g
    assert all(sum(calls_g[s].values()) > 15 and calls_g[s].get("curla_cutout_u8", 0) >= 1
               for s in (0, 1, 2, 3, 4, 5, 6, 7, 10)), calls_g
    assert len(agent._graphs) == 2 and all(len(r) == 2 and all(g["graph"] is not None for g in r)
                                           for r in agent._graphs.values())
    assert logs_e == logs_g
    for k in eager:
        assert torch.equal(eager[k], graph[k]), k
    assert float(eager["critic_steps"][0]) == 14 and float(eager["actor_steps"][0]) == 7
    B, frame = rb.batch_size, rb._frame

    def guards_intact():
        assert len(rb._graph_blocks) == 4
        for g in rb._graph_blocks.values():
            assert len(g["guards"]) == (4 if dedup else 2)
            for guard in g["guards"]:
                assert guard.numel() >= rb.GUARD and bool((guard == rb.GUARD_BYTE).all())
            assert g["shift_u8"].numel() == 3 * B * frame + 32
            assert bool(g["shift_u8"][:3 * B * frame].any()) and not bool(g["shift_u8"][-32:].any())
    guards_intact()
    # an edit of the augmentor is not baked in: no re-capture, the host writes the new boxes into the block
    graphs_before = {k: [g["graph"] for g in r] for k, r in agent._graphs.items()}
    rb.augmentor.max_cut = 12
    host_calls = []
    real_call = _lib.call
    ops_mod.call = lambda name, *a: (host_calls.append(name), real_call(name, *a))[1]
    before = np.random.get_state()
    try:
        agent.update(rb, NullLogger(), 14)
        torch.cuda.synchronize()
    finally:
        ops_mod.call = real_call
    assert host_calls == [] and {k: [g["graph"] for g in r] for k, r in agent._graphs.items()} == graphs_before
    after = np.random.get_state()
    np.random.set_state(before)
    idxs, offs = rb.draw_indices()  # the draw the replay made
    now = np.random.get_state()
    assert np.array_equal(now[1], after[1]) and now[2] == after[2]
    sizes = offs[[6, 8, 10]]
    assert int((sizes & 0xFFFF).max()) <= 12 and int((sizes >> 16).max()) <= 12 and bool(offs[[7, 9, 11]].any())
    n_stored = rb.idx  # the stored stacks, read back from the buffer itself: (obs, -, -, next_obs) as _restated takes them
    stored = (rb.stacks(0, n_stored, 0), None, None, rb.stacks(0, n_stored, 1))
    want = torch.from_numpy(_restated(stored, idxs, offs).reshape(-1))
    assert sum(torch.equal(g["shift_u8"][:3 * B * frame].cpu(), want) for g in rb._graph_blocks.values()) == 1
    guards_intact()


def test_graph_support_is_that_of_the_shift():
    rb, _ = _filled(in_hw=(11, 13), C=3, capacity=41)
    assert rb._both is None and not rb.graph_supported()
    agent = _agent(1, (40, 44), 9)
    with pytest.raises(ValueError, match="RandomCutout.*both rings in one allocation"):
        agent.enable_update_graphs(rb)
    assert _filled()[0].graph_supported() and _filled(dedup_frames=True)[0].graph_supported()
