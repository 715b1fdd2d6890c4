"""``RandomTranslate`` on the device: ``curla_translate_u8`` against a NumPy restatement of its clamp-and-place rule, the
replay buffer's routes (plain ring, frame store, rings in two allocations, n-step, ``sample_cpc``), a whole update against
the update of frames translated on the host, update graphs and batched acting.  Everything is bit for bit
(``torch.equal``): the kernel only moves bytes and the update downstream of it is the existing uint8-ring update, on
frames of the canvas size."""
import collections

import numpy as np
import pytest
import torch

from tests.test_gpu_agent import HP, NullLogger
from tests.test_gpu_graph_aug import _episode, _run, _state
from tests.test_gpu_random_shift import _HostShiftedBuffer

pytestmark = pytest.mark.gpu

GUARD, GUARD_BYTE = 256, 0xA5


def translate_nhwc(frames, ty, tx, Ho, Wo):
    """The restatement on uint8 [n, H, W, C] -> [n, Ho, Wo, C], with the kernel's clamp rule: tyc = clamp(ty, 0, Ho - H),
    txc = clamp(tx, 0, Wo - W)."""
    n, H, W, C = frames.shape
    out = np.zeros((n, Ho, Wo, C), dtype=np.uint8)
    for s in range(n):
        yc, xc = min(max(int(ty[s]), 0), Ho - H), min(max(int(tx[s]), 0), Wo - W)
        out[s, yc:yc + H, xc:xc + W] = frames[s]
    return out


def _edge_tx(H, W, C, Ho, Wo):
    """(ty, tx) for which the image's first byte in some output row is the LAST byte of a 16-byte group of the output
    frame, and one for which it is a group's FIRST byte (tx > 0 where there is one); None where the geometry has none."""
    orb, last, first = Wo * C, None, None
    for tx in list(range(1, Wo - W + 1)) + [0]:
        for ty in range(Ho - H + 1):
            at = {((y * orb) + tx * C) % 16 for y in range(ty, ty + H)}
            if last is None and 15 in at:
                last = (ty, tx)
            if first is None and 0 in at:
                first = (ty, tx)
    return last, first


def _offsets(H, W, C, Ho, Wo, few):
    my, mx = Ho - H, Wo - W
    last, first = _edge_tx(H, W, C, Ho, Wo)
    inner = (my // 2, mx // 2)
    if few:  # six samples: the edge offset takes the interior pair's place where it is one
        if last is not None and 0 < last[1] < mx:
            inner = (my // 2, last[1])
        offs = [(0, 0), (my, mx), (0, mx), (my, 0), inner, (-3, 0x7FFF)]
    else:
        offs = [(0, 0), (my, mx), (0, mx), (my, 0), inner, (-3, 0x7FFF), (0x7FFF, -3), (-1, -1), (my + 1, mx + 1)]
        offs += [o for o in (last, first) if o is not None]
    return offs, (last is not None, first is not None)


GEOMETRIES = [  # (H, W, C), (Ho, Wo), few
    ((5, 7, 3), (8, 9), False),        # output frame of 216 bytes: 13.5 groups, so no vector path
    ((8, 8, 4), (12, 12), False),      # 576 bytes, rows of 48 bytes: whole groups per row
    ((8, 8, 9), (12, 10), False),      # rows of 90 bytes: groups straddle rows and image edges
    ((6, 8, 1), (6, 16), False),       # C = 1, Ho == H, horizontal margin only
    ((7, 5, 9), (7, 5), False),        # no margin at all: a plain gather
    ((84, 84, 9), (92, 92), True),     # the training geometry, n = 6
    # beyond the issue's list, the vector path's remaining branches:
    ((8, 8, 9), (12, 12), False),      # 1296 bytes = 81 groups, rows of 108 bytes: vector groups straddle rows and edges
    ((3, 7, 3), (16, 7), False),       # 336 bytes = 21 groups, Wo == W: the runs of two rows are one run of the source
    ((6, 3, 1), (8, 6), False),        # rows of 6 bytes: a group touches three rows
    ((1, 5, 3), (4, 4 * 3), False),    # a source frame of 15 bytes: shorter than a group, byte-wise
]


@pytest.mark.parametrize("geo,out_hw,few", GEOMETRIES,
                         ids=["%dx%dx%d-%dx%d" % (g + o) for g, o, _ in GEOMETRIES])
def test_kernel_equals_the_restatement(geo, out_hw, few):
    from curla_amd import ops
    (H, W, C), (Ho, Wo) = geo, out_hw
    frame, oframe = H * W * C, Ho * Wo * C
    offs, (has_last, has_first) = _offsets(H, W, C, Ho, Wo, few)
    n = len(offs)
    assert not few or n == 6
    if (H, W, C) == (84, 84, 9):  # rows of 51.75 groups: both edge positions occur, among the six samples too
        assert has_last and has_first
        at = {(y * Wo * C + tx * C) % 16 for ty, tx in offs[:5] for y in range(ty, ty + H)}
        assert {0, 15} <= at
    rows_in_ring = n + 3
    rs = np.random.RandomState(H * W + C + Wo)
    host = rs.randint(1, 256, (rows_in_ring, H, W, C), dtype=np.uint8)  # (no zero byte: a margin byte is told from a pixel)
    store = torch.zeros(rows_in_ring * frame + 32, dtype=torch.uint8, device="cuda")
    ring = store[:rows_in_ring * frame].view(rows_in_ring, H, W, C)  # ring row 0 = the first bytes of its allocation
    assert ring.data_ptr() == store.data_ptr()
    ring.copy_(torch.from_numpy(host))
    ty = np.array([o[0] for o in offs], dtype=np.int32)
    tx = np.array([o[1] for o in offs], dtype=np.int32)
    d_ty, d_tx = torch.from_numpy(ty).cuda(), torch.from_numpy(tx).cuda()
    period = max(1, n - 2)
    rows = rs.randint(0, rows_in_ring, size=period)
    rows[0] = 0  # ring row 0 is a source: nothing lies in front of it
    if period > 2:
        rows[-1] = rows[1]  # a repeat
    cases = [(torch.from_numpy(rows.astype(np.int64)).cuda(), period, rows[np.arange(n) % period]),
             (None, n, np.arange(n)),
             (None, period, np.arange(n) % period)]
    for idx, per, src_rows in cases:
        want = torch.from_numpy(translate_nhwc(host[src_rows], ty, tx, Ho, Wo))
        for lead in (0, 1):  # out on a 16-byte boundary, and one byte off it (no vector path)
            buf = torch.full((GUARD + lead + n * oframe + GUARD,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
            out = buf[GUARD + lead:GUARD + lead + n * oframe].view(n, Ho, Wo, C)
            assert (out.data_ptr() % 16 == 0) == (lead == 0)
            ops.translate_u8(ring, idx, per, d_ty, d_tx, n, out)
            got = buf.cpu()
            assert torch.equal(got[GUARD + lead:GUARD + lead + n * oframe].view(n, Ho, Wo, C), want), (per, lead)
            assert bool((got[:GUARD + lead] == GUARD_BYTE).all()) and bool((got[GUARD + lead + n * oframe:] == GUARD_BYTE).all())
    assert torch.equal(ring.cpu(), torch.from_numpy(host)) and not bool(store[-32:].any())  # the source is only read
    # every sample keeps all its pixels and sets nothing else; out-of-range offsets act as their clamped values
    assert all(int((want[s] != 0).sum()) == frame for s in range(n))
    assert torch.equal(want[5], torch.from_numpy(translate_nhwc(host[src_rows[5:6]], [0], [Wo - W], Ho, Wo))[0])


def test_kernel_refuses_bad_arguments_before_any_launch():
    from curla_amd import _lib
    lib = _lib.load()
    ring = torch.zeros(4 * 4 * 3 + 32, dtype=torch.uint8, device="cuda")
    w = torch.zeros(8, dtype=torch.int32, device="cuda")
    out = torch.full((6 * 6 * 3,), 0x5A, dtype=torch.uint8, device="cuda")
    P = w.data_ptr()

    def rc(frames=ring.data_ptr(), idx=None, period=1, ty=P, tx=P, n=1, chw=(3, 4, 4), hw=(6, 6), o=out.data_ptr()):
        return lib.curla_translate_u8(frames, idx, period, ty, tx, n, *chw, *hw, o, None)
    assert rc(o=None) == -1 and rc(frames=None) == -1 and rc(ty=None) == -1 and rc(tx=None) == -1   # null pointers
    assert rc(ty=P + 1) == -1 and rc(ty=P + 2) == -1 and rc(tx=P + 2) == -1                         # odd offset pointers
    assert rc(idx=P + 4) == -1                                                                      # idx off its 8 bytes
    assert rc(hw=(3, 6)) == -1 and rc(hw=(6, 3)) == -1                                              # Ho < H, Wo < W
    assert rc(n=0) == -1 and rc(period=0) == -1 and rc(chw=(0, 4, 4)) == -1 and rc(chw=(3, 0, 4)) == -1
    assert rc(hw=(2 ** 15, 2 ** 15)) == -3      # Ho Wo C = 3 * 2^30: over the 31 bits of the byte arithmetic
    assert rc(chw=(1, 1, 4), hw=(1, 2 ** 30)) == -3   # one output row of 2^30 bytes: twice a row is over 31 bits
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all())            # nothing was launched
    assert rc() == 0                            # ... and the same arguments, all valid, are taken
    torch.cuda.synchronize()
    assert not bool((out == 0x5A).any())


# ------------------------------------------------------------------------------------------------ 3. buffer routes
IN_HW, OUT_HW, C9 = (11, 13), (15, 16), 9


def _filled(in_hw=IN_HW, out_hw=OUT_HW, C=C9, capacity=40, B=8, n_fill=30, cls=None, **kw):
    import curla_amd
    aug = curla_amd.make_augmentor("translate", in_hw, out_hw)
    rb = (cls or curla_amd.ReplayBuffer)((C,) + in_hw, (2,), capacity, B, torch.device("cuda"), aug, **kw)
    ep = _episode(n_fill, C // 3, in_hw, 6)
    rb.add_batch(*ep)
    return rb, ep


def _injected(rb, n_fill, seed):
    """(idxs, offs [6, B]) with a repeated row and offsets drawn by the augmentor from a private seed."""
    B = rb.batch_size
    keep = np.random.get_state()
    np.random.seed(seed)
    idxs = np.random.randint(0, n_fill, size=B)
    idxs[1] = idxs[0]
    offs = np.zeros((6, B), dtype=np.int32)
    for j in range(3):
        offs[2 * j], offs[2 * j + 1] = rb.augmentor.draw_offsets(B)
    np.random.set_state(keep)
    return idxs, offs


def _restated(aug, stored, idxs, offs, next_rows=None):
    """(obs | next_obs | pos) as uint8 [3B, Ho, Wo, C] through ``RandomTranslate.translate`` of the stored (n, C, H, W)
    stacks ``stored`` = (obs stacks, -, -, next_obs stacks)."""
    next_rows = idxs if next_rows is None else next_rows
    outs = [aug.translate(stacks, offs[2 * j], offs[2 * j + 1])
            for j, stacks in enumerate((stored[0][idxs], stored[3][next_rows], stored[0][idxs]))]
    return np.ascontiguousarray(np.concatenate(outs).transpose(0, 2, 3, 1))


def _check_refs(rb, sample, want):
    B = rb.batch_size
    obs, _, _, nxt, _, kw = sample
    scratch = obs.src
    assert scratch.dtype == torch.uint8 and tuple(scratch.shape) == tuple(want.shape)
    assert torch.equal(scratch.cpu(), torch.from_numpy(want))
    for ref, row0 in ((obs, 0), (nxt, B), (kw["obs_pos"], 2 * B)):
        assert ref.src.data_ptr() == scratch.data_ptr() and ref.is_u8 == 1 and ref.B == B
        assert ref.idx.tolist() == list(range(row0, row0 + B)) and not bool(ref.h1.any()) and not bool(ref.w1.any())
        assert (ref.Hc, ref.Wc) == (ref.Hs, ref.Ws) == tuple(rb.augmentor.output_shape)
        ref.check()
    pair, second = obs.pair
    assert second is nxt and pair.B == 2 * B and pair.idx.tolist() == list(range(2 * B)) and not bool(pair.h1.any())


@pytest.mark.parametrize("route", ["plain", "dedup", "two_allocations", "n_step"])
def test_buffer_routes_give_the_restated_bytes(route):
    """(C, H, W) = (9, 11, 13) -> (15, 16), B = 8.  (A frame of 1287 bytes: capacity 40 puts the second ring on a dword,
    capacity 41 does not.)  Two draws are injected through ``indices=`` -- the way a data-parallel rank hands in its shard
    of a draw: no route treats them specially -- and one is the buffer's own."""
    kw = dict(dedup_frames=True) if route == "dedup" else dict(n_step=3, discount=0.99) if route == "n_step" else {}
    rb, ep = _filled(capacity=41 if route == "two_allocations" else 40, **kw)
    B, n_fill, aug = rb.batch_size, 30, rb.augmentor
    oframe = C9 * OUT_HW[0] * OUT_HW[1]
    if route != "dedup":
        assert (rb._both is None) == (route == "two_allocations")
    assert rb._frame == C9 * IN_HW[0] * IN_HW[1] and rb._scratch_frame() == oframe and oframe % 16 == 0
    assert rb._shift_store.data_ptr() % 256 == 0 and rb._shift_store.stride(0) % 256 == 0
    assert rb._shift_store.shape[1] >= 3 * B * oframe + 32
    stored = (rb.stacks(0, n_fill, 0), None, None, rb.stacks(0, n_fill, 1))
    assert np.array_equal(stored[0], ep[0]) and np.array_equal(stored[3], ep[3])  # the stored frames stay (C, H, W)
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
            offs = np.zeros((6, B), dtype=np.int32)
            for j in range(3):
                offs[2 * j] = np.random.randint(0, OUT_HW[0] - IN_HW[0] + 1, B)
                offs[2 * j + 1] = np.random.randint(0, OUT_HW[1] - IN_HW[1] + 1, B)
        last = next_of(idxs)
        if route == "n_step" and seed == 11:
            assert (last != idxs).any()
        want = _restated(aug, stored, idxs, offs, last)
        _check_refs(rb, sample, want)
        assert torch.equal(sample[1].cpu(), torch.from_numpy(ep[1][idxs]))
        assert not bool(rb._shift_store[rb._sample_slot][3 * B * oframe:].any())  # the slack is never written
    assert bool((want != _restated(aug, stored, idxs, np.zeros_like(offs), last)).any())  # (the offsets did move pixels)
    # sample_cpc(): the reference contract, float NCHW in [0, 255] of the canvas size, the same values
    o, _, _, nx, _, kwargs = rb.sample_cpc((idxs, offs))
    want_f = torch.from_numpy(want.transpose(0, 3, 1, 2).astype(np.float32))
    for t, j in ((o, 0), (nx, 1), (kwargs["obs_pos"], 2)):
        assert t.dtype == torch.float32 and tuple(t.shape) == (B, C9) + OUT_HW
        assert torch.equal(t.cpu(), want_f[j * B:(j + 1) * B])


# ------------------------------------------------------------------------------------------------ 4. a whole update
def _agent(seed, in_hw, out_hw, C):
    import curla_amd
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    np.random.seed(seed)
    aug = curla_amd.make_augmentor("translate", in_hw, out_hw)
    return curla_amd.CurlSacAgent((C,) + out_hw, (2,), torch.device("cuda"), aug, hidden_dim=64, **HP)


def test_an_update_is_the_update_of_the_host_translated_pixels():
    """Steps 0, 1, 2 from a translate buffer with injected draws against the same agent fed frames translated with NumPy
    (handles of the same structure over a host-made ring of canvas-sized frames): the logged losses, the gradient
    buffers, parameters, targets, Adam moments, log_alpha and the device generator end bit-identical -- and differ from
    a run on the untranslated pixels padded to the same size at offset (0, 0)."""
    import curla_amd
    B, in_hw, out_hw, C, n_fill = 32, (40, 44), (46, 52), 9, 200
    aug = curla_amd.make_augmentor("translate", in_hw, out_hw)
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
    scal = lambda i: (ep[1][i], ep[2][i], 1.0 - ep[4][i].astype(np.float32))  # noqa: E731
    batches = [(_restated(aug, ep, i, o),) + scal(i) for i, o in draws]
    plain = [(_restated(aug, ep, i, np.zeros_like(o)),) + scal(i) for i, o in draws]
    for source in (rb, _HostShiftedBuffer(batches, B, out_hw), _HostShiftedBuffer(plain, B, out_hw)):
        agent, L = _agent(5, in_hw, out_hw, C), NullLogger()
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
    assert not torch.equal(a["critic"], c["critic"])  # ... and the offsets did matter


# ------------------------------------------------------------------------------------------------ 5. update graphs
@pytest.mark.parametrize("dedup", [False, True], ids=["translate", "translate+dedup"])
def test_graph_replay_is_the_eager_update_bit_for_bit(dedup):
    """The protocol of tests/test_gpu_graph_aug.py: 14 mixed steps with log_interval 5 (0, 5, 10 log and run eagerly;
    1, 2 warm up; 3, 4, 6, 7 capture; 8, 9, 11, 12, 13 replay) at (40, 44) -> (48, 52); the state compared includes
    NumPy's stream, torch's CPU generator and the device generator.  Then one more replayed step: the minibatch it left
    in its graph slot is the host restatement of the draw that was made."""
    import curla_amd.ops as ops_mod
    from curla_amd import _lib
    setup = dict(aug="translate", dedup_frames=dedup)
    eager, calls_e, logs_e, _, _ = _run(False, **setup)
    graph, calls_g, logs_g, agent, rb = _run(True, **setup)
    replayed = [8, 9, 11, 12, 13]
    assert tuple(rb.augmentor.output_shape) == (48, 52) and rb.obs_shape == (9, 40, 44)
    assert all(calls_e[s].get("curla_translate_u8") == 1 and calls_e[s].get("curla_sample_stage") == 1 for s in range(14))
    assert all(calls_e[s].get("curla_gather_stacks", 0) == (2 if dedup else 0) for s in range(14))
    assert all(calls_e[s].get("curla_random_shift_u8", 0) == 0 and calls_e[s].get("curla_cutout_u8", 0) == 0 for s in range(14))
    assert [sum(calls_g[s].values()) for s in replayed] == [0] * len(replayed), calls_g
    assert all(sum(calls_g[s].values()) > 15 and calls_g[s].get("curla_translate_u8", 0) >= 1
               for s in (0, 1, 2, 3, 4, 5, 6, 7, 10)), calls_g
    assert len(agent._graphs) == 2 and all(len(r) == 2 and all(g["graph"] is not None for g in r)
                                           for r in agent._graphs.values())
    assert logs_e == logs_g
    for k in eager:
        assert torch.equal(eager[k], graph[k]), k
    assert float(eager["critic_steps"][0]) == 14 and float(eager["actor_steps"][0]) == 7
    B, oframe = rb.batch_size, 9 * 48 * 52

    def guards_intact():
        assert len(rb._graph_blocks) == 4
        for g in rb._graph_blocks.values():
            assert len(g["guards"]) == (4 if dedup else 2)
            for guard in g["guards"]:
                assert guard.numel() >= rb.GUARD and bool((guard == rb.GUARD_BYTE).all())
            assert g["shift_u8"].numel() == 3 * B * oframe + 32
            assert bool(g["shift_u8"][:3 * B * oframe].any()) and not bool(g["shift_u8"][-32:].any())
            if dedup:
                assert g["mb_u8"].numel() == 2 * B * rb._frame + 32 and not bool(g["mb_u8"][-32:].any())
    guards_intact()
    graphs_before = {k: [g["graph"] for g in r] for k, r in agent._graphs.items()}
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
    assert offs.shape == (6, B) and offs.min() >= 0 and offs.max() <= 8 and bool(offs.any())
    n_stored = rb.idx
    stored = (rb.stacks(0, n_stored, 0), None, None, rb.stacks(0, n_stored, 1))
    want = torch.from_numpy(_restated(rb.augmentor, stored, idxs, offs).reshape(-1))
    assert sum(torch.equal(g["shift_u8"][:3 * B * oframe].cpu(), want) for g in rb._graph_blocks.values()) == 1
    guards_intact()


def test_graph_support_is_that_of_the_shift():
    rb, _ = _filled(capacity=41)
    assert rb._both is None and not rb.graph_supported()
    agent = _agent(1, (40, 44), (48, 52), 9)
    with pytest.raises(ValueError, match="RandomTranslate.*both rings in one allocation"):
        agent.enable_update_graphs(rb)
    assert _filled()[0].graph_supported() and _filled(dedup_frames=True)[0].graph_supported()


# ------------------------------------------------------------------------------------------------ 6. batched acting
def test_batched_acting_centres_frames_of_the_input_size():
    """select_actions / sample_actions on N = 3 frames of ``input_shape`` equal the calls on their
    ``evaluation_augmentation``, bit for bit, over the input routes; a frame of a third size raises with both sizes."""
    in_hw, out_hw, C = (40, 44), (47, 52), 9  # (an odd margin: the centring floors)
    agent = _agent(3, in_hw, out_hw, C)
    frames = np.random.RandomState(8).randint(0, 256, (3, C) + in_hw, dtype=np.uint8)
    centred = np.stack([agent.augmentor.evaluation_augmentation(f) for f in frames])
    assert centred.shape == (3, C) + out_hw and np.array_equal(centred[:, :, 3:43, 4:48], frames)
    want = agent.select_actions(centred)
    assert want.shape == (3, 2) and np.isfinite(want).all()
    routes = (lambda a: a, list, lambda a: torch.from_numpy(a).cuda(), lambda a: a.astype(np.float32))
    for route in routes:  # uint8 array, sequence of frames, uint8 device tensor, the float route: each against itself
        assert np.array_equal(agent.select_actions(route(frames)), agent.select_actions(route(centred)))
    assert np.array_equal(agent.select_actions(frames), want)
    assert torch.equal(agent.select_actions(frames, as_tensor=True).cpu(), torch.from_numpy(want))
    noise = torch.randn(3, 2, generator=torch.Generator().manual_seed(2))
    assert np.array_equal(agent.sample_actions(frames, noise=noise), agent.sample_actions(centred, noise=noise))
    with pytest.raises(ValueError) as e:
        agent.select_actions(np.zeros((3, C, 42, 44), np.uint8))
    assert str(out_hw) in str(e.value) and str(in_hw) in str(e.value)
    assert not np.array_equal(want, agent.select_actions(np.ascontiguousarray(centred[:, :, ::-1])))  # (pixels matter)
    # margins of 0 and 1: the frame lands at (0, 0) of a larger canvas; it is centred like any other, on every route
    for tight_hw in ((41, 44), (40, 45), (41, 45)):
        tight = _agent(3, in_hw, tight_hw, C)
        placed = np.stack([tight.augmentor.evaluation_augmentation(f) for f in frames])
        assert placed.shape == (3, C) + tight_hw and np.array_equal(placed[:, :, :40, :44], frames)
        for route in routes:
            assert np.array_equal(tight.select_actions(route(frames)), tight.select_actions(route(placed)))
