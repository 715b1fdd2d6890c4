"""``RandomFlip`` and ``RandomRotate`` on the device: ``curla_dihedral_u8`` against a NumPy restatement of its formula and
clamp rule, the replay buffer's routes (plain ring, frame store, rings in two allocations, n-step, ``sample_cpc``), whole
updates against the updates of frames transformed on the host, and update graphs.  Everything is bit for bit
(``torch.equal``): the kernel only moves bytes and the update downstream of it is the existing uint8-ring update.  The
checks of the routes, updates and graphs are written for any of the three one-word scratch augmentations;
tests/test_gpu_grayscale.py runs them for ``RandomGrayscale``."""
import collections

import numpy as np
import pytest
import torch

from tests.test_gpu_agent import HP, NullLogger
from tests.test_gpu_graph_aug import _episode, _run, _state
from tests.test_gpu_random_shift import _HostShiftedBuffer

pytestmark = pytest.mark.gpu

GUARD, GUARD_BYTE = 256, 0xA5
KERNEL = {"flip": "curla_dihedral_u8", "rotate": "curla_dihedral_u8", "grayscale": "curla_grayscale_u8"}
CLAMPED = ((8, 0), (-1, 7), (0x7FFFFFF5, 5))  # (a word of the block, the code it acts as on a square frame)


def dihedral_nhwc(frames, words):
    """The restatement on uint8 [n, H, W, C], with the kernel's clamp rule: code = word & 7, and & 3 where H != W; with
    (a, b) = (x, y) if code & 4, else (y, x): out[y][x] = in[code & 2 ? H - 1 - a : a][code & 1 ? W - 1 - b : b]."""
    n, H, W, C = frames.shape
    out = np.empty_like(frames)
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for s in range(n):
        code = int(words[s]) & (7 if H == W else 3)
        a, b = (x, y) if code & 4 else (y, x)
        out[s] = frames[s][H - 1 - a if code & 2 else a, W - 1 - b if code & 1 else b]
    return out


GEOMETRIES = [  # (H, W, C)
    (5, 7, 3),        # 105 bytes: no vector path
    (8, 8, 4),        # rows of whole groups
    (8, 8, 9),        # rows of 4.5 groups; pixels straddle groups
    (4, 4, 1),        # a group touches four rows
    (12, 12, 3),      # seven runs in a group: more than are held
    (7, 7, 9),        # square, byte-wise
    (4, 4, 32),       # a pixel spans two groups
    (16, 16, 16),
    (84, 84, 9),      # the training geometry, n = 8 plus the three words
    (90, 160, 9),     # non-square
    (136, 136, 9),    # 166 464 B, more than 160 KiB: no whole-frame LDS staging (bands of 15 rows)
    # beyond the issue's list:
    (2, 24, 9),       # not square, rows of 13.5 groups: the 180 degree turn across row ends
    (132, 132, 255),  # 132 segments of 2 x 255 bytes do not fit 64 KiB of LDS: the direct gather
]


@pytest.mark.parametrize("geo", GEOMETRIES, ids=["%dx%dx%d" % g for g in GEOMETRIES])
def test_kernel_equals_the_restatement(geo):
    """Square frames run all eight codes; others 0..3, and 4..7 as their ``code & 3``; every run holds the words 8, -1 and
    0x7FFFFFF5, which act as 0, 7 and 5.  ``out`` on and one byte off a 16-byte boundary, between guard bytes; rows
    given with a repeat, rows None with period n and with period < n; ring row 0 is the start of its allocation."""
    from curla_amd import ops
    H, W, C = geo
    frame = H * W * C
    words = list(range(8)) + [w for w, _ in CLAMPED]
    n = len(words)
    rows_in_ring = n + 3
    rs = np.random.RandomState(H * W + C)
    host = rs.randint(0, 256, (rows_in_ring, H, W, C), dtype=np.uint8)
    store = torch.zeros(rows_in_ring * frame + 32, dtype=torch.uint8, device="cuda")
    ring = store[:rows_in_ring * frame].view(rows_in_ring, H, W, C)  # ring row 0 = the first bytes of its allocation
    assert ring.data_ptr() == store.data_ptr()
    ring.copy_(torch.from_numpy(host))
    d_words = torch.from_numpy(np.array(words, dtype=np.int64).astype(np.int32)).cuda()
    period = n - 2
    rows = rs.randint(0, rows_in_ring, size=period)
    rows[0] = 0  # ring row 0 is a source: nothing lies in front of it
    rows[-1] = rows[1]  # a repeat
    rows[2] = rows_in_ring - 1  # ... and the last row: only the slack lies behind it
    cases = [(torch.from_numpy(rows.astype(np.int64)).cuda(), period, rows[np.arange(n) % period]),
             (None, n, np.arange(n)),
             (None, period, np.arange(n) % period)]
    for idx, per, src_rows in cases:
        want_np = dihedral_nhwc(host[src_rows], words)
        want = torch.from_numpy(want_np)
        for lead in (0, 1):  # out on a 16-byte boundary, and one byte off it (no vector path)
            buf = torch.full((GUARD + lead + n * frame + GUARD,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
            out = buf[GUARD + lead:GUARD + lead + n * frame].view(n, H, W, C)
            assert (out.data_ptr() % 16 == 0) == (lead == 0)
            ops.dihedral_u8(ring, idx, per, d_words, n, out)
            got = buf.cpu()
            assert torch.equal(got[GUARD + lead:GUARD + lead + n * frame].view(n, H, W, C), want), (per, lead)
            assert bool((got[:GUARD + lead] == GUARD_BYTE).all()) and bool((got[GUARD + lead + n * frame:] == GUARD_BYTE).all())
        # the codes are what the table says, and out-of-range words act as their masked values
        src = host[src_rows]
        assert np.array_equal(want_np[0], src[0]) and np.array_equal(want_np[1], src[1][:, ::-1])
        assert np.array_equal(want_np[2], src[2][::-1]) and np.array_equal(want_np[3], src[3][::-1, ::-1])
        for s in range(4, 8):
            if H == W:
                k = {5: 1, 6: 3}.get(s)
                if k:
                    assert np.array_equal(want_np[s], np.rot90(src[s], k))
                else:
                    assert np.array_equal(want_np[s], dihedral_nhwc(src[s:s + 1], [s & 3])[0].transpose(1, 0, 2))
            else:
                assert np.array_equal(want_np[s], dihedral_nhwc(src[s:s + 1], [s & 3])[0])
        for j, (_, code) in enumerate(CLAMPED):
            assert np.array_equal(want_np[8 + j], dihedral_nhwc(src[8 + j:9 + j], [code])[0])
    assert torch.equal(ring.cpu(), torch.from_numpy(host)) and not bool(store[-32:].any())  # the source is only read


def test_kernel_refuses_bad_arguments_before_any_launch():
    from curla_amd import _lib
    lib = _lib.load()
    ring = torch.zeros(4 * 4 * 3 + 32, dtype=torch.uint8, device="cuda")
    w = torch.zeros(8, dtype=torch.int32, device="cuda")
    out = torch.full((4 * 4 * 3,), 0x5A, dtype=torch.uint8, device="cuda")
    P = w.data_ptr()

    def rc(frames=ring.data_ptr(), idx=None, period=1, code=P, n=1, chw=(3, 4, 4), o=out.data_ptr()):
        return lib.curla_dihedral_u8(frames, idx, period, code, n, *chw, o, None)
    assert rc(o=None) == -1 and rc(frames=None) == -1 and rc(code=None) == -1     # null pointers
    assert rc(code=P + 1) == -1 and rc(code=P + 2) == -1                          # the words off their 4 bytes
    assert rc(idx=P + 4) == -1                                                    # idx off its 8 bytes
    assert rc(n=0) == -1 and rc(period=0) == -1
    assert rc(chw=(0, 4, 4)) == -1 and rc(chw=(3, 0, 4)) == -1 and rc(chw=(3, 4, 0)) == -1
    assert rc(chw=(3, 2 ** 15, 2 ** 15)) == -3      # H W C = 3 * 2^30: over the 31 bits of the byte arithmetic
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all())                # nothing was launched
    ring.fill_(7)
    assert rc() == 0                                # ... and the same arguments, all valid, are taken
    torch.cuda.synchronize()
    assert bool((out == 7).all())


# ------------------------------------------------------------------------------------------------ buffer routes
C9 = 9


def restate(name, aug, stacks, word0):
    """The class's host restatement of a tensor's (n, C, H, W) stacks under the words the block carried."""
    from curla_amd.augmentations import ROT90_CODES
    if name == "flip":
        return aug.flip(stacks, word0)
    if name == "rotate":
        return aug.rotate(stacks, [ROT90_CODES.index(int(c)) for c in word0])
    return aug.grey(stacks, word0)


def bare_draw(name, hw, p, B):
    """One tensor's word 0, re-derived with bare NumPy calls in the order the class states."""
    if name == "rotate":
        turns = np.random.randint(0, 4, B) if hw[0] == hw[1] else 2 * np.random.randint(0, 2, B)
        keep = np.random.rand(B) < p
        return np.array([0, 5, 3, 6])[np.where(keep, turns, 0)]
    return (np.random.rand(B) < p).astype(np.int32)


def _filled(name, hw, p, capacity=40, B=8, n_fill=30, **kw):
    import curla_amd
    aug = curla_amd.make_augmentor(name, hw, p=p)
    rb = curla_amd.ReplayBuffer((C9,) + hw, (2,), capacity, B, torch.device("cuda"), aug, **kw)
    ep = _episode(n_fill, C9 // 3, hw, 6)
    rb.add_batch(*ep)
    return rb, ep


def _injected(rb, n_fill, seed):
    """(idxs, offs [6, B]) with a repeated row and words drawn by the augmentor from a private seed."""
    B = rb.batch_size
    keep = np.random.get_state()
    np.random.seed(seed)
    idxs = np.random.randint(0, n_fill, size=B)
    idxs[1] = idxs[0]
    offs = np.zeros((6, B), dtype=np.int32)
    for j in range(3):
        offs[2 * j], offs[2 * j + 1] = rb.augmentor.draw_index_words(B)
    np.random.set_state(keep)
    return idxs, offs


def _restated(name, aug, stored, idxs, offs, next_rows=None):
    """(obs | next_obs | pos) as uint8 [3B, H, W, C] through the host restatement of the stored (n, C, H, W) stacks
    ``stored`` = (obs stacks, -, -, next_obs stacks)."""
    next_rows = idxs if next_rows is None else next_rows
    outs = [restate(name, aug, stacks, offs[2 * j])
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


def check_buffer_route(name, hw, route, p=0.6):
    """B = 8 at (9,) + hw.  Two draws are injected through ``indices=`` and one is the buffer's own, re-derived with bare
    NumPy calls; each against the host restatement, then ``sample_cpc()``'s float NCHW contract.  Rings in two
    allocations need a frame that is no multiple of 4 bytes (an odd capacity then puts the second ring off a dword)."""
    kw = dict(dedup_frames=True) if route == "dedup" else dict(n_step=3, discount=0.99) if route == "n_step" else {}
    rb, ep = _filled(name, hw, p, capacity=41 if route == "two_allocations" else 40, **kw)
    B, n_fill, aug = rb.batch_size, 30, rb.augmentor
    frame = C9 * hw[0] * hw[1]
    if route != "dedup":
        assert (rb._both is None) == (route == "two_allocations")
    assert rb._frame == frame == rb._scratch_frame() and rb._shift_store.shape[1] >= 3 * B * frame + 32
    stored = (rb.stacks(0, n_fill, 0), None, None, rb.stacks(0, n_fill, 1))
    assert np.array_equal(stored[0], ep[0]) and np.array_equal(stored[3], ep[3])
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
    seen = set()
    for seed, injected in ((11, True), (12, True), (13, False)):
        if injected:
            idxs, offs = _injected(rb, n_fill, seed)
            sample = rb.sample_cpc_refs((idxs, offs))
        else:
            np.random.seed(seed)
            sample = rb.sample_cpc_refs()
            np.random.seed(seed)
            idxs = np.random.randint(0, n_fill, size=B)
            offs = np.zeros((6, B), dtype=np.int32)
            for j in range(3):
                offs[2 * j] = bare_draw(name, hw, p, B)
        seen |= set(offs[[0, 2, 4]].ravel().tolist())
        last = next_of(idxs)
        want = _restated(name, aug, stored, idxs, offs, last)
        _check_refs(rb, sample, want)
        assert torch.equal(sample[1].cpu(), torch.from_numpy(ep[1][idxs]))
        assert not bool(rb._shift_store[rb._sample_slot][3 * B * frame:].any())  # the slack is never written
        assert not offs[[1, 3, 5]].any()
    if name == "rotate":
        assert seen == ({0, 5, 3, 6} if hw[0] == hw[1] else {0, 3})  # every turn occurred, the transposing ones too
    else:
        assert seen == {0, 1}
    assert bool((want != _restated(name, aug, stored, idxs, np.zeros_like(offs), last)).any())  # (the words did matter)
    o, _, _, nx, _, kwargs = rb.sample_cpc((idxs, offs))
    want_f = torch.from_numpy(want.transpose(0, 3, 1, 2).astype(np.float32))
    for t, j in ((o, 0), (nx, 1), (kwargs["obs_pos"], 2)):
        assert t.dtype == torch.float32 and tuple(t.shape) == (B, C9) + hw
        assert torch.equal(t.cpu(), want_f[j * B:(j + 1) * B])


ROUTES = [("flip", (12, 12), r) for r in ("plain", "dedup", "n_step")] + \
         [("flip", (11, 13), r) for r in ("plain", "dedup", "two_allocations", "n_step")] + \
         [("rotate", (12, 12), r) for r in ("plain", "dedup", "n_step")] + [("rotate", (11, 11), "two_allocations")]


@pytest.mark.parametrize("name,hw,route", ROUTES, ids=["%s-%dx%d-%s" % (n, h[0], h[1], r) for n, h, r in ROUTES])
def test_buffer_routes_give_the_restated_bytes(name, hw, route):
    """(A frame of 9 x 12 x 12 bytes is a multiple of 4, so both rings always share an allocation there: the rings in two
    allocations run at (9, 11, 13), and for the rotation, which wants a square frame, at (9, 11, 11).)"""
    check_buffer_route(name, hw, route)


# ------------------------------------------------------------------------------------------------ a whole update
def _agent(name, seed, hw, C, p):
    import curla_amd
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    np.random.seed(seed)
    aug = curla_amd.make_augmentor(name, hw, p=p)
    return curla_amd.CurlSacAgent((C,) + hw, (2,), torch.device("cuda"), aug, hidden_dim=64, **HP)


def check_updates_are_those_of_host_transformed_pixels(name, hw):
    """Steps 0, 1, 2 from a buffer of the augmentation (p = 0.3, B = 32) with injected draws against the same agent fed
    frames transformed with NumPy: the logged losses, the gradient buffers, parameters, targets, Adam moments, log_alpha
    and the device generator end bit-identical -- and differ from a run on the untransformed pixels."""
    import curla_amd
    B, C, n_fill, p = 32, 9, 200, 0.3
    aug = curla_amd.make_augmentor(name, hw, p=p)
    ep = _episode(n_fill, C // 3, hw, 6)

    class Injected(curla_amd.ReplayBuffer):
        queue = collections.deque()

        def draw_indices(self):
            return self.queue.popleft()

    rb = Injected((C,) + hw, (2,), 256, B, torch.device("cuda"), aug)
    rb.add_batch(*ep)
    draws = [_injected(rb, n_fill, 30 + s) for s in range(3)]
    for _, o in draws:  # some samples of every tensor are transformed, and some are not
        assert all(0 < int((o[2 * j] != 0).sum()) < B for j in range(3)) and not o[[1, 3, 5]].any()
    if name == "rotate" and hw[0] == hw[1]:
        assert any(int(c) & 4 for _, o in draws for c in o[[0, 2, 4]].ravel())  # transposing codes among them
    Injected.queue.extend(draws)
    scal = lambda i: (ep[1][i], ep[2][i], 1.0 - ep[4][i].astype(np.float32))  # noqa: E731
    batches = [(_restated(name, aug, ep, i, o),) + scal(i) for i, o in draws]
    plain = [(_restated(name, aug, ep, i, np.zeros_like(o)),) + scal(i) for i, o in draws]
    runs = []
    for source in (rb, _HostShiftedBuffer(batches, B, hw), _HostShiftedBuffer(plain, B, hw)):
        agent, L = _agent(name, 5, hw, C, p), NullLogger()
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
    assert not torch.equal(a["critic"], c["critic"])  # ... and the words did matter


@pytest.mark.parametrize("name,hw", [("rotate", (44, 44)), ("flip", (40, 44))], ids=["rotate", "flip"])
def test_three_updates_are_the_updates_of_the_host_transformed_pixels(name, hw):
    check_updates_are_those_of_host_transformed_pixels(name, hw)


# ------------------------------------------------------------------------------------------------ update graphs
def check_graph_replay_is_eager(name):
    """The protocol of tests/test_gpu_graph_aug.py: 14 mixed steps with log_interval 5 (0, 5, 10 log and run eagerly;
    1, 2 warm up; 3, 4, 6, 7 capture; 8, 9, 11, 12, 13 replay) at (40, 44); the state compared includes NumPy's stream,
    torch's CPU generator and the device generator.  Then one more replayed step: the minibatch it left in its graph slot
    is the host restatement of the draw that was made."""
    import curla_amd.ops as ops_mod
    from curla_amd import _lib
    kernel = KERNEL[name]
    eager, calls_e, logs_e, _, _ = _run(False, aug=name)
    graph, calls_g, logs_g, agent, rb = _run(True, aug=name)
    replayed = [8, 9, 11, 12, 13]
    assert tuple(rb.augmentor.output_shape) == (40, 44) and rb.obs_shape == (9, 40, 44)
    assert all(calls_e[s].get(kernel) == 1 and calls_e[s].get("curla_sample_stage") == 1 for s in range(14))
    assert [sum(calls_g[s].values()) for s in replayed] == [0] * len(replayed), calls_g
    assert all(sum(calls_g[s].values()) > 15 and calls_g[s].get(kernel, 0) >= 1 for s in (0, 1, 2, 3, 4, 5, 6, 7, 10)), calls_g
    assert len(agent._graphs) == 2 and all(len(r) == 2 and all(g["graph"] is not None for g in r)
                                           for r in agent._graphs.values())
    assert logs_e == logs_g
    for k in eager:
        assert torch.equal(eager[k], graph[k]), k
    assert float(eager["critic_steps"][0]) == 14 and float(eager["actor_steps"][0]) == 7
    B, frame = rb.batch_size, 9 * 40 * 44

    def guards_intact():
        assert len(rb._graph_blocks) == 4
        for g in rb._graph_blocks.values():
            assert len(g["guards"]) == 2
            for guard in g["guards"]:
                assert guard.numel() >= rb.GUARD and bool((guard == rb.GUARD_BYTE).all())
            assert g["shift_u8"].numel() == 3 * B * frame + 32
            assert bool(g["shift_u8"][:3 * B * frame].any()) and not bool(g["shift_u8"][-32:].any())
    guards_intact()
    host_calls = []
    real_call = _lib.call
    ops_mod.call = lambda name_, *a: (host_calls.append(name_), real_call(name_, *a))[1]
    before = np.random.get_state()
    try:
        agent.update(rb, NullLogger(), 14)
        torch.cuda.synchronize()
    finally:
        ops_mod.call = real_call
    assert host_calls == []
    after = np.random.get_state()
    np.random.set_state(before)
    idxs, offs = rb.draw_indices()  # the draw the replay made
    now = np.random.get_state()
    assert np.array_equal(now[1], after[1]) and now[2] == after[2]
    assert offs.shape == (6, B) and bool(offs[[0, 2, 4]].any()) and not offs[[1, 3, 5]].any()
    n_stored = rb.idx
    stored = (rb.stacks(0, n_stored, 0), None, None, rb.stacks(0, n_stored, 1))
    want = torch.from_numpy(_restated(name, rb.augmentor, stored, idxs, offs).reshape(-1))
    assert sum(torch.equal(g["shift_u8"][:3 * B * frame].cpu(), want) for g in rb._graph_blocks.values()) == 1
    guards_intact()


@pytest.mark.parametrize("name", ["flip", "rotate"])
def test_graph_replay_is_the_eager_update_bit_for_bit(name):
    """(At (40, 44) the rotation draws 0 and 180 degrees; the transposing codes are covered by the kernel, route and
    update tests above.)"""
    check_graph_replay_is_eager(name)
