"""``RandomAffine`` on the device: ``curla_affine_u8`` against the restatement of tests/_affine_ref.py (written from the
formula, independently of ``RandomAffine.warp``), its refusals, the replay buffer's routes (plain ring, frame store, rings
in two allocations, n-step, temporal positives, vectorised environments; ``sample_cpc``), whole updates against the updates
of frames warped on the host, and update graphs.  Everything is bit for bit (``torch.equal``): the map is defined in
integers, and the update downstream of the kernel is the existing uint8-ring update."""
import collections

import numpy as np
import pytest
import torch

from tests._affine_ref import IDENTITY, affine_nhwc, kernel_word_sets
from tests.test_gpu_agent import HP, NullLogger
from tests.test_gpu_graph_aug import _episode, _run, _state
from tests.test_gpu_random_shift import _HostShiftedBuffer

pytestmark = pytest.mark.gpu

GUARD, GUARD_BYTE = 256, 0xA5
KERNEL = "curla_affine_u8"

GEOMETRIES = [  # (H, W, C)
    (5, 7, 3),        # 105 bytes: no vector path
    (8, 8, 4),        # rows of whole groups
    (8, 8, 9),        # rows of 4.5 groups; pixels straddle groups
    (4, 4, 1),        # a group touches four rows
    (7, 7, 9),        # square, byte-wise
    (4, 4, 32),       # a pixel spans two groups
    (16, 16, 16),
    (2, 24, 9),
    (84, 84, 9),      # the training geometry: four bands per sample, the last one short
    (90, 160, 9),     # non-square; under 45 degrees no band's box fits the LDS (the direct gather)
    (136, 136, 9),    # 166 464 B, more than the LDS; under 20 degrees a band is narrowed until its box fits
]


@pytest.fixture(scope="module")
def references():
    """The restatement of every (geometry, fill, rows) the kernel test asks for, computed once."""
    cache = {}

    def get(geo, fill, host, src_rows, words):
        key = (geo, fill, tuple(int(r) for r in src_rows))
        if key not in cache:
            cache[key] = affine_nhwc(host[src_rows], words, fill)
        return cache[key]
    return get


@pytest.mark.parametrize("geo", GEOMETRIES, ids=["%dx%dx%d" % g for g in GEOMETRIES])
def test_kernel_equals_the_restatement(geo, references):
    """One sample per word set of tests/_affine_ref.py (identity, the exact turns, shifts inside and out of the frame,
    half a pixel, a small and a large angle with zoom, minification, magnification, garbage), both fills.  ``out`` on and
    one byte off a 16-byte boundary, between guard bytes; rows given with a repeat, rows None with period n and with
    period < n; ring row 0 is the start of its allocation and the last row has only the slack behind it."""
    from curla_amd import ops
    H, W, C = geo
    frame = H * W * C
    sets = kernel_word_sets(H, W)
    words = [w for _, w in sets]
    n = len(words)
    rows_in_ring = n + 3
    rs = np.random.RandomState(H * W + C)
    host = rs.randint(0, 256, (rows_in_ring, H, W, C), dtype=np.uint8)
    store = torch.zeros(rows_in_ring * frame + 32, dtype=torch.uint8, device="cuda")
    ring = store[:rows_in_ring * frame].view(rows_in_ring, H, W, C)  # ring row 0 = the first bytes of its allocation
    assert ring.data_ptr() == store.data_ptr()
    ring.copy_(torch.from_numpy(host))
    d_words = [torch.from_numpy(np.array([w[k] for w in words], dtype=np.int64).astype(np.int32)).cuda() for k in range(6)]
    period = n - 2
    rows = rs.randint(0, rows_in_ring, size=period)
    rows[0] = 0  # ring row 0 is a source: nothing lies in front of it
    rows[-1] = rows[1]  # a repeat
    rows[2] = rows_in_ring - 1  # ... and the last row: only the slack lies behind it
    cases = [(torch.from_numpy(rows.astype(np.int64)).cuda(), period, rows[np.arange(n) % period]),
             (None, n, np.arange(n)),
             (None, period, np.arange(n) % period)]
    for fill in (1, 0):
        for idx, per, src_rows in cases:
            want_np = references(geo, fill, host, src_rows, words)
            want = torch.from_numpy(want_np)
            for lead in (0, 1):  # out on a 16-byte boundary, and one byte off it (no vector path)
                buf = torch.full((GUARD + lead + n * frame + GUARD,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
                out = buf[GUARD + lead:GUARD + lead + n * frame].view(n, H, W, C)
                assert (out.data_ptr() % 16 == 0) == (lead == 0)
                ops.affine_u8(ring, idx, per, d_words, fill, n, out)
                got = buf.cpu()
                got_frames = got[GUARD + lead:GUARD + lead + n * frame].view(n, H, W, C)
                for s in range(n):
                    assert torch.equal(got_frames[s], want[s]), (sets[s][0], fill, per, lead)
                assert bool((got[:GUARD + lead] == GUARD_BYTE).all()) and bool((got[GUARD + lead + n * frame:] == GUARD_BYTE).all())
            # the word sets are what their names say
            src = host[src_rows]
            assert np.array_equal(want_np[0], src[0]) and np.array_equal(want_np[1], src[1][::-1, ::-1])
            if H == W:
                assert np.array_equal(want_np[2], np.rot90(src[2], 1)) and np.array_equal(want_np[3], np.rot90(src[3], 3))
            inside = want_np[4][1:, :W - 1]
            assert np.array_equal(inside, src[4][:H - 1, 1:])
            pure = np.broadcast_to(src[5][0, W - 1], (H, W, C)) if fill else np.zeros((H, W, C), np.uint8)
            assert np.array_equal(want_np[5], pure)
    assert torch.equal(ring.cpu(), torch.from_numpy(host)) and not bool(store[-32:].any())  # the source is only read


def test_kernel_refuses_bad_arguments_before_any_launch():
    from curla_amd import _lib
    lib = _lib.load()
    ring = torch.zeros(4 * 4 * 3 + 32, dtype=torch.uint8, device="cuda")
    w = torch.zeros(8, dtype=torch.int32, device="cuda")
    one = torch.full((8,), 65536, dtype=torch.int32, device="cuda")
    out = torch.full((4 * 4 * 3,), 0x5A, dtype=torch.uint8, device="cuda")
    Z, P = w.data_ptr(), one.data_ptr()
    ident = [P, Z, Z, Z, P, Z]

    def rc(frames=ring.data_ptr(), idx=None, period=1, m=ident, fill=1, n=1, chw=(3, 4, 4), o=out.data_ptr()):
        return lib.curla_affine_u8(frames, idx, period, *m, fill, n, *chw, o, None)
    assert rc(o=None) == -1 and rc(frames=None) == -1                             # null pointers
    for k in range(6):
        assert rc(m=ident[:k] + [None] + ident[k + 1:]) == -1
        assert rc(m=ident[:k] + [ident[k] + 1] + ident[k + 1:]) == -1             # a word array off its 4 bytes
        assert rc(m=ident[:k] + [ident[k] + 2] + ident[k + 1:]) == -1
    assert rc(idx=Z + 4) == -1                                                    # idx off its 8 bytes
    assert rc(n=0) == -1 and rc(period=0) == -1 and rc(n=-1) == -1
    assert rc(chw=(0, 4, 4)) == -1 and rc(chw=(3, 0, 4)) == -1 and rc(chw=(3, 4, 0)) == -1
    assert rc(fill=2) == -1 and rc(fill=-1) == -1
    assert rc(chw=(3, 2 ** 15, 2 ** 15)) == -3      # H W C = 3 * 2^30: over the 31 bits of the byte arithmetic
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all())                # nothing was launched
    ring.fill_(7)
    assert rc() == 0 and rc(fill=0) == 0            # ... and the same arguments, all valid, are taken
    torch.cuda.synchronize()
    assert bool((out == 7).all())


# ------------------------------------------------------------------------------------------------ buffer routes
C9, N_FILL = 9, 30
AUG_KW = dict(degrees=30.0, scale=(0.7, 1.4), translate=0.1, p=0.8)  # strong enough that every sample visibly moves
ROUTES = {
    "plain": ((12, 12), 40, dict()),
    "plain-40x44": ((40, 44), 40, dict()),
    "dedup": ((12, 12), 40, dict(dedup_frames=True)),
    "two_allocations": ((11, 13), 41, dict()),  # a frame of 1287 bytes in an odd capacity: the second ring off a dword
    "n_step": ((12, 12), 40, dict(n_step=3, discount=0.99)),
    "pos_offset": ((12, 12), 40, dict(pos_offset=2)),
    "n_envs": ((12, 12), 40, dict(n_envs=2, n_step=3, discount=0.99)),
}


def _words_of_tensor(offs, j):
    """[6][B]: word r of tensor j sits in row 6 (r // 2) + 2 j + r % 2 of the draw's [18, B]."""
    return np.stack([offs[6 * (r // 2) + 2 * j + r % 2] for r in range(6)])


def _injected(aug, B, n_rows, seed):
    """(idxs, offs [18, B]) with a repeated row and words drawn by the augmentor from a private seed."""
    keep = np.random.get_state()
    np.random.seed(seed)
    idxs = np.random.randint(0, n_rows, size=B)
    idxs[1] = idxs[0]
    offs = np.zeros((18, B), dtype=np.int32)
    for j in range(3):
        for r, word in enumerate(aug.draw_index_words(B)):
            offs[6 * (r // 2) + 2 * j + r % 2] = word
    np.random.set_state(keep)
    return idxs, offs


def _walk(cont, capacity, links, stride, idxs):
    """The rows reached from ``idxs`` over at most ``links`` set continuity flags, a lane's rows ``stride`` apart."""
    out = []
    for r in idxs:
        for _ in range(links):
            if not cont[r]:
                break
            r = (r + stride) % capacity
        out.append(r)
    return np.array(out, dtype=np.int64)


def _restated(aug, obs_stacks, next_stacks, idxs, offs, next_rows=None, pos_rows=None):
    """(obs | next_obs | pos) as uint8 [3B, H, W, C]: ``RandomAffine.warp`` of the stored (n, C, H, W) stacks at the rows
    the route names (``pos_rows``: the positive is the next_obs of those rows; None: the anchor's obs)."""
    next_rows = idxs if next_rows is None else next_rows
    pos = obs_stacks[idxs] if pos_rows is None else next_stacks[pos_rows]
    outs = [aug.warp(stacks, _words_of_tensor(offs, j)) for j, stacks in enumerate((obs_stacks[idxs], next_stacks[next_rows], pos))]
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


@pytest.mark.parametrize("route", list(ROUTES))
def test_buffer_routes_give_the_restated_bytes(route):
    """B = 8 at (9,) + hw.  Two draws are injected through ``indices=``; the uint8 frames behind the three handles, then
    ``sample_cpc()``'s float NCHW tensors, equal ``RandomAffine.warp`` of the stored stacks at the rows the route names."""
    import curla_amd
    hw, cap, kw = ROUTES[route]
    B, dev = 8, torch.device("cuda")
    aug = curla_amd.make_augmentor("affine", hw, **AUG_KW)
    rb = curla_amd.ReplayBuffer((C9,) + hw, (2,), cap, B, dev, aug, **kw)
    stride = kw.get("n_envs", 1)
    if stride > 1:  # two lanes, one vector step at a time: ring row t N + e is lane e's step t
        lanes = [_episode(N_FILL // stride, C9 // 3, hw, 6 + e) for e in range(stride)]
        for t in range(N_FILL // stride):
            rb.add_vec(*(np.stack([lane[j][t] for lane in lanes]) for j in range(5)))
        ep = [np.stack([lane[j][t] for t in range(N_FILL // stride) for lane in lanes]) for j in range(5)]
    else:
        ep = _episode(N_FILL, C9 // 3, hw, 6)
        rb.add_batch(*ep)
    frame = C9 * hw[0] * hw[1]
    if route != "dedup":
        assert (rb._both is None) == (route == "two_allocations")
    assert rb._frame == frame == rb._scratch_frame() and rb._shift_store.shape[1] >= 3 * B * frame + 32
    assert rb.block_layout()["cut"] > 0 and rb._index_rows == 6
    obs_stacks, next_stacks = rb.stacks(0, N_FILL, 0), rb.stacks(0, N_FILL, 1)
    assert np.array_equal(obs_stacks, ep[0]) and np.array_equal(next_stacks, ep[3])
    cont = np.zeros(cap, dtype=np.uint8)
    if getattr(rb, "_cont_h", None) is not None:
        cont = np.asarray(rb._cont_h).astype(np.uint8)
    moved = False
    for seed in (11, 12):
        idxs, offs = _injected(aug, B, N_FILL, seed)
        next_rows = _walk(cont, cap, kw.get("n_step", 1) - 1, stride, idxs) if "n_step" in kw else None
        pos_rows = _walk(cont, cap, kw["pos_offset"] - 1, stride, idxs) if "pos_offset" in kw else None
        if next_rows is not None:
            assert (next_rows != idxs).any() and (next_rows < N_FILL).all()
            if stride > 1:
                assert not np.array_equal(next_rows, _walk(cont, cap, 2, 1, idxs))  # the stride did matter
        if pos_rows is not None:
            assert (pos_rows != idxs).any() and (pos_rows < N_FILL).all()
        want = _restated(aug, obs_stacks, next_stacks, idxs, offs, next_rows, pos_rows)
        sample = rb.sample_cpc_refs((idxs, offs))
        _check_refs(rb, sample, want)
        assert torch.equal(sample[1].cpu(), torch.from_numpy(ep[1][idxs]))
        assert not bool(rb._shift_store[rb._sample_slot][3 * B * frame:].any())  # the slack is never written
        plain = offs.copy()
        for j in range(3):
            for r in range(6):
                plain[6 * (r // 2) + 2 * j + r % 2] = IDENTITY[r]
        unmoved = _restated(aug, obs_stacks, next_stacks, idxs, plain, next_rows, pos_rows)
        assert np.array_equal(unmoved[:B].transpose(0, 3, 1, 2), obs_stacks[idxs])
        moved = moved or bool((want != unmoved).any())
        o, _, _, nx, _, kwargs = rb.sample_cpc((idxs, offs))
        want_f = torch.from_numpy(want.transpose(0, 3, 1, 2).astype(np.float32))
        for t, j in ((o, 0), (nx, 1), (kwargs["obs_pos"], 2)):
            assert t.dtype == torch.float32 and tuple(t.shape) == (B, C9) + hw
            assert torch.equal(t.cpu(), want_f[j * B:(j + 1) * B])
    assert moved  # (the words did matter)


# ------------------------------------------------------------------------------------------------ a whole update
def _agent(seed, hw, C, **aug_kw):
    import curla_amd
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    np.random.seed(seed)
    aug = curla_amd.make_augmentor("affine", hw, **aug_kw)
    return curla_amd.CurlSacAgent((C,) + hw, (2,), torch.device("cuda"), aug, hidden_dim=64, **HP)


def test_two_updates_are_the_updates_of_the_host_warped_pixels():
    """Steps 0 and 1 (critic + actor + target update, critic + CURL) from a buffer of ``make_augmentor('affine', hw)``
    with injected draws, against the same agent fed frames warped with NumPy (``RandomAffine.warp``): the logged losses,
    the gradient buffers, every flat parameter buffer, the targets, Adam moments, log_alpha and the device generator end
    bit-identical -- and differ from a run on the unwarped pixels."""
    import curla_amd
    B, C, hw, n_fill = 32, 9, (40, 44), 200
    aug = curla_amd.make_augmentor("affine", hw)
    ep = _episode(n_fill, C // 3, hw, 6)

    class Injected(curla_amd.ReplayBuffer):
        queue = collections.deque()

        def draw_indices(self):
            return self.queue.popleft()

    rb = Injected((C,) + hw, (2,), 256, B, torch.device("cuda"), aug)
    rb.add_batch(*ep)
    draws = [_injected(aug, B, n_fill, 30 + s) for s in range(2)]
    Injected.queue.extend(draws)
    scal = lambda i: (ep[1][i], ep[2][i], 1.0 - ep[4][i].astype(np.float32))  # noqa: E731
    ident = np.zeros((18, B), dtype=np.int32)
    for j in range(3):
        for r in range(6):
            ident[6 * (r // 2) + 2 * j + r % 2] = IDENTITY[r]
    batches = [(_restated(aug, ep[0], ep[3], i, o),) + scal(i) for i, o in draws]
    plain = [(_restated(aug, ep[0], ep[3], i, ident),) + scal(i) for i, _ in draws]
    runs = []
    for source in (rb, _HostShiftedBuffer(batches, B, hw), _HostShiftedBuffer(plain, B, hw)):
        agent, L = _agent(5, hw, C), NullLogger()
        losses = []
        for step in range(2):
            agent.update(source, L, step)
            losses.append(dict(L.scalars))
        torch.cuda.synchronize()
        state = _state(agent, source)
        state["critic_grad"], state["actor_grad"] = agent._critic_gflat.cpu().clone(), agent._actor_gflat.cpu().clone()
        runs.append((state, losses))
    assert not Injected.queue
    (a, la), (b, lb), (c, _) = runs
    assert la == lb and len(la[1]) >= 4
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert float(a["critic_steps"][0]) == 2 and float(a["actor_steps"][0]) == 1
    assert not torch.equal(a["critic"], c["critic"])  # ... and the words did matter


# ------------------------------------------------------------------------------------------------ update graphs
@pytest.mark.parametrize("dedup", [False, True], ids=["affine", "affine+dedup"])
def test_graph_replay_is_the_eager_update_bit_for_bit(dedup):
    """The protocol of tests/test_gpu_graph_aug.py: 14 mixed steps with log_interval 5 (0, 5, 10 log and run eagerly;
    1, 2 warm up; 3, 4, 6, 7 capture; 8, 9, 11, 12, 13 replay) at (40, 44); the state compared includes NumPy's stream,
    torch's CPU generator and the device generator.  The graphed run calls curla_affine_u8 only while capturing."""
    setup = dict(aug="affine", dedup_frames=dedup)
    eager, calls_e, logs_e, _, _ = _run(False, **setup)
    graph, calls_g, logs_g, agent, rb = _run(True, **setup)
    replayed = [8, 9, 11, 12, 13]
    assert rb.graph_supported() and type(rb.augmentor).__name__ == "RandomAffine"
    assert tuple(rb.augmentor.output_shape) == (40, 44) and rb.obs_shape == (9, 40, 44)
    assert all(calls_e[s].get(KERNEL) == 1 and calls_e[s].get("curla_sample_stage") == 1 for s in range(14))
    assert all(calls_e[s].get("curla_gather_stacks", 0) == (2 if dedup else 0) for s in range(14))
    assert [sum(calls_g[s].values()) for s in replayed] == [0] * len(replayed), calls_g
    assert all(sum(calls_g[s].values()) > 15 and calls_g[s].get(KERNEL, 0) >= 1 for s in (0, 1, 2, 3, 4, 5, 6, 7, 10)), calls_g
    assert len(agent._graphs) == 2 and all(len(r) == 2 and all(g["graph"] is not None for g in r)
                                           for r in agent._graphs.values())
    assert logs_e == logs_g
    for k in eager:
        assert torch.equal(eager[k], graph[k]), k
    assert float(eager["critic_steps"][0]) == 14 and float(eager["actor_steps"][0]) == 7
    B, frame = rb.batch_size, 9 * 40 * 44
    assert len(rb._graph_blocks) == 4
    for g in rb._graph_blocks.values():
        assert len(g["guards"]) == (4 if dedup else 2)
        for guard in g["guards"]:
            assert guard.numel() >= rb.GUARD and bool((guard == rb.GUARD_BYTE).all())
        assert g["shift_u8"].numel() == 3 * B * frame + 32
        assert bool(g["shift_u8"][:3 * B * frame].any()) and not bool(g["shift_u8"][-32:].any())
