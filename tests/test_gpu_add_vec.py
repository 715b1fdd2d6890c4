"""Vectorised environments on the device (``ReplayBuffer(n_envs=N)``): the strided chain walks against their NumPy
restatement and, at stride 1, against the entry points they generalise; curla_add_vec's bytes against N single-environment
buffers fed by add(); sampling, a whole update and graph replay on a vector n-step buffer; priorities of new rows.

Everything is compared bit for bit: the kernels move bytes and indices, and the n-step composition does at most n - 1
rounded multiply-adds in a fixed order, which the restatement repeats with float32 scalars."""
import numpy as np
import pytest
import torch

from tests.test_add_vec_host import streams
from tests.test_gpu_agent import HP, NullLogger
from tests.test_gpu_nstep import _guarded

pytestmark = pytest.mark.gpu

N = 3


def walk(reward, not_done, cont, capacity, n, gamma, r0, stride):
    """tests/test_gpu_nstep.py's restatement with the lane's stride: (reward_n, not_done_n, r_last) of a sample that
    starts at ring row r0."""
    gamma = np.float32(gamma)
    R, g, r, m = np.float32(reward[r0]), np.float32(1.0), int(r0), 1
    while m < n and cont[r]:
        r = (r + stride) % capacity
        g = np.float32(g * gamma)
        R = np.float32(R + np.float32(g * np.float32(reward[r])))
        m += 1
    return R, np.float32(np.float32(not_done[r]) * g), r


def walk_all(reward, not_done, cont, capacity, n, gamma, idx, stride):
    out = [walk(reward, not_done, cont, capacity, n, gamma, r0, stride) for r0 in idx]
    return (np.array([o[0] for o in out], dtype=np.float32), np.array([o[1] for o in out], dtype=np.float32),
            np.array([o[2] for o in out], dtype=np.int64))


def pos_rows(cont, capacity, k, idx, stride):
    """The rows whose next_obs is the positive: idx walked at most k - 1 links of its lane."""
    out = []
    for r in idx:
        r = int(r)
        for _ in range(k - 1):
            if not cont[r]:
                break
            r = (r + stride) % capacity
        out.append(r)
    return np.array(out, dtype=np.int64)


# ------------------------------------------------------------------------------------------------ the walk kernels
CAP, STRIDE, A, B = 18, 3, 2, 24
#       row  0  1  2   3  4  5   6  7  8   9 10 11  12 13 14  15 16 17     lane e = rows e, e + 3, ...
CONT = [1, 1, 0, 1, 0, 1, 1, 0, 0, 1, 1, 0, 1, 1, 1, 0, 1, 0]
IDX = list(range(CAP)) + [16, 13, 0, 15, 5, 10]   # every row once plus six repeats
NS, GAMMAS, KS = (1, 2, 3, 5), (0.99, 1.0), (1, 2, 4)
NR_OFF = 2 * B * 8 + 6 * B * 4                    # idx int64 [2B] | offsets int32 [6][B] | next_row int64 [B] |
POS_OFF = NR_OFF + 8 * B                          # pos_row int64 [2][B] | pos_run int64 [3B]
RUN_OFF = POS_OFF + 16 * B
NBYTES = RUN_OFF + 24 * B
GUARD_BYTE = 0xA5


def test_the_flags_hold_every_case():
    """Runs shorter than, equal to and longer than n - 1 for every n; lane 1 crosses the ring's end; and a stride-1 walk
    over the same flags ends elsewhere for most start rows, so a kernel that ignored the stride could not pass."""
    runs = []
    for r0 in range(CAP):
        r, L = r0, 0
        while CONT[r]:
            r, L = (r + STRIDE) % CAP, L + 1
        runs.append(L)
    assert runs == [5, 1, 0, 4, 0, 1, 3, 0, 0, 2, 4, 0, 1, 3, 1, 0, 2, 0]
    for n in (2, 3, 5):
        assert any(L < n - 1 for L in runs) and any(L == n - 1 for L in runs) and any(L > n - 1 for L in runs)
    assert CONT[16] and 16 % STRIDE == 1 and (16 + STRIDE) % CAP == 1 and CONT[1]
    z = np.zeros(CAP, dtype=np.float32)
    differ = [int((walk_all(z, z, CONT, CAP, n, 1.0, range(CAP), STRIDE)[2]
                   != walk_all(z, z, CONT, CAP, n, 1.0, range(CAP), 1)[2]).sum()) for n in (2, 3, 5)]
    assert differ == [11, 11, 10]
    assert sorted(set(IDX)) == list(range(CAP)) and len(IDX) == B


@pytest.fixture(scope="module")
def ring():
    """The scalar rows of a ring of 18 (random float32, negatives included), the flags and the host block, made once and
    never written."""
    rs = np.random.RandomState(7)
    sc = rs.randn(CAP, A + 2).astype(np.float32)
    assert (sc[:, A] < 0).any() and (sc[:, A] > 0).any()
    host = np.full(NBYTES, 0x77, dtype=np.uint8)
    i64 = host[:2 * B * 8].view(np.int64)
    i64[:B] = IDX
    i64[B:] = i64[:B] + CAP
    host[2 * B * 8:NR_OFF].view(np.int32)[:] = rs.randint(0, 9, 6 * B)
    dev = torch.device("cuda")
    return dict(sc=sc, host=host, sc_d=torch.from_numpy(sc).to(dev),
                cont_d=torch.tensor(CONT, dtype=torch.uint8, device=dev), pinned=torch.from_numpy(host.copy()).pin_memory())


def _launch(ring, entry, n, gamma, k, with_run, stride, names="strided", cap=CAP, outs=None):
    """One route of ReplayBuffer._stage through the C ABI, by name: ``names`` "strided" calls the _strided entry points
    with ``stride``, "old" their namesakes (no stride argument).  ``entry``: "device" = the block is on the device
    already (curla_nstep_compose, then curla_pos_walk), "pinned" = one staging launch with both walks
    (curla_sample_stage_pos), "pinned_nstep" = one staging launch with the composition alone
    (curla_sample_stage_nstep; k and with_run do not apply).  Returns the block's bytes, the three outputs, the guards."""
    from curla_amd import ops
    from curla_amd._lib import call, ptr, stream
    if outs is None:
        outs = _guarded([NBYTES, 4 * B * A, 4 * B, 4 * B])
    (blk, act, rew, nd), guards = outs
    act, rew, nd = act.view(torch.float32), rew.view(torch.float32), nd.view(torch.float32)
    sfx, st = ("_strided", (stride,)) if names == "strided" else ("", ())
    run = RUN_OFF if with_run else -1
    sc, cont = ptr(ring["sc_d"]), ptr(ring["cont_d"])
    o = (ptr(act), ptr(rew), ptr(nd), stream())
    if entry == "device":
        blk.copy_(torch.from_numpy(ring["host"]))
        call("curla_nstep_compose" + sfx, ptr(blk), NR_OFF, sc, cont, cap, *st, n, gamma, B, A, *o)
        call("curla_pos_walk" + sfx, ptr(blk), POS_OFF, run, NR_OFF, cont, cap, *st, k, n, B, stream())
    elif entry == "pinned":
        call("curla_sample_stage_pos" + sfx, ops.host_device_pointer(ring["pinned"]), ptr(blk), NBYTES, NR_OFF, POS_OFF, run,
             sc, cont, cap, *st, n, gamma, k, B, A, *o)
    else:
        call("curla_sample_stage_nstep" + sfx, ops.host_device_pointer(ring["pinned"]), ptr(blk), NBYTES, NR_OFF, sc, cont,
             cap, *st, n, gamma, B, A, *o)
    torch.cuda.synchronize()
    return blk.cpu().numpy(), act.cpu().numpy().reshape(B, A), rew.cpu().numpy(), nd.cpu().numpy(), guards


def _expected(ring, entry, n, gamma, k, with_run, stride):
    sc, want = ring["sc"], ring["host"].copy()
    want_r, want_nd, last = walk_all(sc[:, A], sc[:, A + 1], CONT, CAP, n, gamma, IDX, stride)
    want[B * 8:2 * B * 8].view(np.int64)[:] = CAP + last
    want[NR_OFF:POS_OFF].view(np.int64)[:] = last
    if entry != "pinned_nstep":
        r = pos_rows(CONT, CAP, k, IDX, stride)
        want[POS_OFF:RUN_OFF].view(np.int64)[:] = np.concatenate([r, CAP + r])
        if with_run:
            want[RUN_OFF:].view(np.int64)[:] = np.concatenate([IDX, CAP + last, CAP + r])
    return want, want_r, want_nd, last


@pytest.mark.parametrize("with_run", [False, True])
@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("entry", ["device", "pinned"])
def test_walk_kernels_against_the_strided_restatement(ring, entry, n, gamma, with_run):
    """A1, k in {1, 2, 4}: reward, not_done, the bootstrap rows (twice), the positive's rows (twice), the run of a scratch
    augmentation, every word of the block that no walk owns as the host wrote it, the guards around every buffer."""
    outs = _guarded([NBYTES, 4 * B * A, 4 * B, 4 * B])
    for k in KS:
        got, act, rew, nd, guards = _launch(ring, entry, n, gamma, k, with_run, STRIDE, outs=outs)
        want, want_r, want_nd, last = _expected(ring, entry, n, gamma, k, with_run, STRIDE)
        assert np.array_equal(rew, want_r) and np.array_equal(nd, want_nd), k
        assert np.array_equal(got[B * 8:2 * B * 8].view(np.int64), CAP + last), k
        assert np.array_equal(got[NR_OFF:POS_OFF].view(np.int64), last), k
        assert np.array_equal(got[POS_OFF:RUN_OFF].view(np.int64), want[POS_OFF:RUN_OFF].view(np.int64)), k
        assert np.array_equal(got, want), k  # the run region, and every untouched word
        assert np.array_equal(act, ring["sc"][IDX, :A])
        assert all(bool((g == GUARD_BYTE).all()) and g.numel() >= 256 for g in guards)
        if n > 1:  # walks happened, some across the ring's end, and not where a stride-1 walk ends
            assert (last != np.array(IDX)).any() and (last < np.array(IDX)).any()
            one = walk_all(ring["sc"][:, A], ring["sc"][:, A + 1], CONT, CAP, n, gamma, IDX, 1)
            assert not np.array_equal(one[2], last) and not np.array_equal(one[0], want_r)
        if k > 1:
            assert not np.array_equal(pos_rows(CONT, CAP, k, IDX, 1), pos_rows(CONT, CAP, k, IDX, STRIDE))


@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("n", NS)
def test_staged_composition_against_the_strided_restatement(ring, n, gamma):
    """A1, the staging launch without a positive (curla_sample_stage_nstep_strided)."""
    got, act, rew, nd, guards = _launch(ring, "pinned_nstep", n, gamma, 1, False, STRIDE)
    want, want_r, want_nd, _ = _expected(ring, "pinned_nstep", n, gamma, 1, False, STRIDE)
    assert np.array_equal(rew, want_r) and np.array_equal(nd, want_nd) and np.array_equal(got, want)
    assert np.array_equal(act, ring["sc"][IDX, :A])
    assert all(bool((g == GUARD_BYTE).all()) for g in guards)


@pytest.mark.parametrize("entry", ["device", "pinned", "pinned_nstep"])
def test_stride_1_through_the_strided_entry_points_is_the_old_entry_point(ring, entry):
    """A2: on the same inputs, for every n, gamma, k and with and without a run region, the _strided entry point with
    stride 1 leaves the bytes its namesake leaves -- which are the stride-1 restatement's."""
    cases = [(n, g, k, run) for n in NS for g in GAMMAS for k in KS for run in (False, True)]
    if entry == "pinned_nstep":
        cases = [(n, g, 1, False) for n in NS for g in GAMMAS]
    outs = [_guarded([NBYTES, 4 * B * A, 4 * B, 4 * B]) for _ in range(2)]
    for n, gamma, k, with_run in cases:
        new = _launch(ring, entry, n, gamma, k, with_run, 1, "strided", outs=outs[0])
        old = _launch(ring, entry, n, gamma, k, with_run, None, "old", outs=outs[1])
        for a, b in zip(new[:4], old[:4]):
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), (n, gamma, k, with_run)
        want, want_r, want_nd, _ = _expected(ring, entry, n, gamma, k, with_run, 1)
        assert np.array_equal(new[0], want) and np.array_equal(new[2], want_r) and np.array_equal(new[3], want_nd)
        assert all(bool((g == GUARD_BYTE).all()) for g in new[4] + old[4])


def test_entry_points_refuse_bad_arguments(ring):
    """A3: CURLA_ERR_ARG before any launch -- the block, the outputs and the rings are what they were."""
    from curla_amd import _lib, ops
    outs = _guarded([NBYTES, 4 * B * A, 4 * B, 4 * B])
    (blk, act, rew, nd), guards = outs
    blk.copy_(torch.from_numpy(ring["host"]))
    before = [t.clone() for t in (act, rew, nd)]
    for entry in ("device", "pinned", "pinned_nstep"):
        for stride, cap in ((0, CAP), (-1, CAP), (-3, CAP), (4, CAP), (5, CAP), (2 * CAP, CAP), (3, 0), (3, 17)):
            with pytest.raises(_lib.CurlaHipError, match="CURLA_ERR_ARG"):
                _launch(ring, entry, 3, 0.99, 2, True, stride, cap=cap, outs=outs)
            blk.copy_(torch.from_numpy(ring["host"]))  # ("device" stages the block itself before the refused call)
    with pytest.raises(_lib.CurlaHipError, match="CURLA_ERR_ARG"):  # the positive's walk alone
        ops.pos_walk(blk, POS_OFF, RUN_OFF, NR_OFF, ring["cont_d"], CAP, 2, 3, B, stride=4)
    torch.cuda.synchronize()
    assert np.array_equal(blk.cpu().numpy(), ring["host"])
    assert all(torch.equal(a, b) for a, b in zip(before, (act, rew, nd)))
    assert all(bool((g == GUARD_BYTE).all()) for g in guards)
    # curla_add_vec: a ring of 6 rows of (3, 2, 2) frames and a block for N = 3, all between guards
    C, H, W, cap, fr = 3, 2, 2, 6, 12
    sc_off = (2 * N * fr + 15) & ~15
    (block, rings, sc, cont), guards = _guarded([sc_off + 4 * N * (A + 2) + 2 * N, 2 * cap * fr, 4 * cap * (A + 2), cap])
    for t in (block, rings, sc, cont):
        t.fill_(0x3C)
    obs_ring, next_ring = rings[:cap * fr].view(cap, H, W, C), rings[cap * fr:].view(cap, H, W, C)
    good = dict(block=block, obs=obs_ring, next=next_ring, sc=sc.view(torch.float32).view(cap, A + 2), cont=cont, cap=cap,
                first=3, prev=1, N=N, C=C, H=H, W=W, A=A)
    bad = [dict(N=0), dict(N=-1), dict(first=1), dict(first=4), dict(first=6), dict(first=-3), dict(N=4, first=4),
           dict(block=None), dict(obs=None), dict(next=None), dict(sc=None), dict(cont=None), dict(cap=3, first=0),
           dict(C=0), dict(H=0), dict(W=0), dict(A=0)]
    for b in bad:
        a = {**good, **b}
        with pytest.raises(_lib.CurlaHipError, match="CURLA_ERR_ARG"):
            _lib.call("curla_add_vec", *(_lib.ptr(a[k]) for k in ("block", "obs", "next", "sc", "cont")), a["cap"],
                      a["first"], a["prev"], a["N"], a["C"], a["H"], a["W"], a["A"], _lib.stream())
    torch.cuda.synchronize()
    assert all(bool((t == 0x3C).all()) for t in (block, rings, sc, cont))
    assert all(bool((g == GUARD_BYTE).all()) for g in guards)


# ------------------------------------------------------------------------------------------------ curla_add_vec
def _chained(C, hw, link, done, seed):
    """A stream of len(link) transitions of (C,) + hw frames with the given links (next_obs[t] is obs[t + 1] where
    link[t]) and dones: test_nstep_host.episodes() for any channel count."""
    rs = np.random.RandomState(seed)
    frame = lambda: rs.randint(0, 256, (C,) + hw, dtype=np.uint8)  # noqa: E731
    T = len(link)
    obs, nxt, cur = [], [], frame()
    for t in range(T):
        obs.append(cur), nxt.append(frame())
        cur = nxt[-1] if link[t] else frame()
    return np.stack(obs), rs.uniform(-1, 1, (T, A)).astype(np.float32), rs.randn(T).astype(np.float32), np.stack(nxt), done


def _stores(rb):
    """Every byte the write paths may touch: the ring allocation(s) with their slack, the scalar rows, the flags."""
    rings = [rb._ring_store] if rb._both is not None else [rb._obs_store, rb._next_store]
    return rings + [rb._sc.view(torch.uint8).view(-1), rb._cont]


# (C, H, W): the dword path; the byte path (35 pixels: no whole number of 4-pixel groups), rings in one allocation; the
# byte path with capacity * frame % 4 != 0, rings in two allocations
GEOMETRIES = {"dwords": (9, 20, 20), "bytes": (4, 5, 7), "bytes_two_allocations": (3, 5, 7)}


@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_add_vec_stores_what_three_add_fed_buffers_store(geometry):
    """A4: 12 vector steps into a ring of 21 = 3 lanes of 7 (the ring wraps; the step at rows 18..20 and the one after
    it have their previous run at the ring's end) against three capacity-7 buffers fed one lane each by add().  After
    every step: lane e of obs, next_obs, the scalar rows and the flags equals single[e]'s, and every byte of the stores
    outside the rows the step names -- the other rows, the 32 bytes of slack -- is what it was before the call."""
    from curla_amd import IdentityAugmentation, ReplayBuffer
    C, H, W = GEOMETRIES[geometry]
    lanes, _ = streams()
    lanes = [_chained(C, (H, W), l[5], l[4], 10 + e) for e, l in enumerate(lanes)]
    dev, aug, cap, fr = torch.device("cuda"), IdentityAugmentation((H, W)), 21, C * H * W
    mk = lambda c, n: ReplayBuffer((C, H, W), (A,), c, 4, dev, aug, n_step=3, discount=0.99, n_envs=n)  # noqa: E731
    vec, single = mk(cap, N), [mk(cap // N, 1) for _ in range(N)]
    assert (vec._both is None) == (geometry == "bytes_two_allocations") == ((cap * fr) % 4 != 0)
    assert ((H * W) % 4 == 0) == (geometry == "dwords")
    for t in _stores(vec)[:-2]:
        t.fill_(0x5A)  # (the slack included)
    vec._sc.fill_(-7.0)
    vec._cont.fill_(9)
    for t in range(12):
        first, prev = (t * N) % cap, ((t - 1) * N) % cap
        before = [s.clone() for s in _stores(vec)]
        vec.add_vec(*(np.stack([l[j][t] for l in lanes]) for j in range(5)))
        for e in range(N):
            single[e].add(*(lanes[e][j][t] for j in range(5)))
        torch.cuda.synchronize()
        assert vec.idx == (first + N) % cap and vec.full == (t >= 6)
        seen = min(t + 1, 7)  # rows of a lane that hold a transition
        rows = sorted((s * N) % cap // N for s in range(t + 1 - seen, t + 1))
        for e in range(N):
            assert torch.equal(vec.obses[e::N][rows], single[e].obses[rows]), (t, e)
            assert torch.equal(vec.next_obses[e::N][rows], single[e].next_obses[rows]), (t, e)
            assert torch.equal(vec._sc[e::N][rows], single[e]._sc[rows]), (t, e)
            assert torch.equal(vec._cont[e::N][rows], single[e]._cont[rows]), (t, e)
        assert np.array_equal(vec._cont.cpu().numpy()[[r * N + e for r in rows for e in range(N)]],
                              vec._cont_h[[r * N + e for r in rows for e in range(N)]])
        # what the call may have written: rows first .. first + N - 1 of both rings and of the scalars, the flags of
        # the new run and (from the second step on) of the previous one
        after = _stores(vec)
        keep = torch.ones(cap, dtype=torch.bool, device=dev)
        keep[first:first + N] = False
        ring_keep = keep.repeat_interleave(fr)
        if vec._both is not None:
            mask = torch.cat([ring_keep, ring_keep, torch.ones(32, dtype=torch.bool, device=dev)])
            assert torch.equal(after[0][mask], before[0][mask]), t
        else:
            mask = torch.cat([ring_keep, torch.ones(32, dtype=torch.bool, device=dev)])
            assert torch.equal(after[0][mask], before[0][mask]) and torch.equal(after[1][mask], before[1][mask]), t
        sc_keep = keep.repeat_interleave(4 * (A + 2))
        assert torch.equal(after[-2][sc_keep], before[-2][sc_keep]), t
        if t > 0:
            keep[prev:prev + N] = False
        assert torch.equal(after[-1][keep], before[-1][keep]), t
    assert vec._cont_h.reshape(7, N).T.tolist() == [[0, 1, 1, 1, 0, 1, 1], [1, 1, 1, 1, 0, 1, 0], [1, 1, 1, 1, 0, 0, 0]]
    assert np.array_equal(vec._cont.cpu().numpy(), vec._cont_h)
    # the planar frames arrived transposed: ring row (t N + e) % capacity is lane e's step t, HWC
    for e in range(N):
        r = (11 * N + e) % cap
        assert np.array_equal(vec.obses[r].permute(2, 0, 1).cpu().numpy(), lanes[e][0][11])
        assert np.array_equal(vec.next_obses[r].permute(2, 0, 1).cpu().numpy(), lanes[e][3][11])


@pytest.mark.parametrize("prioritized", [False, True])
def test_an_add_vec_is_one_copy_and_one_launch(monkeypatch, prioritized):
    """On the device: one tensor copy (the pinned block) and one library call, curla_add_vec -- plus curla_per_set on a
    prioritized buffer -- per vector step, the step with a previous run at the ring's end included."""
    import curla_amd.ops as ops_mod
    from curla_amd import IdentityAugmentation, ReplayBuffer
    rb = ReplayBuffer((9, 20, 20), (A,), 6, 4, torch.device("cuda"), IdentityAugmentation((20, 20)), n_step=3,
                      discount=0.99, n_envs=N, prioritized=prioritized)
    _, vec = streams()
    copies, calls, real_copy, real_call = [], [], torch.Tensor.copy_, ops_mod.call

    def copy_(self, *a, **k):
        copies.append(self.data_ptr())
        return real_copy(self, *a, **k)

    def call(name, *a):
        calls.append(name)
        return real_call(name, *a)
    monkeypatch.setattr(torch.Tensor, "copy_", copy_)
    monkeypatch.setattr(ops_mod, "call", call)
    for t in range(3):  # rows 0..2, rows 3..5, rows 0..2 again (previous run: rows 3..5, the ring's end)
        rb.add_vec(*(a[t] for a in vec))
    torch.cuda.synchronize()
    assert copies == [rb._d_add.data_ptr()] * 3
    assert calls == (["curla_add_vec"] + ["curla_per_set"] * prioritized) * 3
    assert rb.idx == 3 and rb.full and np.array_equal(rb._cont.cpu().numpy(), rb._cont_h)


# ------------------------------------------------------------------------------------------------ sampling
SAMPLE_CAP, SAMPLE_B, HW = 21, 8, (20, 20)


def _augmentor(kind):
    import curla_amd
    return {"ring": lambda: curla_amd.RandomCrop(HW, (16, 18)), "scratch": lambda: curla_amd.RandomShift(HW, 2),
            "float": lambda: curla_amd.RandomConv(HW)}[kind]()


@pytest.mark.parametrize("kind", ["ring", "scratch", "float"])
def test_a_vector_buffer_samples_along_its_lanes(kind):
    """A5: X = n_envs=3, n_step=3, pos_offset=2, capacity 21, B = 8, filled past a wrap with the host tests' three
    streams.  The sampled reward and not_done are the strided restatement's over the host mirrors; next_obs is the 1-step
    next_obs of the restated bootstrap rows and the positive the next_obs of the restated positive rows, as a twin without
    either keyword hands them out; obs and the actions are the sampled rows'.  And the same seed on an n_envs=1 buffer
    that holds as many rows draws the same host RNG values."""
    from curla_amd import ReplayBuffer
    from tests.test_gpu_temporal_pos import _pos_as_next, _sample
    _, vec = streams()
    aug, dev = _augmentor(kind), torch.device("cuda")
    kw = dict(staged_aug=True) if kind == "float" else {}
    X = ReplayBuffer((9,) + HW, (A,), SAMPLE_CAP, SAMPLE_B, dev, aug, n_step=3, discount=0.99, pos_offset=2, n_envs=N, **kw)
    Y = ReplayBuffer((9,) + HW, (A,), SAMPLE_CAP, SAMPLE_B, dev, aug, n_envs=N, **kw)
    assert X._kind == kind and X.staged_aug == (kind == "float")
    for t in range(12):
        for rb in (X, Y):
            rb.add_vec(*(a[t] for a in vec))
    flags = X._cont_h.copy()
    assert np.array_equal(X._cont.cpu().numpy(), flags) and flags.sum() == 14
    np.random.seed(31)
    idxs, offs = X.draw_indices()
    one = ReplayBuffer((9,) + HW, (A,), SAMPLE_CAP, SAMPLE_B, dev, aug, **kw)
    for e in range(N):  # lane by lane: 36 rows into the ring of 21, as many as X holds
        one.add_batch(*(a[:, e] for a in vec))
    assert (one.idx, one.full) == (X.idx, X.full) == (15, True)
    np.random.seed(31)
    idxs1, offs1 = one.draw_indices()
    assert np.array_equal(idxs, idxs1) and np.array_equal(offs, offs1)
    idxs = np.array([16, 2, 15, 12, 0, 7, 20, 16])  # 15 -> 18 -> 0 crosses the ring's end; 12 is one of the newest rows
    sc = X._sc.cpu().numpy()
    want_r, want_nd, last = walk_all(sc[:, A], sc[:, A + 1], flags, SAMPLE_CAP, 3, 0.99, idxs, N)
    r = pos_rows(flags, SAMPLE_CAP, 2, idxs, N)
    assert (last != idxs).sum() >= 3 and (last == idxs).sum() >= 2 and (last < idxs).any() and (r != last).any()
    assert not np.array_equal(walk_all(sc[:, A], sc[:, A + 1], flags, SAMPLE_CAP, 3, 0.99, idxs, 1)[2], last)
    ox, nx, px, ax, rx, dx, _ = _sample(X, idxs, offs)
    o0, n0, _, a0, _, _, _ = _sample(Y, idxs, offs)
    assert torch.equal(ox, o0) and torch.equal(ax, a0) and not torch.equal(nx, n0)
    assert np.array_equal(rx.cpu().numpy().reshape(-1), want_r) and np.array_equal(dx.cpu().numpy().reshape(-1), want_nd)
    _, n_last, _, _, _, _, _ = _sample(Y, last, offs)
    assert torch.equal(nx, n_last)
    _, n_r, _, _, _, _, _ = _sample(Y, r, _pos_as_next(offs), pos_params_as_next=True)
    assert torch.equal(px, n_r)


# ------------------------------------------------------------------------------------------------ whole update
def test_update_equals_a_one_step_update_on_host_composed_rows():
    """A6: X = n_envs=3, n_step=3, fed the three streams by add_vec.  Y = n_envs=1, n_step=1, row j = (obs_j, action_j,
    restated reward, restated not_done, next_obs of row r_last(j)), the restatement walking with stride 3.  Two agents
    with the same seed, 4 updates (even and odd steps) on the same injected indices: parameters, targets, Adam moments
    and log_alpha end bit-identical -- and differ from a stride-1 composition of the same rows."""
    import curla_amd
    from tests.test_gpu_graph_aug import _state
    in_hw, out_hw, cap, Bb, n, gamma = (34, 40), (28, 34), 48, 8, 3, HP["discount"]
    _, vec = streams(hw=in_hw)
    obs, act, rew, nxt, done = (a.reshape((36,) + a.shape[2:]) for a in vec)
    T, dev = 36, torch.device("cuda")
    aug = curla_amd.RandomCrop(in_hw, out_hw)
    X = curla_amd.ReplayBuffer((9,) + in_hw, (2,), cap, Bb, dev, aug, n_step=n, discount=gamma, n_envs=N)
    for t in range(12):
        X.add_vec(*(a[t] for a in vec))
    flags = X._cont.cpu().numpy()
    assert np.array_equal(flags, X._cont_h) and flags[:T].sum() == 26 and not flags[T - N:].any()
    nd = 1.0 - done.astype(np.float32)
    assert np.array_equal(X._sc.cpu().numpy()[:T, 2], rew) and np.array_equal(X._sc.cpu().numpy()[:T, 3], nd)

    def composed(stride):
        want_r, want_nd, last = walk_all(rew, nd, flags, cap, n, gamma, np.arange(T), stride)
        Y = curla_amd.ReplayBuffer((9,) + in_hw, (2,), cap, Bb, dev, aug)
        for t in range(T):
            Y.add(obs[t], act[t], 0.0, nxt[last[t]], False)
        Y.rewards[:T] = torch.from_numpy(want_r).to(dev).view(T, 1)
        Y.not_dones[:T] = torch.from_numpy(want_nd).to(dev).view(T, 1)
        return Y
    rs = np.random.RandomState(2)
    draws = [(rs.randint(0, T, Bb), rs.randint(0, 7, (6, Bb)).astype(np.int32)) for _ in range(4)]
    states = []
    for rb in (X, composed(N), composed(1)):
        curla_amd.set_seed_everywhere(11)
        agent = curla_amd.CurlSacAgent((9,) + out_hw, (2,), dev, aug, hidden_dim=64, **HP)
        it = iter(draws)
        rb.draw_indices = lambda it=it: next(it)
        for step in range(4):
            agent.update(rb, NullLogger(), step)
        torch.cuda.synchronize()
        states.append(_state(agent, rb))
    assert float(states[0]["critic_steps"][0]) == 4 and float(states[0]["actor_steps"][0]) == 2
    for k in states[0]:
        assert torch.equal(states[0][k], states[1][k]), k
    assert not torch.equal(states[0]["critic"], states[2]["critic"])


def test_graph_replay_of_a_vector_buffer_is_the_eager_update(monkeypatch):
    """A6: update graphs on an n_envs=3, n_step=3, pos_offset=2 buffer.  10 mixed steps as in tests/test_gpu_graph_aug.py
    (0 and 5 log and run eagerly; 1, 2 warm up; 3, 4, 6, 7 capture; 8 and 9 replay): the two replayed updates make no
    kernel call from the host and the run ends where the eager run ends."""
    import curla_amd
    import tests.test_gpu_graph_aug as G

    def build(aug, B=64, seed=5):
        torch.manual_seed(seed)
        torch.cuda.manual_seed_all(seed)
        np.random.seed(seed)
        dev, in_hw = torch.device("cuda"), (40, 44)
        augmentor = curla_amd.make_augmentor(aug, in_hw, (32, 36))
        agent = curla_amd.CurlSacAgent((9, 32, 36), (2,), dev, augmentor, hidden_dim=64, **{**HP, "log_interval": 5})
        rb = curla_amd.ReplayBuffer((9,) + in_hw, (2,), 300, B, dev, augmentor, n_step=3, discount=HP["discount"],
                                    pos_offset=2, n_envs=N)
        lanes = [G._episode(80, 3, in_hw, 6 + e) for e in range(N)]
        for t in range(80):
            rb.add_vec(*(np.stack([l[j][t] for l in lanes]) for j in range(5)))
        return agent, rb
    monkeypatch.setattr(G, "_build", build)
    eager, calls_e, logs_e, _, rb_e = G._run(False, steps=10, aug="random_crop")
    graph, calls_g, logs_g, agent, rb = G._run(True, steps=10, aug="random_crop")
    assert rb.graph_supported() and rb.idx == rb_e.idx == 240 and int(rb._cont.sum()) == int(rb._cont_h.sum()) > 180
    assert [sum(calls_g[s].values()) for s in (8, 9)] == [0, 0], calls_g
    assert all(calls_e[s].get("curla_sample_stage_pos_strided") == 1 and not calls_e[s].get("curla_sample_stage_pos")
               for s in range(10))
    assert calls_g[7].get("curla_sample_stage_pos_strided") == 1  # recorded by the capture
    assert len(agent._graphs) == 2 and all(len(r) == 2 and all(g["graph"] is not None for g in r)
                                           for r in agent._graphs.values())
    assert agent._graph_rb_key() == (3, HP["discount"], 2, N)
    assert logs_e == logs_g
    for k in eager:
        assert torch.equal(eager[k], graph[k]), k


# ------------------------------------------------------------------------------------------------ prioritized
def test_new_rows_of_a_vector_step_take_the_maximum():
    """A7: after an add_vec the N new rows hold the largest value given so far, and the chunk sums are the float64 sums
    of their chunks' rows -- also where the run straddles two chunks (rows 255 .. 257)."""
    from curla_amd import IdentityAugmentation, ReplayBuffer, ops
    dev, cap = torch.device("cuda"), 516
    rb = ReplayBuffer((3, 4, 4), (A,), cap, 4, dev, IdentityAugmentation((4, 4)), prioritized=True, n_envs=N)
    rs = np.random.RandomState(3)
    step = lambda: (rs.randint(0, 256, (N, 3, 4, 4), dtype=np.uint8), rs.uniform(-1, 1, (N, A)), rs.randn(N),  # noqa: E731
                    rs.randint(0, 256, (N, 3, 4, 4), dtype=np.uint8), np.zeros(N, dtype=bool))

    def check(first, value, written):
        torch.cuda.synchronize()
        s = rb._per_s.cpu().numpy()
        assert s[first:first + N].tolist() == [value] * N and float(rb._per_max) == value
        assert int((s > 0).sum()) == written
        want = [s[c * ops.PER_CHUNK:(c + 1) * ops.PER_CHUNK].astype(np.float64).sum() for c in range(ops.per_chunks(cap))]
        assert rb._per_sums.cpu().numpy().tolist() == want
    rb.add_vec(*step())
    check(0, 1.0, 3)
    rb.update_priorities(torch.tensor([1], device=dev), torch.tensor([2.5], device=dev))
    rb.add_vec(*step())
    check(3, 2.5, 6)
    assert rb.priorities().tolist() == [1.0, 2.5, 1.0, 2.5, 2.5, 2.5]
    rb.idx = 255  # the next run straddles the chunk border at row 256
    rb.add_vec(*step())
    check(255, 2.5, 9)
    assert rb.idx == 258 and rb._per_sums.cpu().numpy().tolist() == [2 * 1.0 + 2.5 * 5, 2.5 * 2, 0.0]
