"""n-step returns on the device (``ReplayBuffer(n_step=...)``): the composition kernel against its NumPy restatement,
the bootstrap rows on every route a minibatch's next_obs can take, a whole update against a 1-step buffer whose rows were
composed on the host, and graph replay against the eager run.

Everything is compared bit for bit (``torch.equal`` / ``np.array_equal``): the kernel moves indices and does at most
n - 1 rounded multiply-adds in a fixed order, which the restatement repeats with float32 scalars."""
import numpy as np
import pytest
import torch

from tests.test_gpu_agent import HP, NullLogger
from tests.test_nstep_host import episodes

pytestmark = pytest.mark.gpu


def walk(reward, not_done, cont, capacity, n, gamma, r0):
    """The restatement: (reward_n, not_done_n, r_last) of a sample that starts at ring row r0 -- float32 scalars, every
    product and sum rounded on its own, in the kernel's order."""
    gamma = np.float32(gamma)
    R, g, r, m = np.float32(reward[r0]), np.float32(1.0), int(r0), 1
    while m < n and cont[r]:
        r = (r + 1) % capacity
        g = np.float32(g * gamma)
        R = np.float32(R + np.float32(g * np.float32(reward[r])))
        m += 1
    return R, np.float32(np.float32(not_done[r]) * g), r


def walk_all(reward, not_done, cont, capacity, n, gamma, idx):
    out = [walk(reward, not_done, cont, capacity, n, gamma, r0) for r0 in idx]
    return (np.array([o[0] for o in out], dtype=np.float32), np.array([o[1] for o in out], dtype=np.float32),
            np.array([o[2] for o in out], dtype=np.int64))


# ------------------------------------------------------------------------------------------------ the kernel
CAP, A, B = 11, 2, 16
#       row  0  1  2  3  4  5  6  7  8  9 10      runs of set flags: 9,10,0 (crosses the ring's end), 2..6, none at 1, 7, 8
CONT = [1, 0, 1, 1, 1, 1, 1, 0, 0, 1, 1]
IDX = list(range(CAP)) + [10, 10, 2, 9, 0]        # every row, repeats, the row just before the wrap
NR_OFF = 2 * B * 8 + 6 * B * 4                    # the block: idx int64 [2B] | offsets int32 [6][B] | next_row int64 [B]
NBYTES = NR_OFF + 8 * B
GUARD, GUARD_BYTE = 256, 0xA5


@pytest.fixture(scope="module")
def ring():
    """The scalar rows of a ring of 11 (random float32, negatives included; not_done arbitrary floats: the kernel
    multiplies whatever is stored), the flags and the host block, made once and never written."""
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
                cont_d=torch.tensor(CONT, dtype=torch.uint8, device=dev))


def _guarded(sizes):
    """uint8 device buffers of ``sizes`` bytes between 256-byte guards of 0xA5, in one allocation."""
    dev = torch.device("cuda")
    padded = [(n + GUARD - 1) // GUARD * GUARD for n in sizes]
    store = torch.full((GUARD + sum(p + GUARD for p in padded),), GUARD_BYTE, dtype=torch.uint8, device=dev)
    out, guards, at = [], [store[:GUARD]], GUARD
    for n, pn in zip(sizes, padded):
        out.append(store[at:at + n])
        guards.append(store[at + n:at + pn + GUARD])
        at += pn + GUARD
    return out, guards


def test_the_flags_hold_runs_shorter_equal_and_longer_than_every_n():
    runs = []
    for r0 in range(CAP):
        r, L = r0, 0
        while CONT[r]:
            r, L = (r + 1) % CAP, L + 1
        runs.append(L)
    assert runs == [1, 0, 5, 4, 3, 2, 1, 0, 0, 3, 2]
    for n in (2, 3, 5):
        assert any(L < n - 1 for L in runs) and any(L == n - 1 for L in runs) and any(L > n - 1 for L in runs)
    assert CONT[CAP - 1] and CONT[0] and set(IDX) == set(range(CAP)) and len(IDX) == B


@pytest.mark.parametrize("gamma", [0.99, 1.0])
@pytest.mark.parametrize("n", [1, 2, 3, 5])
@pytest.mark.parametrize("entry", ["compose", "stage"])
def test_kernel_against_the_restatement(ring, entry, n, gamma):
    from curla_amd import ops
    sc, host = ring["sc"], ring["host"]
    (blk, act, rew, nd), guards = _guarded([NBYTES, 4 * B * A, 4 * B, 4 * B])
    act, rew, nd = act.view(torch.float32), rew.view(torch.float32), nd.view(torch.float32)
    if entry == "compose":  # on a block that is already on the device
        blk.copy_(torch.from_numpy(host))
        ops.nstep_compose(blk, NR_OFF, ring["sc_d"], ring["cont_d"], CAP, n, gamma, B, A, act, rew, nd)
    else:                   # staged from a pinned block, composed in the same launch
        pinned = torch.from_numpy(host.copy()).pin_memory()
        ops.sample_stage_nstep(ops.host_device_pointer(pinned), blk, NBYTES, NR_OFF, ring["sc_d"], ring["cont_d"], CAP, n,
                               gamma, B, A, act, rew, nd)
    torch.cuda.synchronize()
    want_r, want_nd, last = walk_all(sc[:, A], sc[:, A + 1], CONT, CAP, n, gamma, IDX)
    got = blk.cpu().numpy()
    assert np.array_equal(rew.cpu().numpy(), want_r)
    assert np.array_equal(nd.cpu().numpy(), want_nd)
    assert np.array_equal(got[B * 8:2 * B * 8].view(np.int64), CAP + last)
    assert np.array_equal(got[NR_OFF:].view(np.int64), last)
    assert np.array_equal(act.cpu().numpy().reshape(B, A), sc[IDX, :A])
    # the sampled rows and the offset rows are what the host wrote; nothing outside the buffers was touched
    assert np.array_equal(got[:B * 8], host[:B * 8]) and np.array_equal(got[2 * B * 8:NR_OFF], host[2 * B * 8:NR_OFF])
    assert all(bool((g == GUARD_BYTE).all()) and g.numel() >= GUARD for g in guards)
    if n > 1:
        assert (last != np.array(IDX)).any() and (last < np.array(IDX)).any()  # walks happened, some across the wrap
    else:  # n = 1 is the plain gather and idx + capacity
        ga, gr, gn = (torch.empty(k, device="cuda") for k in (B * A, B, B))
        ops.gather_transition_scalars(ring["sc_d"], torch.tensor(IDX, device="cuda"), B, A, ga, gr, gn)
        assert torch.equal(ga, act) and torch.equal(gr, rew) and torch.equal(gn, nd)
        assert np.array_equal(got[B * 8:2 * B * 8], host[B * 8:2 * B * 8])


def test_entry_points_refuse_bad_arguments(ring):
    from curla_amd import _lib, ops
    (blk, act, rew, nd), _ = _guarded([NBYTES, 4 * B * A, 4 * B, 4 * B])
    blk.copy_(torch.from_numpy(ring["host"]))
    pinned = torch.from_numpy(ring["host"].copy()).pin_memory()
    hp = ops.host_device_pointer(pinned)
    good = dict(off=NR_OFF, cont=ring["cont_d"], cap=CAP, n=3)
    for bad in (dict(off=NR_OFF + 4), dict(cont=None), dict(cap=0), dict(n=0)):
        k = {**good, **bad}
        with pytest.raises(_lib.CurlaHipError, match="CURLA_ERR_ARG"):
            ops.nstep_compose(blk, k["off"], ring["sc_d"], k["cont"], k["cap"], k["n"], 0.99, B, A, act, rew, nd)
        with pytest.raises(_lib.CurlaHipError, match="CURLA_ERR_ARG"):
            ops.sample_stage_nstep(hp, blk, NBYTES, k["off"], ring["sc_d"], k["cont"], k["cap"], k["n"], 0.99, B, A, act,
                                   rew, nd)
    torch.cuda.synchronize()
    assert np.array_equal(blk.cpu().numpy(), ring["host"])  # nothing was launched


# ------------------------------------------------------------------------------------------------ buffer routes
STORES = {"one_allocation": dict(obs=(9, 20, 20), kw={}), "two_allocations": dict(obs=(3, 7, 9), kw={}),
          "dedup": dict(obs=(9, 20, 20), kw=dict(dedup_frames=True))}


def _augmentor(name, hw):
    import curla_amd
    if name == "random_crop":
        return curla_amd.RandomCrop(hw, (hw[0] - 4, hw[1] - 2))
    if name == "random_shift":
        return curla_amd.RandomShift(hw, 2)
    return curla_amd.make_augmentor(name, hw, None)


def _pixels(ref):
    """What a minibatch handle points at, as a float NCHW tensor."""
    from curla_amd import ops
    ref.check()
    if ref.is_u8 == 2:
        return ref.src.permute(0, 3, 1, 2).contiguous()
    t = torch.empty((ref.B, ref.C, ref.Hc, ref.Wc), dtype=torch.float32, device=ref.src.device)
    ops.crop_nchw(ref.src, ref.idx, ref.h1, ref.w1, ref.B, (ref.Hc, ref.Wc), out_f32=t)
    return t


@pytest.mark.parametrize("aug_name", ["random_crop", "random_shift", "identity", "color_jiggle"])
@pytest.mark.parametrize("store", list(STORES))
def test_next_obs_comes_from_the_bootstrap_row_on_every_route(store, aug_name):
    """Capacity 13, B = 8, episodes of 1 to 6 steps, 20 adds (the ring wraps) into an n_step=3 buffer and into a twin
    with n_step=1.  With the same forced parameters, the n-step sample's next_obs is the twin's 1-step next_obs of the
    rows r_last; obs, pos and the actions are the twin's of the sampled rows; rewards and not_dones are the
    restatement's.  Both APIs: the sample_cpc tensors and what the sample_cpc_refs handles point at."""
    from curla_amd import ReplayBuffer
    cfg = STORES[store]
    c, hw = cfg["obs"][0], cfg["obs"][1:]
    cap, Bb, n, gamma = 13, 8, 3, 0.99
    obs, act, rew, nxt, done, link = episodes((3, 1, 6, 2, 4, 4), ("done", "cut", "done", "cut", "done", "open"), hw=hw,
                                              k=c // 3, seed=3)
    aug = _augmentor(aug_name, hw)
    kw = dict(cfg["kw"], **(dict(staged_aug=True) if aug_name == "color_jiggle" else {}))
    dev = torch.device("cuda")
    X = ReplayBuffer(cfg["obs"], (2,), cap, Bb, dev, aug, n_step=n, discount=gamma, **kw)
    Y = ReplayBuffer(cfg["obs"], (2,), cap, Bb, dev, aug, **kw)
    assert (X._both is None) == (store == "two_allocations") if store != "dedup" else X.obses is None
    T = len(obs)
    assert T == 20
    for t in range(T):
        for rb in (X, Y):
            rb.add(obs[t], act[t], rew[t], nxt[t], done[t])
    # the flags on the device are the host mirror's, and the rule's
    want_flags = np.zeros(cap, dtype=np.uint8)
    for t in range(T):
        want_flags[t % cap] = link[t] if t < T - 1 else 0
    assert np.array_equal(X._cont_h, want_flags) and np.array_equal(X._cont.cpu().numpy(), want_flags)
    idxs = np.array([0, 5, 6, 7, 12, 3, 12, 9])  # row 6 is the newest (t = 19); 12 -> 0 crosses the ring's end
    rs = np.random.RandomState(1)
    offs = np.zeros((6, Bb), dtype=np.int32)
    if aug_name in ("random_crop", "random_shift"):
        offs = rs.randint(0, 3, (6, Bb)).astype(np.int32)
    sc = X._sc.cpu().numpy()
    want_r, want_nd, last = walk_all(sc[:, 2], sc[:, 3], want_flags, cap, n, gamma, idxs)
    assert (last != idxs).any() and (last == idxs).any() and last[4] == 1  # 12 -> 0 -> 1

    def sample(rb, rows, refs):
        torch.manual_seed(5)  # (ColorJiggle draws its parameters from torch's CPU generator)
        if not refs:
            return rb.sample_cpc(indices=(rows, offs))
        o, a, r, nx, d, kwargs = rb.sample_cpc_refs(indices=(rows, offs))
        out = [_pixels(ref) for ref in (o, nx, kwargs["obs_pos"])]
        if o.pair is not None:  # (obs | next_obs) as one handle of 2B: its second half is next_obs
            assert o.pair[0].B == 2 * Bb and torch.equal(_pixels(o.pair[0]), torch.cat([out[0], out[1]]))
        return out[0], a.clone(), r.clone(), out[1], d.clone(), dict(obs_pos=out[2])

    for refs in (False, True):
        o, a, r, nx, d, kwargs = sample(X, idxs, refs)
        o1, a1, _, _, _, kw1 = sample(Y, idxs, refs)
        _, _, _, nx_last, _, _ = sample(Y, last, refs)
        assert torch.equal(nx, nx_last)
        assert torch.equal(o, o1) and torch.equal(kwargs["obs_pos"], kw1["obs_pos"]) and torch.equal(a, a1)
        assert np.array_equal(r.cpu().numpy().reshape(-1), want_r) and np.array_equal(d.cpu().numpy().reshape(-1), want_nd)
        _, _, _, nx_plain, _, _ = sample(Y, idxs, refs)
        assert not torch.equal(nx, nx_plain)  # (the 1-step next_obs of the sampled rows is something else)


# ------------------------------------------------------------------------------------------------ whole update
def _agent(aug, out_hw, seed):
    import curla_amd
    curla_amd.set_seed_everywhere(seed)
    return curla_amd.CurlSacAgent((9,) + out_hw, (2,), torch.device("cuda"), aug, hidden_dim=64, **HP)


def test_update_equals_a_one_step_update_on_host_composed_rows():
    """X: n_step=3, fed an episode stream.  Y: n_step=1, row j = (obs_j, action_j, restated reward, restated not_done,
    next_obs of row r_last(j)).  Two agents with the same seed, 4 updates (even and odd steps) on the same injected
    indices: parameters, targets, Adam moments and log_alpha end bit-identical."""
    import curla_amd
    from tests.test_gpu_graph_aug import _state
    in_hw, out_hw, cap, Bb, n, gamma = (34, 40), (28, 34), 32, 8, 3, HP["discount"]
    obs, act, rew, nxt, done, link = episodes((5, 1, 7, 3, 2, 6), ("done", "cut", "done", "cut", "done", "open"), hw=in_hw,
                                              seed=4)
    T = len(obs)
    dev = torch.device("cuda")
    aug = curla_amd.RandomCrop(in_hw, out_hw)
    X = curla_amd.ReplayBuffer((9,) + in_hw, (2,), cap, Bb, dev, aug, n_step=n, discount=gamma)
    Y = curla_amd.ReplayBuffer((9,) + in_hw, (2,), cap, Bb, dev, aug)
    for t in range(T):
        X.add(obs[t], act[t], rew[t], nxt[t], done[t])
    flags = X._cont.cpu().numpy()
    assert flags[:T].tolist() == link[:T - 1].tolist() + [0]
    nd = 1.0 - done.astype(np.float32)
    want_r, want_nd, last = walk_all(rew, nd, flags, cap, n, gamma, np.arange(T))
    for t in range(T):
        Y.add(obs[t], act[t], 0.0, nxt[last[t]], False)
    Y.rewards[:T] = torch.from_numpy(want_r).to(dev).view(T, 1)
    Y.not_dones[:T] = torch.from_numpy(want_nd).to(dev).view(T, 1)
    rs = np.random.RandomState(2)
    draws = [(rs.randint(0, T, Bb), rs.randint(0, 7, (6, Bb)).astype(np.int32)) for _ in range(4)]
    states = []
    for rb in (X, Y):
        agent = _agent(aug, out_hw, 11)
        it = iter(draws)
        rb.draw_indices = lambda it=it: next(it)
        L = NullLogger()
        for step in range(4):
            agent.update(rb, L, step)
        torch.cuda.synchronize()
        states.append(_state(agent, rb))
    assert float(states[0]["critic_steps"][0]) == 4 and float(states[0]["actor_steps"][0]) == 2
    for k in states[0]:
        assert torch.equal(states[0][k], states[1][k]), k
    # ... and the n-step targets are not the 1-step ones: a 1-step buffer of the same stream ends elsewhere
    Z = curla_amd.ReplayBuffer((9,) + in_hw, (2,), cap, Bb, dev, aug)
    for t in range(T):
        Z.add(obs[t], act[t], rew[t], nxt[t], done[t])
    agent = _agent(aug, out_hw, 11)
    it = iter(draws)
    Z.draw_indices = lambda: next(it)
    for step in range(4):
        agent.update(Z, NullLogger(), step)
    torch.cuda.synchronize()
    assert not torch.equal(_state(agent, Z)["critic"], states[0]["critic"])


# ------------------------------------------------------------------------------------------------ graphs
@pytest.mark.parametrize("dedup", [False, True])
def test_graph_replay_of_an_n_step_buffer_is_the_eager_update(monkeypatch, dedup):
    """14 mixed steps as in tests/test_gpu_graph_aug.py (8, 9, 11, 12, 13 replay), n_step=3, RandomCrop, and three
    transitions added in front of step 10, i.e. between two replays: the replays read the flags when they run, so the
    graphed run ends where the eager run of the same stream ends, and a replayed step makes no kernel call."""
    import curla_amd
    import tests.test_gpu_graph_aug as G

    def build(aug, dedup_frames=False, B=64, seed=5):
        torch.manual_seed(seed)
        torch.cuda.manual_seed_all(seed)
        np.random.seed(seed)
        dev = torch.device("cuda")
        in_hw = (40, 44)
        augmentor = curla_amd.make_augmentor(aug, in_hw, (32, 36))
        agent = curla_amd.CurlSacAgent((9, 32, 36), (2,), dev, augmentor, hidden_dim=64, **{**HP, "log_interval": 5})
        rb = curla_amd.ReplayBuffer((9,) + in_hw, (2,), 512, B, dev, augmentor, dedup_frames=dedup_frames, n_step=3,
                                    discount=HP["discount"])
        rb.add_batch(*G._episode(400, 3, in_hw, 6))
        extra = G._episode(3, 3, in_hw, 8)
        update = agent.update

        def update_with_adds(rb_, L, step):
            if step == 10:
                for t in range(3):
                    rb_.add(extra[0][t], extra[1][t], extra[2][t], extra[3][t], extra[4][t])
            return update(rb_, L, step)
        agent.update = update_with_adds
        return agent, rb
    monkeypatch.setattr(G, "_build", build)
    setup = dict(aug="random_crop", dedup_frames=dedup)
    eager, calls_e, logs_e, _, rb_e = G._run(False, **setup)
    graph, calls_g, logs_g, agent, rb = G._run(True, **setup)
    replayed = [8, 9, 11, 12, 13]
    assert [sum(calls_g[s].values()) for s in replayed] == [0] * len(replayed), calls_g
    assert all(calls_e[s].get("curla_sample_stage_nstep") == 1 and not calls_e[s].get("curla_sample_stage")
               for s in range(14))
    assert calls_g[7].get("curla_sample_stage_nstep") == 1  # recorded by the capture
    assert len(agent._graphs) == 2 and all(len(r) == 2 and all(g["graph"] is not None for g in r)
                                           for r in agent._graphs.values())
    assert rb.idx == rb_e.idx == 403 and int(rb._cont.sum()) == int(rb._cont_h.sum()) > 300
    assert logs_e == logs_g
    for k in eager:
        assert torch.equal(eager[k], graph[k]), k
