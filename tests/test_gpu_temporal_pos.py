"""Temporal positives on the device (``ReplayBuffer(pos_offset=...)``): the chain walk against its NumPy restatement on
both entry points, alone and beside the n-step walk; the positive's pixels on every route a minibatch can take, against
a twin buffer without the keyword that is asked for the restated rows; whole updates against updates on hand-assembled
samples; graph replay against the eager run; persistence.

Everything is compared bit for bit: the walk moves indices, and the pixels it selects go through the kernels that the
twin's next_obs goes through."""
import numpy as np
import pytest
import torch

from tests.test_gpu_agent import HP, NullLogger
from tests.test_gpu_nstep import _guarded, _pixels, walk_all
from tests.test_nstep_host import episodes

pytestmark = pytest.mark.gpu


def walk(cont, capacity, k, t):
    """The restatement: the row whose next_obs is the positive of sampled row t, and the links it walked."""
    r, steps = int(t), 0
    for _ in range(k - 1):
        if not cont[r]:
            break
        r, steps = (r + 1) % capacity, steps + 1
    return r, steps


def rows_of(cont, capacity, k, idx):
    return np.array([walk(cont, capacity, k, t)[0] for t in idx], dtype=np.int64)


# ------------------------------------------------------------------------------------------------ the kernel
CAP, A, B = 11, 2, 8
#       row  0  1  2  3  4  5  6  7  8  9 10      runs of set flags: 9,10,0 (crosses the ring's end), 2..6, none at 1, 7, 8
CONT = [1, 0, 1, 1, 1, 1, 1, 0, 0, 1, 1]
HEAD = 8                                          # the write head: row 7 is the newest transition, its flag is 0
IDX = [9, 2, 6, 7, 10, 3, 1, 5]
KS = (1, 2, 3, 5)
NR_OFF = 2 * B * 8 + 6 * B * 4                    # idx int64 [2B] | offsets int32 [6][B] | next_row int64 [B] |
POS_OFF = NR_OFF + 8 * B                          # pos_row int64 [2][B] | pos_run int64 [3B]
RUN_OFF = POS_OFF + 16 * B
NBYTES = RUN_OFF + 24 * B
GUARD_BYTE = 0xA5


def test_the_fixture_holds_every_case():
    runs = []
    for r0 in IDX:
        r, L = r0, 0
        while CONT[r]:
            r, L = (r + 1) % CAP, L + 1
        runs.append(L)
    assert runs == [3, 5, 1, 0, 2, 4, 0, 2] and len(IDX) == B
    for k in KS[1:]:  # runs shorter than, equal to and longer than the k - 1 links of every k
        assert any(L < k - 1 for L in runs) and any(L == k - 1 for L in runs) and any(L > k - 1 for L in runs)
    assert CONT[CAP - 1] and CONT[0] and 9 in IDX and 10 in IDX    # a run across the ring's end, walked from two rows
    assert CONT[HEAD - 1] == 0 and HEAD - 1 in IDX                 # a start row directly behind the write head
    assert walk(CONT, CAP, 3, 10) == (1, 2) and walk(CONT, CAP, 5, 9) == (1, 3) and walk(CONT, CAP, 5, 7) == (7, 0)


@pytest.fixture(scope="module")
def ring():
    rs = np.random.RandomState(7)
    sc = rs.randn(CAP, A + 2).astype(np.float32)
    host = np.full(NBYTES, 0x77, dtype=np.uint8)
    i64 = host[:2 * B * 8].view(np.int64)
    i64[:B] = IDX
    i64[B:] = i64[:B] + CAP
    host[2 * B * 8:NR_OFF].view(np.int32)[:] = rs.randint(0, 9, 6 * B)
    dev = torch.device("cuda")
    return dict(sc=sc, host=host, sc_d=torch.from_numpy(sc).to(dev),
                cont_d=torch.tensor(CONT, dtype=torch.uint8, device=dev))


@pytest.mark.parametrize("with_run", [False, True])
@pytest.mark.parametrize("n", [None, 3])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("entry", ["walk", "stage"])
def test_kernel_against_the_restatement(ring, entry, k, n, with_run):
    """``n`` None: no n-step walk (the block's next_row region belongs to nobody).  3: combined with the n-step
    composition, gamma 0.99, whose outputs are held to tests/test_gpu_nstep.py's restatement."""
    from curla_amd import ops
    sc, host = ring["sc"], ring["host"]
    (blk, act, rew, nd), guards = _guarded([NBYTES, 4 * B * A, 4 * B, 4 * B])
    act, rew, nd = act.view(torch.float32), rew.view(torch.float32), nd.view(torch.float32)
    nr, run, gamma = (NR_OFF if n else None), (RUN_OFF if with_run else None), 0.99
    if entry == "walk":  # on a block that is already on the device, behind the composition where there is one
        blk.copy_(torch.from_numpy(host))
        if n:
            ops.nstep_compose(blk, NR_OFF, ring["sc_d"], ring["cont_d"], CAP, n, gamma, B, A, act, rew, nd)
        else:
            ops.gather_transition_scalars(ring["sc_d"], blk[:8 * B].view(torch.int64), B, A, act, rew, nd)
        ops.pos_walk(blk, POS_OFF, run, nr, ring["cont_d"], CAP, k, n or 1, B)
    else:                # staged from a pinned block, both walks in the same launch
        pinned = torch.from_numpy(host.copy()).pin_memory()
        ops.sample_stage_pos(ops.host_device_pointer(pinned), blk, NBYTES, nr, POS_OFF, run, ring["sc_d"], ring["cont_d"],
                             CAP, n or 1, gamma, k, B, A, act, rew, nd)
    torch.cuda.synchronize()
    got = blk.cpu().numpy()
    r = rows_of(CONT, CAP, k, IDX)
    want = host.copy()
    want[POS_OFF:RUN_OFF].view(np.int64)[:] = np.concatenate([r, CAP + r])
    want_r, want_nd, last = walk_all(sc[:, A], sc[:, A + 1], CONT, CAP, n or 1, gamma, IDX)
    if n:
        want[B * 8:2 * B * 8].view(np.int64)[:] = CAP + last
        want[NR_OFF:POS_OFF].view(np.int64)[:] = last
    if with_run:
        want[RUN_OFF:].view(np.int64)[:] = np.concatenate([IDX, CAP + last, CAP + r])
    # the walks' words bit-exact, every word they do not own as the host wrote it
    assert np.array_equal(got[POS_OFF:RUN_OFF].view(np.int64), want[POS_OFF:RUN_OFF].view(np.int64))
    assert np.array_equal(got, want)
    assert np.array_equal(rew.cpu().numpy(), want_r) and np.array_equal(nd.cpu().numpy(), want_nd)
    assert np.array_equal(act.cpu().numpy().reshape(B, A), sc[IDX, :A])
    assert all(bool((g == GUARD_BYTE).all()) and g.numel() >= 256 for g in guards)
    if k > 1:
        assert (r != np.array(IDX)).any() and (r < np.array(IDX)).any()  # walks happened, some across the ring's end
    else:
        assert np.array_equal(r, IDX)


def test_k_1_reads_no_flag(ring):
    """``cont`` may be NULL when nothing reads it: k = 1 without an n-step walk."""
    from curla_amd import ops
    (blk, act, rew, nd), guards = _guarded([NBYTES, 4 * B * A, 4 * B, 4 * B])
    act, rew, nd = act.view(torch.float32), rew.view(torch.float32), nd.view(torch.float32)
    pinned = torch.from_numpy(ring["host"].copy()).pin_memory()
    ops.sample_stage_pos(ops.host_device_pointer(pinned), blk, NBYTES, None, POS_OFF, RUN_OFF, ring["sc_d"], None, CAP, 1,
                         1.0, 1, B, A, act, rew, nd)
    torch.cuda.synchronize()
    staged = blk.cpu().numpy().copy()
    blk[POS_OFF:].fill_(0x11)
    ops.pos_walk(blk, POS_OFF, RUN_OFF, None, None, CAP, 1, 1, B)
    torch.cuda.synchronize()
    idx = np.array(IDX, dtype=np.int64)
    for got in (staged, blk.cpu().numpy()):
        assert np.array_equal(got[POS_OFF:RUN_OFF].view(np.int64), np.concatenate([idx, CAP + idx]))
        assert np.array_equal(got[RUN_OFF:].view(np.int64), np.concatenate([idx, CAP + idx, CAP + idx]))
        assert np.array_equal(got[:POS_OFF], ring["host"][:POS_OFF])
    assert all(bool((g == GUARD_BYTE).all()) for g in guards)


def test_entry_points_refuse_bad_arguments(ring):
    from curla_amd import _lib, ops
    (blk, act, rew, nd), guards = _guarded([NBYTES, 4 * B * A, 4 * B, 4 * B])
    act, rew, nd = act.view(torch.float32), rew.view(torch.float32), nd.view(torch.float32)
    blk.copy_(torch.from_numpy(ring["host"]))
    outs = [t.clone() for t in (act, rew, nd)]
    pinned = torch.from_numpy(ring["host"].copy()).pin_memory()
    hp = ops.host_device_pointer(pinned)
    good = dict(blk=blk, pos=POS_OFF, run=RUN_OFF, nr=NR_OFF, cont=ring["cont_d"], cap=CAP, k=3, n=3)
    both = [dict(pos=POS_OFF + 4), dict(run=RUN_OFF + 4),            # not 8-byte aligned
            dict(pos=8 * B), dict(pos=0), dict(run=8 * B),            # inside the idx run
            dict(pos=NR_OFF), dict(pos=NR_OFF - 8), dict(run=NR_OFF), dict(nr=POS_OFF + 8 * B),  # overlaps next_row
            dict(run=POS_OFF + 8 * B), dict(run=POS_OFF - 8),         # run overlaps pos
            dict(pos=-8), dict(run=-8), dict(nr=-8),
            dict(k=0), dict(k=-1), dict(n=0), dict(cap=0), dict(cont=None), dict(blk=None)]
    stage_only = [dict(pos=NBYTES - 8 * B, run=None), dict(pos=NBYTES, run=None), dict(run=NBYTES - 16 * B),  # past the end
                  dict(nr=None), dict(sc=None), dict(hp=None), dict(act=None)]  # (n = 3 needs a next_row region)
    for bad in both:
        a = {**good, **bad}
        with pytest.raises(_lib.CurlaHipError, match="CURLA_ERR_ARG"):
            ops.pos_walk(a["blk"], a["pos"], a["run"], a["nr"], a["cont"], a["cap"], a["k"], a["n"], B)
    for bad in both + stage_only:
        a = {**good, "sc": ring["sc_d"], "hp": hp, "act": act, **bad}
        with pytest.raises(_lib.CurlaHipError, match="CURLA_ERR_ARG"):
            ops.sample_stage_pos(a["hp"], a["blk"], NBYTES, a["nr"], a["pos"], a["run"], a["sc"], a["cont"], a["cap"],
                                 a["n"], 0.99, a["k"], B, A, a["act"], rew, nd)
    # the flags may only be missing when nothing reads them
    for k, n in ((2, 1), (1, 2)):
        with pytest.raises(_lib.CurlaHipError, match="CURLA_ERR_ARG"):
            ops.pos_walk(blk, POS_OFF, RUN_OFF, None, None, CAP, k, n, B)
    with pytest.raises(_lib.CurlaHipError, match="CURLA_ERR_ARG"):
        ops.sample_stage_pos(hp, blk, NBYTES, None, POS_OFF, None, ring["sc_d"], None, CAP, 1, 0.99, 2, B, A, act, rew, nd)
    torch.cuda.synchronize()
    assert np.array_equal(blk.cpu().numpy(), ring["host"])  # nothing was launched
    assert all(torch.equal(a, b) for a, b in zip(outs, (act, rew, nd)))
    assert all(bool((g == GUARD_BYTE).all()) for g in guards)


# ------------------------------------------------------------------------------------------------ buffer routes
STORES = {"one_allocation": dict(obs=(3, 4, 4), crop=(3, 3), kw={}), "two_allocations": dict(obs=(3, 11, 13), crop=(9, 11), kw={}),
          "dedup": dict(obs=(3, 4, 4), crop=(3, 3), kw=dict(dedup_frames=True))}
LENGTHS, ENDS = (3, 1, 6, 2, 4, 4), ("done", "cut", "done", "cut", "done", "open")
ROUTE_CAP, ROUTE_B, ROUTE_SEED = 13, 8, 25


def _augmentor(name, cfg):
    import curla_amd
    hw = cfg["obs"][1:]
    if name == "random_crop":
        return curla_amd.RandomCrop(hw, cfg["crop"])
    if name == "random_shift":
        return curla_amd.RandomShift(hw, 2)
    return curla_amd.make_augmentor(name, hw, None)


def _stream(cfg):
    return episodes(LENGTHS, ENDS, hw=cfg["obs"][1:], k=cfg["obs"][0] // 3, seed=3)


def _flags(link, cap, T):
    flags = np.zeros(cap, dtype=np.uint8)
    for t in range(T):
        flags[t % cap] = link[t] if t < T - 1 else 0
    return flags


def _pair(store, aug_name, cap=ROUTE_CAP, adds=20, **x_kw):
    """Buffer X (``x_kw``) and its twin Y without pos_offset, fed the same 20 transitions (episodes of 1 to 6 steps, a
    done, truncations, the ring of 13 wraps); the flags the stream gives by the rule."""
    from curla_amd import ReplayBuffer
    cfg = STORES[store]
    aug = _augmentor(aug_name, cfg)
    kw = dict(cfg["kw"], **(dict(staged_aug=True) if aug_name == "color_jiggle" else {}))
    dev = torch.device("cuda")
    y_kw = {k: v for k, v in x_kw.items() if k not in ("pos_offset", "prioritized")}
    X = ReplayBuffer(cfg["obs"], (2,), cap, ROUTE_B, dev, aug, **kw, **x_kw)
    Y = ReplayBuffer(cfg["obs"], (2,), cap, ROUTE_B, dev, aug, **kw, **y_kw)
    assert (X.obses is None) if store == "dedup" else ((X._both is None) == (store == "two_allocations"))
    obs, act, rew, nxt, done, link = _stream(cfg)
    assert len(obs) == 20 and min(LENGTHS) == 1 and max(LENGTHS) == 6
    for t in range(adds):
        for rb in (X, Y):
            rb.add(obs[t], act[t], rew[t], nxt[t], done[t])
    return X, Y, _flags(link, cap, adds)


def _draw(aug_name, cfg, seed=ROUTE_SEED):
    """(idxs, offs) of one minibatch, drawn once: rows from the ring of 13, offsets inside what the augmentation draws."""
    rs = np.random.RandomState(seed)
    idxs = rs.randint(0, ROUTE_CAP, ROUTE_B)
    offs = np.zeros((6, ROUTE_B), dtype=np.int32)
    if aug_name == "random_crop":
        hw, crop = cfg["obs"][1:], cfg["crop"]
        offs[0::2] = rs.randint(0, hw[0] - crop[0] + 1, (3, ROUTE_B))
        offs[1::2] = rs.randint(0, hw[1] - crop[1] + 1, (3, ROUTE_B))
    elif aug_name == "random_shift":
        offs = rs.randint(0, 5, (6, ROUTE_B)).astype(np.int32)
    return idxs, offs


def _pos_as_next(offs):
    """The offsets of a twin's sample whose next_obs slot carries the positive's offset rows."""
    out = offs.copy()
    out[2], out[3] = offs[4], offs[5]
    return out


def _sample(rb, rows, offs, pos_params_as_next=False):
    """One sample_cpc_refs as (obs, next_obs, pos pixels, actions, rewards, not_dones, obs handle).  A staged float
    augmentation draws its parameters from torch's CPU generator, re-seeded here: every call draws the same three sets;
    ``pos_params_as_next`` hands the third set (the positive's) to the next_obs slot."""
    torch.manual_seed(5)
    draw_aug = rb.draw_aug
    if pos_params_as_next and rb.staged_aug:
        def swapped():
            drawn = draw_aug()
            return [drawn[0], drawn[2], drawn[2]]
        rb.draw_aug = swapped
    try:
        o, a, r, nx, d, kwargs = rb.sample_cpc_refs(indices=(rows, offs))
    finally:
        if "draw_aug" in vars(rb):
            del rb.draw_aug
    assert kwargs["obs_anchor"] is o and kwargs["time_anchor"] is None and kwargs["time_pos"] is None
    px = [_pixels(ref) for ref in (o, nx, kwargs["obs_pos"])]
    if o.pair is not None:  # (obs | next_obs) as one handle of 2B: unchanged by the positive
        assert o.pair[0].B == 2 * ROUTE_B and torch.equal(_pixels(o.pair[0]), torch.cat([px[0], px[1]]))
    return px[0], px[1], px[2], a.clone(), r.clone(), d.clone(), o


def test_the_drawn_minibatch_holds_every_case():
    """Plain NumPy: the minibatch of seed 25 on the stream's flags, for the k = 3 of the route tests."""
    _, _, _, _, _, link = _stream(STORES["one_allocation"])
    flags = _flags(link, ROUTE_CAP, 20)
    assert flags.tolist() == [1, 1, 0, 1, 1, 1, 0, 1, 1, 0, 1, 0, 1]
    idxs, _ = _draw("identity", STORES["one_allocation"])
    assert idxs.tolist() == [4, 10, 6, 7, 12, 2, 8, 12]
    walked = [walk(flags, ROUTE_CAP, 3, t) for t in idxs]
    r, steps = np.array([w[0] for w in walked]), np.array([w[1] for w in walked])
    assert r.tolist() == [6, 11, 6, 9, 1, 2, 9, 1]
    assert (r != idxs).sum() >= 2 and (steps < 2).sum() >= 2 and (r < idxs).sum() >= 1
    assert 6 in idxs and 19 % ROUTE_CAP == 6  # the newest row: nothing to walk to


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("aug_name", ["random_crop", "random_shift", "identity", "color_jiggle"])
@pytest.mark.parametrize("store", list(STORES))
def test_the_positive_is_next_obs_of_the_restated_row_on_every_route(store, aug_name, k):
    """X (pos_offset=k) samples (idxs, offs).  Its twin Y samples the restated rows r with the positive's offsets (and,
    staged, its parameters) in the next_obs slot: X's positive is Y's next_obs, bit for bit.  X's obs, next_obs and
    scalars are Y's of (idxs, offs).  sample_cpc materialises what the handles point at."""
    cfg = STORES[store]
    X, Y, flags = _pair(store, aug_name, pos_offset=k)
    assert X.pos_offset == k and hasattr(X, "_cont") == (k > 1)
    if k > 1:
        assert np.array_equal(X._cont.cpu().numpy(), flags) and np.array_equal(X._cont_h, flags)
    idxs, offs = _draw(aug_name, cfg)
    r = rows_of(flags, ROUTE_CAP, k, idxs)
    assert (r != idxs).sum() >= 2 if k > 1 else np.array_equal(r, idxs)
    ox, nx, px, ax, rx, dx, _ = _sample(X, idxs, offs)
    o0, n0, p0, a0, r0, d0, _ = _sample(Y, idxs, offs)
    assert torch.equal(ox, o0) and torch.equal(nx, n0)
    assert torch.equal(ax, a0) and torch.equal(rx, r0) and torch.equal(dx, d0)
    assert not torch.equal(px, p0)  # (an augmentation of obs[t] is something else)
    _, n_r, _, _, _, _, _ = _sample(Y, r, _pos_as_next(offs), pos_params_as_next=True)
    assert torch.equal(px, n_r)
    # the materialised, reference-typed tensors
    torch.manual_seed(5)
    o, a, rw, nxt, d, kwargs = X.sample_cpc(indices=(idxs, offs))
    assert torch.equal(kwargs["obs_pos"], px) and torch.equal(o, ox) and torch.equal(nxt, nx)
    assert torch.equal(a, ax) and torch.equal(rw, rx) and torch.equal(d, dx) and kwargs["obs_anchor"] is o


@pytest.mark.parametrize("store", list(STORES))
def test_k_equal_n_makes_the_positive_the_bootstrap_frame(store):
    """n_step=3 and pos_offset=3 walk the same links: with the positive's offsets set to next_obs's, the two handles
    point at identical pixels -- and the n-step scalars are what they are without a positive."""
    cfg = STORES[store]
    X, Y, flags = _pair(store, "random_crop", n_step=3, discount=0.99, pos_offset=3)
    assert Y.n_step == 3 and Y.pos_offset == 0
    idxs, offs = _draw("random_crop", cfg)
    offs[4], offs[5] = offs[2], offs[3]
    ox, nx, px, ax, rx, dx, _ = _sample(X, idxs, offs)
    o0, n0, p0, a0, r0, d0, _ = _sample(Y, idxs, offs)
    assert torch.equal(px, nx) and not torch.equal(px, p0)
    assert torch.equal(ox, o0) and torch.equal(nx, n0) and torch.equal(rx, r0) and torch.equal(dx, d0)
    sc = X._sc.cpu().numpy()
    want_r, want_nd, last = walk_all(sc[:, 2], sc[:, 3], flags, ROUTE_CAP, 3, 0.99, idxs)
    assert np.array_equal(rx.cpu().numpy().reshape(-1), want_r) and np.array_equal(dx.cpu().numpy().reshape(-1), want_nd)
    assert np.array_equal(last, rows_of(flags, ROUTE_CAP, 3, idxs))


@pytest.mark.parametrize("aug_name", ["random_crop", "random_shift"])
def test_a_prioritized_buffer_walks_from_the_drawn_rows(aug_name):
    """The rows are drawn on the device: read back from obs.per.rows, their restated positives are what the twin gives."""
    cfg = STORES["one_allocation"]
    X, Y, flags = _pair("one_allocation", aug_name, prioritized=True, pos_offset=2)
    _, offs = _draw(aug_name, cfg)
    u = (np.arange(ROUTE_B) + np.random.RandomState(3).random_sample(ROUTE_B)) / ROUTE_B
    ox, nx, px, ax, rx, dx, handle = _sample(X, u, offs)
    rows = handle.per.rows.cpu().numpy()
    assert rows.min() >= 0 and rows.max() < ROUTE_CAP and len(set(rows.tolist())) >= 4
    r = rows_of(flags, ROUTE_CAP, 2, rows)
    assert (r != rows).sum() >= 2 and (r == rows).sum() >= 1
    o0, n0, _, a0, r0, d0, _ = _sample(Y, rows, offs)
    assert torch.equal(ox, o0) and torch.equal(nx, n0) and torch.equal(ax, a0) and torch.equal(rx, r0)
    _, n_r, _, _, _, _, _ = _sample(Y, r, _pos_as_next(offs))
    assert torch.equal(px, n_r)


def test_save_and_load_keep_the_positives(tmp_path):
    """A buffer that loads what another saved rebuilds the flags: the same injected sample has the same pixels."""
    from curla_amd import ReplayBuffer
    cfg = STORES["one_allocation"]
    aug = _augmentor("random_crop", cfg)
    dev = torch.device("cuda")
    mk = lambda: ReplayBuffer(cfg["obs"], (2,), 32, ROUTE_B, dev, aug, pos_offset=3)  # noqa: E731
    obs, act, rew, nxt, done, link = _stream(cfg)
    X = mk()
    for t in range(20):
        X.add(obs[t], act[t], rew[t], nxt[t], done[t])
        if t in (7, 19):
            X.save(str(tmp_path))
    fresh = mk()
    fresh.load(str(tmp_path))
    assert fresh.idx == 20 and torch.equal(fresh._cont, X._cont) and np.array_equal(fresh._cont_h, X._cont_h)
    assert X._cont_h[:20].tolist() == link[:19].tolist() + [0]
    rs = np.random.RandomState(1)
    idxs, offs = rs.randint(0, 20, ROUTE_B), rs.randint(0, 2, (6, ROUTE_B)).astype(np.int32)
    r = rows_of(X._cont_h, 32, 3, idxs)
    assert (r != idxs).sum() >= 2
    a, b = _sample(X, idxs, offs), _sample(fresh, idxs, offs)
    for j in range(3):
        assert torch.equal(a[j], b[j]), j
    assert not torch.equal(a[0], a[2])


# ------------------------------------------------------------------------------------------------ whole update
def test_update_equals_an_update_on_hand_assembled_samples():
    """The golden tiny agent, three updates.  X: pos_offset=2, ``agent.update``.  Y: the twin without the keyword,
    ``_update_phases`` on (obs, action, reward, next_obs, not_done) of the sampled rows and, as the positive, the next_obs
    handle of a second sample at the restated rows with the positive's offsets.  Parameters, Adam moments and every logged
    loss end bit-identical -- and the CURL loss is not the one of a pos_offset=0 run."""
    import curla_amd
    from tests._util import load
    from tests.test_gpu_agent import _tiny_agent
    from tests.test_gpu_graph_aug import _episode, _state
    in_hw, cap, Bb, k = (34, 40), 64, 8, 2
    ep = _episode(48, 3, in_hw, 6)
    rs = np.random.RandomState(2)
    draws = [(rs.randint(0, 48, Bb), rs.randint(0, 7, (6, Bb)).astype(np.int32)) for _ in range(3)]
    dev = torch.device("cuda")

    def start(**kw):
        agent, aug = _tiny_agent(load("tiny.npz"))
        torch.manual_seed(7)
        torch.cuda.manual_seed_all(7)
        np.random.seed(7)
        rb = curla_amd.ReplayBuffer((9,) + in_hw, (2,), cap, Bb, dev, aug, **kw)
        rb.add_batch(*ep)
        return agent, rb

    def run_update(**kw):
        agent, rb = start(**kw)
        it = iter(draws)
        rb.draw_indices = lambda: next(it)
        logs = []
        for step in range(3):
            L = NullLogger()
            agent.update(rb, L, step)
            logs.append(dict(L.scalars))
        torch.cuda.synchronize()
        return _state(agent, rb), logs, rb

    state_x, logs_x, X = run_update(pos_offset=k)
    flags = X._cont.cpu().numpy()
    assert flags[:48].sum() > 30 and not flags[47] and not flags[6]  # an episode ends every 7th step
    agent, Y = start()
    logs_y = []
    for step, (idxs, offs) in enumerate(draws):
        r = rows_of(flags, cap, k, idxs)
        assert (r != idxs).sum() >= 4 and (step == 0 or (r == idxs).any())  # (draws 1 and 2 hold an episode's last row)
        obs, act, rew, nxt, nd, _ = Y.sample_cpc_refs(indices=(idxs, offs))
        _, _, _, pos, _, _ = Y.sample_cpc_refs(indices=(r, _pos_as_next(offs)))
        L = NullLogger()
        agent._update_phases((obs, act, rew, nxt, nd, dict(obs_anchor=obs, obs_pos=pos, time_anchor=None, time_pos=None)),
                             L, step)
        logs_y.append(dict(L.scalars))
    torch.cuda.synchronize()
    state_y = _state(agent, Y)
    assert float(state_x["critic_steps"][0]) == 3 and float(state_x["cpc_steps"][0]) >= 1
    assert "train/curl_loss" in logs_x[0] and logs_x == logs_y
    for name in state_x:
        assert torch.equal(state_x[name], state_y[name]), name
    # not vacuous: the same draws with the positive an augmentation of obs give another CURL loss
    state_0, logs_0, _ = run_update()
    assert logs_0[0]["train/curl_loss"] != logs_x[0]["train/curl_loss"]
    assert logs_0[0]["train_critic/loss"] == logs_x[0]["train_critic/loss"]
    assert not torch.equal(state_0["critic"], state_x["critic"])


# ------------------------------------------------------------------------------------------------ graphs
@pytest.mark.parametrize("dedup", [False, True])
@pytest.mark.parametrize("n_step", [1, 3])
def test_graph_replay_of_a_temporal_positive_is_the_eager_update(monkeypatch, n_step, dedup):
    """14 mixed steps as in tests/test_gpu_nstep.py (8, 9, 11, 12, 13 replay), pos_offset=3, RandomCrop, three
    transitions added between two replays: the walk is a node of the captured graph and reads the flags when it runs."""
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
        kw = dict(n_step=n_step, discount=HP["discount"]) if n_step > 1 else {}
        rb = curla_amd.ReplayBuffer((9,) + in_hw, (2,), 512, B, dev, augmentor, dedup_frames=dedup_frames, pos_offset=3,
                                    **kw)
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
    assert all(calls_e[s].get("curla_sample_stage_pos") == 1 and not calls_e[s].get("curla_sample_stage")
               and not calls_e[s].get("curla_sample_stage_nstep") and not calls_e[s].get("curla_pos_walk")
               and calls_e[s].get("curla_gather_stacks", 0) == (3 if dedup else 0) for s in range(14))
    assert calls_g[7].get("curla_sample_stage_pos") == 1  # recorded by the capture
    assert len(agent._graphs) == 2 and all(len(r) == 2 and all(g["graph"] is not None for g in r)
                                           for r in agent._graphs.values())
    assert rb.idx == rb_e.idx == 403 and int(rb._cont.sum()) == int(rb._cont_h.sum()) > 300
    assert logs_e == logs_g
    for name in eager:
        assert torch.equal(eager[name], graph[name]), name
    blocks = rb._graph_blocks
    assert len(blocks) == 4
    for g in blocks.values():
        assert len(g["guards"]) == (2 if dedup else 0)
        for guard in g["guards"]:
            assert guard.numel() >= rb.GUARD and bool((guard == rb.GUARD_BYTE).all())
        if dedup:  # | obs | next_obs | pos stacks; the 32 bytes of loader slack behind them are read, never written
            assert g["mb_u8"].numel() == 3 * 64 * rb._frame + 32 and not bool(g["mb_u8"][-32:].any())
            assert bool(g["mb_u8"][2 * 64 * rb._frame:-32].any())
