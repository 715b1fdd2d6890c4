"""Host side of ``ReplayBuffer(pos_offset=...)`` without a GPU (``device="cpu"`` buffers and the launch-trace hook, which
computes nothing): the constructor, that a buffer with ``pos_offset=0`` is the buffer without the keyword, the
continuity flags that a positive more than one step ahead keeps without n-step returns, the block layout and the launch
schedule of a sample on every route."""
import numpy as np
import pytest
import torch

import curla_amd
from curla_amd import _lib
from curla_amd.utils import ReplayBuffer
from tests.test_nstep_host import SCRIPT, episodes, expected_flags

C, HW, A = 9, (20, 20), 2


def walk(cont, capacity, k, t):
    """The restatement: the row whose next_obs is the positive of sampled row t."""
    r = int(t)
    for _ in range(k - 1):
        if not cont[r]:
            break
        r = (r + 1) % capacity
    return r


def _augmentor(kind):
    return {"ring": lambda: curla_amd.RandomCrop(HW, (16, 16)), "scratch": lambda: curla_amd.RandomShift(HW, 2),
            "float": lambda: curla_amd.ColorJiggle(HW)}[kind]()


def _buffer(capacity, kind="ring", B=4, **kw):
    if kw.get("n_step", 1) > 1:
        kw.setdefault("discount", 0.99)
    if kind == "float":
        kw.setdefault("staged_aug", True)
    return ReplayBuffer((C,) + HW, (A,), capacity, B, "cpu", _augmentor(kind), **kw)


def _filled(capacity=16, **kw):
    obs, act, rew, nxt, done, _ = episodes(**SCRIPT)
    rb = _buffer(capacity, **kw)
    for t in range(12):
        rb.add(obs[t], act[t], rew[t], nxt[t], done[t])
    # a CPU buffer has no pinned index slots; stand in for their device addresses so that sampling takes the route of a
    # device buffer (the staging kernel) under the trace hook -- as a prioritized buffer never does
    if not rb.prioritized:
        rb._h_index_dev = [4096 * (k + 1) for k in range(rb._n_slots)]
    return rb


def _traced(fn):
    calls = []
    _lib.set_trace_hook(lambda name, args: calls.append((name, args)))
    try:
        torch.manual_seed(3)  # (a float augmentation draws its parameters from torch's CPU generator)
        fn()
    finally:
        _lib.set_trace_hook(None)
    return calls


def _relative(rb, trace):
    """A launch trace with every address inside one of the buffer's own allocations replaced by (attribute, offset), and
    every other address (a tensor allocated for the call) by a placeholder: two buffers of the same construction then
    give the same list."""
    bases = sorted((t.data_ptr(), t.numel() * t.element_size(), name) for name, t in vars(rb).items()
                   if isinstance(t, torch.Tensor) and t.numel() and t._base is None)
    out = []
    for name, args in trace:
        row = []
        for a in args:
            hit = [(nm, a - lo) for lo, size, nm in bases if isinstance(a, int) and lo <= a < lo + size]
            row.append(hit[0] if hit else "<fresh>" if isinstance(a, int) and a >= 1 << 32 else a)
        out.append((name, tuple(row)))
    return out


def _idx(B=4, rows=6):
    return np.array([0, 5, 11, 3][:B]), np.zeros((rows, B), dtype=np.int32)


# ---------------------------------------------------------------------------------------------------- constructor
def test_constructor_validation():
    for bad in (-1, True, False, 1.5, 2.0, "2", None):
        with pytest.raises(ValueError, match="pos_offset"):
            _buffer(8, pos_offset=bad)
    rb = _buffer(8, pos_offset=3)
    assert rb.pos_offset == 3 and type(rb.pos_offset) is int
    assert _buffer(8, pos_offset=np.int64(2)).pos_offset == 2
    assert _buffer(8).pos_offset == 0 and _buffer(8, pos_offset=0).pos_offset == 0
    with pytest.raises(AttributeError):
        rb.pos_offset = 1  # it decides the block layout: fixed at construction
    assert rb.pos_offset == 3


# ---------------------------------------------------------------------------------------------------- off is unchanged
@pytest.mark.parametrize("n_step", [1, 3])
@pytest.mark.parametrize("store", [dict(), dict(dedup_frames=True)])
@pytest.mark.parametrize("kind", ["ring", "scratch", "float"])
def test_pos_offset_0_is_the_buffer_as_it_was(kind, store, n_step):
    default = _filled(kind=kind, n_step=n_step, **store)
    zero = _filled(kind=kind, n_step=n_step, pos_offset=0, **store)
    lay = zero.block_layout()
    assert lay == default.block_layout() and "pos_row" not in lay and "pos_run" not in lay
    shapes = lambda rb: {k: (tuple(v.shape), v.dtype) for k, v in vars(rb).items()  # noqa: E731
                         if isinstance(v, (torch.Tensor, np.ndarray))}
    assert shapes(zero) == shapes(default)  # every allocation, name by name
    assert hasattr(zero, "_cont") == (n_step > 1)
    slot_shapes = lambda rb: [{k: tuple(v.shape) for k, v in s.items() if isinstance(v, torch.Tensor)}  # noqa: E731
                              for s in rb._sample_slots]
    assert slot_shapes(zero) == slot_shapes(default)
    idx = _idx()
    t0 = _traced(lambda: zero.sample_cpc_refs(indices=idx))
    td = _traced(lambda: default.sample_cpc_refs(indices=idx))
    assert [n for n, _ in t0][0] == ("curla_sample_stage_nstep" if n_step > 1 else "curla_sample_stage")
    assert not {"curla_pos_walk", "curla_sample_stage_pos"} & {n for n, _ in t0}
    assert _relative(zero, t0) == _relative(default, td)
    n = lay.get("next_row", lay["nbytes"])  # (next_row is the device's to write: the host leaves it as allocated)
    assert torch.equal(zero._h_index[0, :n], default._h_index[0, :n])  # the pinned block holds the same bytes
    # the copy route and a graph slot as well
    zero._h_index_dev = default._h_index_dev = None
    t0 = _traced(lambda: zero.sample_cpc_refs(indices=idx))
    td = _traced(lambda: default.sample_cpc_refs(indices=idx))
    assert _relative(zero, t0) == _relative(default, td) and "curla_pos_walk" not in [n for n, _ in t0]
    _traced(lambda: (zero.graph_block(0), default.graph_block(0)))  # (the pinned block's device address: a call)
    g0, gd = zero.graph_block(0), default.graph_block(0)
    assert {k: tuple(v.shape) for k, v in g0.items() if isinstance(v, torch.Tensor)} \
        == {k: tuple(v.shape) for k, v in gd.items() if isinstance(v, torch.Tensor)}


# ---------------------------------------------------------------------------------------------------- flags
@pytest.mark.parametrize("dedup", [False, True])
def test_a_positive_three_steps_ahead_keeps_the_flags_of_n_step_3(dedup, tmp_path):
    """Capacity 7, 12 adds (the ring wraps): a done, a truncation (done=False, reset frame next), an open episode.
    ``pos_offset=3, n_step=1`` keeps exactly the flags ``n_step=3`` keeps -- through add, add_batch (one longer than
    the ring included) and save / load."""
    obs, act, rew, nxt, done, link = episodes(**SCRIPT)
    assert done[0] and not done[2] and not np.array_equal(nxt[2], obs[3])  # a done; a truncation only the bytes tell
    P, N = _buffer(7, pos_offset=3, dedup_frames=dedup), _buffer(7, n_step=3, dedup_frames=dedup)
    assert P.n_step == 1 and P.discount is None
    for t in range(12):
        for rb in (P, N):
            rb.add(obs[t], act[t], rew[t], nxt[t], done[t])
        assert np.array_equal(P._cont_h, expected_flags(link, 7, t)), t
        assert np.array_equal(P._cont_h, N._cont_h) and np.array_equal(P._cont.numpy(), P._cont_h)
    assert P.full and P.idx == 5 and P._cont_h.tolist() == [0, 1, 1, 1, 0, 1, 1]
    # add_batch: cuts inside an episode and at episode ends, then one bulk write longer than the ring
    bulk = _buffer(7, pos_offset=3, dedup_frames=dedup)
    for lo, hi in ((0, 2), (2, 3), (3, 9), (9, 12)):
        bulk.add_batch(obs[lo:hi], act[lo:hi], rew[lo:hi], nxt[lo:hi], done[lo:hi])
        assert np.array_equal(bulk._cont_h, expected_flags(link, 7, hi - 1)), (lo, hi)
    assert np.array_equal(bulk._cont.numpy(), N._cont_h)
    long = _buffer(7, pos_offset=3, dedup_frames=dedup)
    long.add(obs[0], act[0], rew[0], nxt[0], done[0])
    long.add_batch(obs[1:], act[1:], rew[1:], nxt[1:], done[1:])
    assert np.array_equal(long._cont_h, N._cont_h) and np.array_equal(long._cont.numpy(), N._cont_h)
    if dedup:  # (saving a frame store gathers its stacks with a kernel; its load() is add_batch, covered above)
        return
    # save / load: the flags are rebuilt from the payload
    big_p, big_n = _buffer(16, pos_offset=3), _buffer(16, n_step=3)
    for t in range(12):
        for rb in (big_p, big_n):
            rb.add(obs[t], act[t], rew[t], nxt[t], done[t])
        if t in (4, 11):
            big_p.save(str(tmp_path))
    fresh = _buffer(16, pos_offset=3)
    fresh.load(str(tmp_path))
    assert fresh.idx == 12 and np.array_equal(fresh._cont_h, big_n._cont_h)
    assert np.array_equal(fresh._cont.numpy(), big_n._cont_h) and big_n._cont_h[:12].tolist() == link[:11].tolist() + [0]
    store = _buffer(16, pos_offset=3, dedup_frames=True)  # the same files into a frame store
    store.load(str(tmp_path))
    assert np.array_equal(store._cont_h, big_n._cont_h)


@pytest.mark.parametrize("dedup", [False, True])
def test_a_positive_one_step_ahead_keeps_no_flags(dedup):
    rb = _filled(pos_offset=1, dedup_frames=dedup)
    for attr in ("_cont", "_cont_h", "_last_next", "_chain", "_cont_off"):
        assert not hasattr(rb, attr)
    assert rb._d_add.numel() == _filled(dedup_frames=dedup)._d_add.numel()  # no flag bytes in the add block
    t = _traced(lambda: rb.sample_cpc_refs(indices=_idx()))
    a = t[0][1]
    assert t[0][0] == "curla_sample_stage_pos" and a[7] is None and (a[9], a[11]) == (1, 1)  # cont, n, k
    rb._h_index_dev = None
    t = _traced(lambda: rb.sample_cpc_refs(indices=_idx()))
    walks = [args for n, args in t if n == "curla_pos_walk"]
    assert len(walks) == 1 and walks[0][4] is None and (walks[0][6], walks[0][7]) == (1, 1)


# ---------------------------------------------------------------------------------------------------- layout
@pytest.mark.parametrize("B", [4, 5])
@pytest.mark.parametrize("kind", ["ring", "scratch", "float"])
def test_layout(kind, B):
    for extra in (dict(), dict(n_step=3), dict(prioritized=True), dict(n_step=3, prioritized=True)):
        off = _buffer(16, kind=kind, B=B, **extra).block_layout()
        assert "pos_row" not in off and "pos_run" not in off and off["nbytes"] % 8 == 0
        for k in (1, 3):
            lay = _buffer(16, kind=kind, B=B, pos_offset=k, **extra).block_layout()
            assert lay["nbytes"] % 8 == 0 and lay["pos_row"] % 8 == 0 and lay["tail"] == lay["nbytes"]
            assert ("pos_run" in lay) == (kind == "scratch")
            assert lay["nbytes"] == off["nbytes"] + 16 * B + (24 * B if kind == "scratch" else 0)
            # behind next_row, in front of the prioritized fields, nothing overlapping
            fields = [("pos_row", 16 * B)] + [("pos_run", 24 * B)] * (kind == "scratch")
            if "next_row" in lay:
                assert lay["next_row"] == off["next_row"] and lay["pos_row"] == lay["next_row"] + 8 * B
            else:
                assert lay["pos_row"] == off.get("u", off["nbytes"])
            if "u" in lay:
                assert lay["u"] == lay[fields[-1][0]] + fields[-1][1] and lay["u"] % 8 == 0
            if kind == "scratch":
                assert lay["pos_run"] == lay["pos_row"] + 16 * B
            for key in ("idx", "offs", "offs_end", "aug", "aug_stride", "cut"):
                assert lay.get(key) == off.get(key)


# ---------------------------------------------------------------------------------------------------- launches
def _names(trace):
    return [n for n, _ in trace]


@pytest.mark.parametrize("n_step", [1, 3])
@pytest.mark.parametrize("store", [dict(), dict(dedup_frames=True)])
@pytest.mark.parametrize("kind", ["ring", "scratch", "float"])
def test_a_temporal_positive_launches_as_many_kernels(kind, store, n_step):
    """Pinned-in-place route: the staging launch changes its name and nothing is added -- but for the frame store's
    third gather.  Copy route: the same plus ONE stand-alone walk, behind the composition and in front of everything
    that reads pixels.  A graph slot records what the rotating slots launch."""
    off = _filled(kind=kind, n_step=n_step, **store)
    on = _filled(kind=kind, n_step=n_step, pos_offset=3, **store)
    B, lay = 4, on.block_layout()
    idx = _idx()
    t_off = _traced(lambda: off.sample_cpc_refs(indices=idx))
    t_on = _traced(lambda: on.sample_cpc_refs(indices=idx))
    stage = "curla_sample_stage_nstep" if n_step > 1 else "curla_sample_stage"
    assert _names(t_off)[0] == stage and _names(t_on)[0] == "curla_sample_stage_pos"
    assert _names(t_on).count("curla_gather_stacks") == _names(t_off).count("curla_gather_stacks") + (1 if store else 0)
    assert _names(t_on).count("curla_gather_stacks") == (3 if store else 0)
    rest = lambda names: [n for n in names[1:] if n != "curla_gather_stacks"]  # noqa: E731
    assert rest(_names(t_on)) == rest(_names(t_off)) and len(t_on) == len(t_off) + (1 if store else 0)
    a = t_on[0][1]
    blk = on._d_index[on._sample_slot]
    assert (a[1], a[2], a[3], a[4], a[5]) == (blk.data_ptr(), lay["nbytes"], lay.get("next_row", -1), lay["pos_row"],
                                              lay.get("pos_run", -1))
    assert (a[7], a[8], a[9], a[11], a[12], a[13]) == (on._cont.data_ptr(), 16, n_step, 3, B, A)
    if store:  # the third gather: next_obs frame ids at the positive's rows, into the third run of the [3B] store
        g = [args for n, args in t_on if n == "curla_gather_stacks"]
        mb = on._mb_store[on._sample_slot]
        assert mb.numel() == 3 * B * C * HW[0] * HW[1] + 32 and off._mb_store.shape[1] == 2 * B * C * HW[0] * HW[1] + 32
        assert g[2][1] == g[1][1] == on._fid[:, 1, :].data_ptr() and g[0][1] == on._fid.data_ptr()
        assert g[2][3] == blk.data_ptr() + lay["pos_row"]
        assert [x[-2] for x in g] == [mb.data_ptr() + j * B * C * HW[0] * HW[1] for j in range(3)]
    if kind == "scratch":  # still ONE augmentation launch: 3B samples, period 3B, the rows of the block's run
        s_on = [args for n, args in t_on if n == "curla_random_shift_u8"]
        s_off = [args for n, args in t_off if n == "curla_random_shift_u8"]
        assert len(s_on) == len(s_off) == 1 and s_on[0][6] == s_off[0][6] == 3 * B
        assert s_on[0][2] == 3 * B and s_off[0][2] == 2 * B
        assert s_on[0][1] == (None if store else blk.data_ptr() + lay["pos_run"])
    # a graph slot records the same launches
    _traced(lambda: (on.graph_block(0), off.graph_block(0)))  # (the pinned block's device address: a call)
    g = on.graph_block(0)
    tg = _traced(lambda: on.graph_refs(0))
    assert _names(tg) == _names(t_on) and tg[0][1][1] == g["dev"].data_ptr() and tg[0][1][2] == lay["graph_nbytes"]
    if store:
        assert g["mb_u8"].numel() == 3 * B * C * HW[0] * HW[1] + 32 and g["ar2"].numel() == 3 * B
        assert off.graph_block(0)["mb_u8"].numel() == 2 * B * C * HW[0] * HW[1] + 32
    # the copy route
    off._h_index_dev = on._h_index_dev = None
    c_off = _traced(lambda: off.sample_cpc_refs(indices=idx))
    c_on = _traced(lambda: on.sample_cpc_refs(indices=idx))
    head = ["curla_gather_transition_scalars"] + ["curla_nstep_compose"] * (n_step > 1)
    assert _names(c_off)[:len(head)] == head and _names(c_on)[:len(head) + 1] == head + ["curla_pos_walk"]
    assert _names(c_on)[len(head) + 1:] == _names(t_on)[1:] and _names(c_off)[len(head):] == _names(t_off)[1:]
    w = c_on[len(head)][1]
    blk = on._d_index[on._sample_slot]
    assert w[:4] == (blk.data_ptr(), lay["pos_row"], lay.get("pos_run", -1), lay.get("next_row", -1))
    assert w[4:9] == (on._cont.data_ptr(), 16, 3, n_step, B)


def test_two_allocations_read_the_positive_from_the_next_obs_ring():
    """A ring whose halves cannot share an allocation (capacity * frame not a multiple of 4): one scratch launch per
    tensor, the positive's from ``next_obses`` at the raw rows."""
    hw = (7, 9)
    mk = lambda **kw: ReplayBuffer((3,) + hw, (A,), 13, 4, "cpu", curla_amd.RandomShift(hw, 2), **kw)  # noqa: E731
    obs, act, rew, nxt, done, _ = episodes((3, 4), ("done", "open"), hw=hw, k=1)
    traces = []
    for rb in (mk(), mk(pos_offset=2)):
        assert rb._both is None
        for t in range(7):
            rb.add(obs[t], act[t], rew[t], nxt[t], done[t])
        rb._h_index_dev = [4096 * (k + 1) for k in range(rb._n_slots)]
        traces.append((rb, _traced(lambda: rb.sample_cpc_refs(indices=_idx()))))
    (off, t_off), (on, t_on) = traces
    assert _names(t_off) == ["curla_sample_stage"] + ["curla_random_shift_u8"] * 3
    assert _names(t_on) == ["curla_sample_stage_pos"] + ["curla_random_shift_u8"] * 3
    lay, blk = on.block_layout(), on._d_index[on._sample_slot]
    assert t_off[3][1][0] == off.obses.data_ptr() and t_on[3][1][0] == on.next_obses.data_ptr()
    assert t_on[3][1][1] == blk.data_ptr() + lay["pos_row"] and t_on[2][1][1] == blk.data_ptr()


def test_a_prioritized_buffer_walks_behind_the_draw():
    on = _filled(prioritized=True, pos_offset=2)
    off = _filled(prioritized=True)
    u = ((np.arange(4) + 0.5) / 4, np.zeros((6, 4), dtype=np.int32))
    t_on = _traced(lambda: on.sample_cpc_refs(indices=u))
    t_off = _traced(lambda: off.sample_cpc_refs(indices=u))
    assert _names(t_on) == ["curla_per_sample", "curla_gather_transition_scalars", "curla_pos_walk"]
    assert _names(t_off) == ["curla_per_sample", "curla_gather_transition_scalars"]
    lay = on.block_layout()
    assert lay["pos_row"] < lay["u"] < lay["prob"] and t_on[2][1][1] == lay["pos_row"] and t_on[2][1][6] == 2


def test_the_graph_fingerprint_covers_pos_offset():
    from tests.test_host_logic import HP
    aug = curla_amd.RandomCrop(HW, (16, 16))
    curla_amd.set_seed_everywhere(1)
    agent = curla_amd.CurlSacAgent((C, 16, 16), (A,), "cpu", aug, hidden_dim=64, **HP)
    agent._graph_rb = _filled()
    k0 = agent._graph_key()
    agent._graph_rb = _filled(pos_offset=0)
    assert agent._graph_key() == k0
    agent._graph_rb = _filled(pos_offset=3)
    k3 = agent._graph_key()
    agent._graph_rb = _filled(pos_offset=2)
    assert len({k0, k3, agent._graph_key()}) == 3


def test_the_restatement_on_the_scripted_flags():
    """(what the GPU tests hold the kernel to, on flags a reader can check by eye)"""
    cont = [0, 1, 1, 1, 0, 1, 1]  # capacity 7: the flags of the scripted stream after 12 adds
    assert [walk(cont, 7, 1, t) for t in range(7)] == list(range(7))
    assert [walk(cont, 7, 2, t) for t in range(7)] == [0, 2, 3, 4, 4, 6, 0]
    assert [walk(cont, 7, 3, t) for t in range(7)] == [0, 3, 4, 4, 4, 0, 0]
    assert [walk(cont, 7, 9, t) for t in range(7)] == [0, 4, 4, 4, 4, 0, 0]
