"""Host side of ``ReplayBuffer(n_step=...)`` without a GPU (``device="cpu"`` buffers and the launch-trace hook, which
computes nothing): the continuity flags that every write path derives from the data it is handed, the constructor and
the agent's discount check, that the default buffer is untouched, and the launch schedule of an n-step sample."""
import numpy as np
import pytest
import torch

import curla_amd
from curla_amd import _lib
from curla_amd.utils import ReplayBuffer
from tests.test_host_logic import HP, NullLogger

C, HW, A = 9, (20, 20), 2


def episodes(lengths, ends, hw=HW, k=C // 3, seed=0):
    """A frame-stacked stream of episodes of the given lengths; ``ends[e]`` says how episode e ends: "done"
    (``done=True``), "cut" (a time-limit truncation: ``done=False`` and the next obs is a reset stack) or "open" (the
    stream simply continues -- only sensible for the last one).  Returns the five arrays of add_batch and ``link``:
    link[t] = 1 when transition t + 1 continues transition t (not done, next_obs[t] == obs[t + 1])."""
    rs = np.random.RandomState(seed)
    frame = lambda: rs.randint(0, 256, (3,) + hw, dtype=np.uint8)  # noqa: E731
    obs, nxt, done, link = [], [], [], []
    for n, end in zip(lengths, ends):
        stack = [frame()] * k
        for s in range(n):
            new = stack[1:] + [frame()]
            obs.append(np.concatenate(stack)), nxt.append(np.concatenate(new))
            last = s == n - 1
            done.append(last and end == "done")
            link.append(0 if last and end != "open" else 1)
            stack = new
    T = len(obs)
    return (np.stack(obs), rs.uniform(-1, 1, (T, A)).astype(np.float32), rs.randn(T).astype(np.float32), np.stack(nxt),
            np.array(done), np.array(link, dtype=np.uint8))


def expected_flags(link, capacity, t_last):
    """The rule of the issue after adds 0..t_last: a row's flag is its transition's link, unless that transition is the
    newest one."""
    flags = np.zeros(capacity, dtype=np.uint8)
    for t in range(t_last + 1):
        flags[t % capacity] = link[t] if t < t_last else 0
    return flags


def _buffer(capacity, n_step=3, B=4, **kw):
    """A CPU buffer with ``n_step`` passed explicitly (1 included); ``discount`` defaults to 0.99 where it is needed."""
    aug = curla_amd.RandomCrop(HW, (16, 16))
    if n_step > 1:
        kw.setdefault("discount", 0.99)
    return ReplayBuffer((C,) + HW, (A,), capacity, B, "cpu", aug, n_step=n_step, **kw)


SCRIPT = dict(lengths=(1, 2, 5, 4), ends=("done", "cut", "done", "open"))  # 12 transitions


@pytest.mark.parametrize("dedup", [False, True])
def test_flags_from_a_scripted_stream(dedup):
    """Capacity 7, 12 adds (the ring wraps): episodes of 1, 2 and 5 steps, one ended by done=True, one truncated
    (done=False, reset frame next), one still running.  After EVERY add the newest row's flag is 0 and every other
    row -- the one just before an overwritten row included -- carries its transition's link."""
    obs, act, rew, nxt, done, link = episodes(**SCRIPT)
    assert len(obs) == 12 and link.tolist() == [0, 1, 0, 1, 1, 1, 1, 0, 1, 1, 1, 1]
    assert not done[2] and not np.array_equal(nxt[2], obs[3])  # the truncation: only the bytes tell
    rb = _buffer(7, dedup_frames=dedup)
    for t in range(12):
        rb.add(obs[t], act[t], rew[t], nxt[t], done[t])
        assert rb._cont_h[t % 7] == 0
        assert np.array_equal(rb._cont_h, expected_flags(link, 7, t)), t
        assert np.array_equal(rb._cont.numpy(), rb._cont_h)  # the device array follows its mirror
    assert rb._cont_h.tolist() == [0, 1, 1, 1, 0, 1, 1]
    assert rb._cont.dtype == torch.uint8 and rb._cont.shape == (7,)


@pytest.mark.parametrize("dedup", [False, True])
def test_add_batch_gives_the_flags_of_the_add_loop(dedup):
    """... including the pair (previous add, first element of the batch) and a batch that wraps the ring."""
    obs, act, rew, nxt, done, link = episodes(**SCRIPT)
    loop, bulk = _buffer(7, dedup_frames=dedup), _buffer(7, dedup_frames=dedup)
    for t in range(12):
        loop.add(obs[t], act[t], rew[t], nxt[t], done[t])
    for lo, hi in ((0, 2), (2, 3), (3, 9), (9, 12)):  # cuts inside an episode (1|2, 8|9) and at episode ends
        if hi - lo == 1:
            bulk.add(obs[lo], act[lo], rew[lo], nxt[lo], done[lo])
        else:
            bulk.add_batch(obs[lo:hi], act[lo:hi], rew[lo:hi], nxt[lo:hi], done[lo:hi])
        assert np.array_equal(bulk._cont_h, expected_flags(link, 7, hi - 1)), (lo, hi)
    assert np.array_equal(bulk._cont_h, loop._cont_h) and np.array_equal(bulk._cont.numpy(), loop._cont_h)
    assert bulk.idx == loop.idx == 5 and bulk.full


def test_save_and_load_rebuild_the_flags(tmp_path, dedup=False):
    """Two chunks, the cut inside an episode: a fresh buffer that loads them has the flags of the buffer that saved
    them, and the payload on disk is still the reference's five arrays.  (Plain ring: saving a frame store gathers its
    stacks with a kernel, and its load() is add_batch, covered above.)"""
    obs, act, rew, nxt, done, link = episodes(**SCRIPT)
    rb = _buffer(16, dedup_frames=dedup)
    for t in range(12):
        rb.add(obs[t], act[t], rew[t], nxt[t], done[t])
        if t in (4, 11):
            rb.save(str(tmp_path))
    assert sorted(p.name for p in tmp_path.iterdir()) == ["0_5.pt", "5_12.pt"]
    payload = torch.load(str(tmp_path / "5_12.pt"), weights_only=False)
    assert len(payload) == 5 and all(isinstance(a, np.ndarray) for a in payload)
    assert [a.shape for a in payload] == [(7, C) + HW, (7, C) + HW, (7, A), (7, 1), (7, 1)]
    fresh = _buffer(16, dedup_frames=dedup)
    fresh.load(str(tmp_path))
    assert fresh.idx == 12
    assert np.array_equal(fresh._cont_h, rb._cont_h) and np.array_equal(fresh._cont.numpy(), rb._cont_h)
    assert rb._cont_h[:12].tolist() == link[:11].tolist() + [0]
    store = _buffer(16, dedup_frames=True)  # the same files into a frame store (its load() goes through add())
    store.load(str(tmp_path))
    assert store.idx == 12 and np.array_equal(store._cont_h, rb._cont_h)
    # ... and the stream goes on from a loaded buffer as from the one that saved it
    o2, a2, r2, n2, d2, _ = episodes((2,), ("done",), seed=9)
    for b in (rb, fresh):
        b.add(nxt[11], a2[0], r2[0], n2[0], False)   # continues transition 11
        b.add(o2[0], a2[1], r2[1], n2[1], True)      # a reset stack: does not continue the one just added
    assert rb._cont_h[11:14].tolist() == fresh._cont_h[11:14].tolist() == [1, 0, 0]


def test_constructor_validation():
    aug = curla_amd.RandomCrop(HW, (16, 16))
    mk = lambda **kw: ReplayBuffer((C,) + HW, (A,), 8, 4, "cpu", aug, **kw)  # noqa: E731
    for bad in (0, -1, True, False, 2.0, 3.5, None, "3"):
        with pytest.raises(ValueError):
            mk(n_step=bad, discount=0.99)
    with pytest.raises(ValueError):
        mk(n_step=3)  # discount is required
    for bad in (0.0, -0.5, 1.5, True, "0.99", float("nan")):
        with pytest.raises(ValueError):
            mk(n_step=3, discount=bad)
    rb = mk(n_step=3, discount=0.99)
    assert rb.n_step == 3 and rb.discount == 0.99 and type(rb.discount) is float
    assert mk(n_step=2, discount=1.0).discount == 1.0
    plain = mk()
    assert plain.n_step == 1 and plain.discount is None and not hasattr(plain, "_cont")
    assert mk(n_step=1).discount is None


def _traced(fn):
    calls = []
    _lib.set_trace_hook(lambda name, args: calls.append((name, args)))
    try:
        fn()
    finally:
        _lib.set_trace_hook(None)
    return calls


def _filled(n_step, **kw):
    """n_step=None: a buffer constructed without either keyword."""
    obs, act, rew, nxt, done, _ = episodes(**SCRIPT)
    if n_step is None:
        rb = ReplayBuffer((C,) + HW, (A,), 16, 4, "cpu", curla_amd.RandomCrop(HW, (16, 16)), **kw)
    else:
        rb = _buffer(16, n_step=n_step, **kw)
    for t in range(12):
        rb.add(obs[t], act[t], rew[t], nxt[t], done[t])
    # a CPU buffer has no pinned index slots; stand in for their device addresses so that sampling takes the route of
    # a device buffer (the staging kernel) under the trace hook
    rb._h_index_dev = [4096 * (k + 1) for k in range(rb._n_slots)]
    return rb


def test_the_agent_refuses_a_discount_that_is_not_the_buffers():
    aug = curla_amd.RandomCrop(HW, (16, 16))
    curla_amd.set_seed_everywhere(1)
    agent = curla_amd.CurlSacAgent((C, 16, 16), (A,), "cpu", aug, hidden_dim=64, **HP)
    rb = _filled(3)
    rb.discount = 0.95
    calls = []
    _lib.set_trace_hook(lambda name, args: calls.append(name))
    try:
        with pytest.raises(ValueError, match=r"0\.95.*0\.99"):
            agent.update(rb, NullLogger(), 1)
        with pytest.raises(ValueError, match=r"0\.95.*0\.99"):
            agent._update_graphed(rb, NullLogger(), 1)
        assert not calls  # refused before anything is drawn or launched
        rb.discount = 0.99
        agent.update(rb, NullLogger(), 1)
        assert "curla_sample_stage_nstep" in calls
        # the graphs' fingerprint covers the buffer's (n_step, discount)
        agent._graph_rb = rb
        k0 = agent._graph_key()
        rb.discount = agent.discount = 0.9
        assert agent._graph_key() != k0
        agent._graph_rb = _filled(1)
        agent.discount = 0.99
        assert agent._graph_key() != k0
    finally:
        _lib.set_trace_hook(None)


def _relative(rb, trace):
    """A launch trace with every address replaced by its offset inside the buffer's own allocation (two buffers of
    the same construction then give the same list)."""
    bases = sorted((t.data_ptr(), t.numel() * t.element_size(), name) for name, t in vars(rb).items()
                   if isinstance(t, torch.Tensor) and t.numel() and t._base is None)
    out = []
    for name, args in trace:
        row = []
        for a in args:
            hit = [(nm, a - lo) for lo, size, nm in bases if isinstance(a, int) and lo <= a < lo + size]
            row.append(hit[0] if hit else a)
        out.append((name, tuple(row)))
    return out


@pytest.mark.parametrize("explicit", [dict(), dict(discount=None), dict(discount=0.99)])
@pytest.mark.parametrize("kw", [dict(), dict(dedup_frames=True)])
def test_n_step_1_is_the_buffer_as_it_was(kw, explicit):
    """A buffer constructed with n_step=1 spelled out (with and without a discount) against one constructed without
    the keywords, both fed the same stream: the same block layout (no next_row region), the same allocations and --
    addresses taken relative to each buffer's own tensors -- the same launch trace for one sample_cpc_refs()."""
    default = _filled(None, **kw)
    one = _filled(1, **kw, **explicit)
    assert one.n_step == default.n_step == 1 and one.discount == explicit.get("discount")
    lay = one.block_layout()
    assert lay == default.block_layout() and "next_row" not in lay
    assert lay["nbytes"] == lay["tail"] == 2 * 4 * 8 + 6 * 4 * 4
    shapes = lambda rb: {k: (tuple(v.shape), v.dtype) for k, v in vars(rb).items()  # noqa: E731
                         if isinstance(v, (torch.Tensor, np.ndarray))}
    assert shapes(one) == shapes(default)  # every allocation, name by name
    assert one._d_add_sc.numel() == A + 2
    for attr in ("_cont", "_cont_h", "_last_next", "_chain"):
        assert not hasattr(one, attr)
    assert torch.equal(one._sc[:12], default._sc[:12])
    assert torch.equal(one.frames, default.frames) if kw else torch.equal(one._both, default._both)
    idx = (np.array([0, 5, 11, 3]), np.zeros((6, 4), dtype=np.int32))
    trace = _traced(lambda: one.sample_cpc_refs(indices=idx))
    names = [n for n, _ in trace]
    assert names == ["curla_sample_stage"] + ["curla_gather_stacks"] * (2 if kw else 0)
    trace_d = _traced(lambda: default.sample_cpc_refs(indices=idx))
    assert _relative(one, trace) == _relative(default, trace_d)
    stage = trace[0][1]
    assert len(stage) == 10 and stage[2] == lay["nbytes"] and (stage[4], stage[5]) == (4, A)
    assert stage[1] == one._d_index[one._sample_slot].data_ptr()
    # the pinned block holds the same bytes
    assert torch.equal(one._h_index[0, :lay["nbytes"]], default._h_index[0, :lay["nbytes"]])
    # add() launches what it launched: nothing about flags
    o, a, r, n, d, _ = episodes((1,), ("done",))
    adds = _traced(lambda: one.add(o[0], a[0], r[0], n[0], d[0]))
    assert [n for n, _ in adds] == []  # (a CPU buffer stores on the host)


@pytest.mark.parametrize("dedup", [False, True])
def test_a_bulk_write_longer_than_the_ring_gives_the_flags_of_the_add_loop(dedup):
    """add_batch of 12 transitions into a ring of 7, in one call and behind a single add (so that the batch overwrites
    the row of the previous add): rows written twice keep the flag of their last writer."""
    obs, act, rew, nxt, done, link = episodes(**SCRIPT)
    for first in (0, 1):
        loop, bulk = _buffer(7, dedup_frames=dedup), _buffer(7, dedup_frames=dedup)
        for t in range(12):
            loop.add(obs[t], act[t], rew[t], nxt[t], done[t])
        for t in range(first):
            bulk.add(obs[t], act[t], rew[t], nxt[t], done[t])
        bulk.add_batch(obs[first:], act[first:], rew[first:], nxt[first:], done[first:])
        assert np.array_equal(bulk._cont_h, expected_flags(link, 7, 11)), first
        assert np.array_equal(bulk._cont_h, loop._cont_h) and np.array_equal(bulk._cont.numpy(), loop._cont_h)
        assert bulk.idx == loop.idx == 5 and bulk.full
    # exactly the ring's length behind one add: the batch's last row IS the previous add's row
    exact = _buffer(7, dedup_frames=dedup)
    exact.add(obs[0], act[0], rew[0], nxt[0], done[0])
    exact.add_batch(obs[1:8], act[1:8], rew[1:8], nxt[1:8], done[1:8])
    assert np.array_equal(exact._cont_h, expected_flags(link, 7, 7))
    assert np.array_equal(exact._cont.numpy(), exact._cont_h)


@pytest.mark.parametrize("kw", [dict(), dict(dedup_frames=True)])
def test_an_n_step_sample_launches_as_many_kernels(kw):
    idx = (np.array([0, 5, 11, 3]), np.zeros((6, 4), dtype=np.int32))
    one, three = _filled(None, **kw), _filled(3, **kw)
    t1 = _traced(lambda: one.sample_cpc_refs(indices=idx))
    t3 = _traced(lambda: three.sample_cpc_refs(indices=idx))
    assert [n for n, _ in t3] == [n.replace("curla_sample_stage", "curla_sample_stage_nstep") for n, _ in t1]
    lay = three.block_layout()
    assert lay["next_row"] == one.block_layout()["nbytes"] and lay["nbytes"] == lay["tail"] == lay["next_row"] + 8 * 4
    a = t3[0][1]
    blk = three._d_index[three._sample_slot]
    assert (a[1], a[2], a[3]) == (blk.data_ptr(), lay["nbytes"], lay["next_row"])
    assert (a[5], a[6], a[7], a[8]) == (three._cont.data_ptr(), 16, 3, 0.99)
    if kw:  # the frame store gathers the next_obs stacks at the bootstrap rows, the obs stacks at the sampled rows
        assert t3[1][1][3] == blk.data_ptr() and t3[2][1][3] == blk.data_ptr() + lay["next_row"]
    # a graph slot records the same launch
    _traced(lambda: three.graph_block(0))
    g = three.graph_block(0)
    tg = _traced(lambda: three.graph_refs(0))
    assert [n for n, _ in tg] == [n for n, _ in t3]
    assert tg[0][1][1] == g["dev"].data_ptr() and tg[0][1][2] == lay["graph_nbytes"] and g["tail"] == lay["tail"]
    # the route without pinned slots: copy, gather, compose -- in front of everything that reads pixels
    three._h_index_dev = None
    tc = _traced(lambda: three.sample_cpc_refs(indices=idx))
    assert [n for n, _ in tc][:2] == ["curla_gather_transition_scalars", "curla_nstep_compose"]
    assert [n for n, _ in tc][2:] == [n for n, _ in t3][1:]
