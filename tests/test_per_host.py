"""Host side of ``ReplayBuffer(prioritized=True)`` without a GPU (``device="cpu"`` buffers and the launch-trace hook,
which computes nothing): the constructor, the NumPy stream of a draw, the block layout, the launch schedule of a sample
and of the write paths, and the three entry points in the C ABI.  What the kernels compute: tests/test_gpu_per.py."""
import os
import re

import numpy as np
import pytest
import torch

import curla_amd
from curla_amd import _lib, ops
from curla_amd.utils import PerHandle, ReplayBuffer

C, HW, CROP, A, B = 9, (20, 20), (16, 16), 2, 4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("curla_per_set", "curla_per_sample", "curla_per_td")
AUGS = ["identity", "random_crop", "random_shift", "cutout", "cutout_color", "translate", "flip", "rotate", "grayscale",
        "color_jiggle", "noisy_cover", "random_conv", "random_crop+cutout", "translate+cutout_color"]


def _aug(name="random_crop"):
    return curla_amd.make_augmentor(name, HW, CROP if name.startswith("random_crop") else None, min_cut=2, max_cut=5)


def _rb(name="random_crop", capacity=16, device="cpu", batch=B, **kw):
    if kw.get("n_step", 1) > 1:
        kw.setdefault("discount", 0.99)
    return ReplayBuffer((C,) + HW, (A,), capacity, batch, device, _aug(name), **kw)


def _transitions(n, seed=0):
    """n <= 12 frame-stacked transitions (episodes of 1, 2, 5 and 4 steps: the frame store finds the shared frames)."""
    from tests.test_nstep_host import SCRIPT, episodes
    return tuple(a[:n] for a in episodes(seed=seed, **SCRIPT)[:5])


def _traced(fn):
    calls = []
    _lib.set_trace_hook(lambda name, args: calls.append((name, args)))
    try:
        out = fn()
    finally:
        _lib.set_trace_hook(None)
    return calls, out


def _same_stream(a, b):
    return np.array_equal(a[1], b[1]) and a[2] == b[2]


def test_constructor_validation():
    for bad in (dict(per_alpha=-0.1), dict(per_alpha=float("nan")), dict(per_alpha="0.6"), dict(per_alpha=True),
                dict(per_beta=-0.01), dict(per_beta=1.01), dict(per_beta=None), dict(per_beta=float("nan")),
                dict(per_eps=0.0), dict(per_eps=-1e-6), dict(per_eps=float("inf")), dict(per_eps=None)):
        with pytest.raises(ValueError):
            _rb(prioritized=True, **bad)
    rb = _rb(prioritized=True)
    assert rb.prioritized is True and (rb.per_alpha, rb.per_beta, rb.per_eps) == (0.6, 0.4, 1e-6)
    for ok in (dict(per_alpha=0), dict(per_alpha=2.5), dict(per_beta=0), dict(per_beta=1), dict(per_eps=1e-12)):
        _rb(prioritized=True, **ok)
    assert rb._per_s.dtype == torch.float32 and rb._per_s.shape == (16,) and not rb._per_s.any()
    assert rb._per_sums.dtype == torch.float64 and rb._per_sums.shape == (1,)
    assert rb._per_max.dtype == torch.float32 and rb._per_max.tolist() == [1.0]
    assert _rb(prioritized=True, capacity=ops.PER_CHUNK + 1)._per_sums.shape == (2,)
    assert rb.graph_supported() is False
    # the attributes are read at every use: an edit that breaks the rule is refused where it is used
    rb.idx = 8
    rb.per_beta = 1.5
    u = rb.draw_indices()
    calls, (obs, *_) = _traced(lambda: rb.sample_cpc_refs(indices=u))
    t = torch.zeros(2 * B)
    with pytest.raises(ValueError):
        _traced(lambda: obs.per.td_update(t, B, t, t, t, t, t))
    # off: no storage, no methods' worth of state
    plain = _rb()
    assert plain.prioritized is False and not any(k.startswith("_per") for k in vars(plain))
    for call in (plain.priorities, lambda: plain.update_priorities(torch.zeros(1, dtype=torch.int64), torch.zeros(1))):
        with pytest.raises(RuntimeError):
            call()
    with pytest.raises(ValueError):
        rb.update_priorities(torch.zeros(2, dtype=torch.int32), torch.zeros(2))
    with pytest.raises(ValueError):
        rb.update_priorities(torch.zeros(2, dtype=torch.int64), torch.zeros(3))
    with pytest.raises(ValueError):
        _rb(prioritized=True).draw_indices()  # nothing to sample


@pytest.mark.parametrize("name", ["random_crop", "cutout_color", "random_crop+cutout"])
def test_a_prioritized_draw_is_random_sample_then_the_augmentors_words(name):
    rb, plain = _rb(name, capacity=64, prioritized=True), _rb(name, capacity=64)
    rb.idx = plain.idx = 40
    np.random.seed(5)
    u, offs = rb.draw_indices()
    after = np.random.get_state()
    np.random.seed(5)
    r = np.random.random_sample(B)
    words = [rb.augmentor.draw_index_words(B) for _ in range(3)]
    assert _same_stream(after, np.random.get_state())
    assert u.dtype == np.float64 and np.array_equal(u, (np.arange(B) + r) / B) and (u >= 0).all() and (u < 1).all()
    assert offs.dtype == np.int32 and offs.shape == (6 * max(1, (rb._index_rows + 1) // 2), B)
    for j in range(3):
        for k, w in enumerate(words[j]):
            assert np.array_equal(offs[6 * (k // 2) + 2 * j + k % 2], np.broadcast_to(w, (B,)))
    # off: the stream is what it was -- one randint, then the same words
    np.random.seed(5)
    idxs, offs0 = plain.draw_indices()
    after = np.random.get_state()
    np.random.seed(5)
    want = np.random.randint(0, 40, size=B)
    for _ in range(3):
        plain.augmentor.draw_index_words(B)
    assert _same_stream(after, np.random.get_state())
    assert np.array_equal(idxs, want) and offs0.shape == offs.shape


def _parent_layout(rb):
    """block_layout() as it was before prioritized replay, restated."""
    n = 2 * B * 8 + 6 * B * 4
    lay = dict(idx=0, offs=2 * B * 8, offs_end=n, aug=None, aug_stride=0, aug_order=None, aug_rng=None)
    if rb.staged_aug:
        stride, fields = rb.augmentor.staged_layout(B, rb.obs_shape)
        lay.update(aug=n, aug_stride=stride, **fields)
        n += 3 * stride
    if rb._index_rows > 2:
        lay["cut"] = n
        n += (rb._index_rows - 2) * 3 * B * 4
    if rb.n_step > 1:
        lay["next_row"] = n
        n += 8 * B
    lay.update(nbytes=n, tail=n, graph_nbytes=n + rb.GRAPH_TAIL)
    return lay


@pytest.mark.parametrize("n_step", [1, 3])
@pytest.mark.parametrize("name", AUGS + ["color_jiggle+staged", "random_conv+staged"])
def test_block_layout(name, n_step):
    kw = dict(n_step=n_step)
    if name.endswith("+staged"):
        name, kw["staged_aug"] = name[:-len("+staged")], True
    off, off2, on = _rb(name, **kw), _rb(name, prioritized=False, per_beta=0.9, **kw), _rb(name, prioritized=True, **kw)
    parent = _parent_layout(off)
    assert off.block_layout() == parent and off2.block_layout() == parent
    assert "u" not in parent and "prob" not in parent
    lay = on.block_layout()
    moved = ("nbytes", "tail", "graph_nbytes", "u", "prob")
    assert {k: v for k, v in lay.items() if k not in moved} == {k: v for k, v in parent.items() if k not in moved}
    assert lay["u"] == parent["nbytes"] and lay["u"] % 8 == 0 and lay["prob"] == lay["u"] + 8 * B
    assert lay["nbytes"] == lay["tail"] >= lay["prob"] + 4 * B and lay["nbytes"] % 8 == 0
    assert lay["graph_nbytes"] == lay["nbytes"] + on.GRAPH_TAIL
    odd = _rb(name, batch=5, prioritized=True, **kw).block_layout()
    assert odd["nbytes"] % 8 == 0 and odd["u"] % 8 == 0 and odd["nbytes"] >= odd["prob"] + 4 * 5


@pytest.mark.parametrize("kw", [dict(), dict(dedup_frames=True), dict(n_step=3), dict(n_step=3, dedup_frames=True)])
def test_launch_order_of_a_prioritized_sample(kw):
    rb = _rb(prioritized=True, **kw)
    rb.add_batch(*_transitions(12))
    assert rb._h_index_dev is None  # the block goes by the copy, never by the in-place staging launch
    np.random.seed(3)
    ind = rb.draw_indices()
    calls, out = _traced(lambda: rb.sample_cpc_refs(indices=ind))
    names = [n for n, _ in calls]
    want = ["curla_per_sample", "curla_gather_transition_scalars"] + ["curla_nstep_compose"] * (rb.n_step > 1)
    assert names == want + ["curla_gather_stacks"] * (2 if rb.dedup_frames else 0)
    lay, blk = rb.block_layout(), rb._d_index[rb._sample_slot]
    a = calls[0][1]
    assert a[:7] == (rb._per_s.data_ptr(), rb._per_sums.data_ptr(), 16, blk.data_ptr(), lay["u"], lay["prob"], B)
    assert calls[1][1][1] == blk.data_ptr()  # the gather reads the rows the draw wrote
    # the host block: zeros where the rows go, u where the draw reads it; the device block got the copy
    host = rb._h_index[0]
    assert not host[:16 * B].any() and not host[lay["prob"]:lay["nbytes"]].any()
    assert np.array_equal(host[lay["u"]:lay["u"] + 8 * B].view(torch.float64).numpy(), ind[0])
    assert torch.equal(blk, host)
    # the hand-over rides on the obs handle; the six-tuple and the keys are what they were
    obs, act, rew, nxt, nd, kwargs = out
    assert sorted(kwargs) == ["obs_anchor", "obs_pos", "time_anchor", "time_pos"] and kwargs["obs_anchor"] is obs
    per = obs.per
    assert isinstance(per, PerHandle) and nxt.per is None and kwargs["obs_pos"].per is None
    assert per.rows.dtype == torch.int64 and per.rows.shape == (B,) and per.rows.data_ptr() == blk.data_ptr()
    assert per.prob.dtype == torch.float32 and per.prob.shape == (B,) and per.prob.data_ptr() == blk.data_ptr() + lay["prob"]
    # ... and its update is curla_per_td, then curla_per_set on the minibatch's rows with the candidates
    q, t, dq, loss, w, val = (torch.zeros(n) for n in (2 * B, B, 2 * B, 1, B, B))
    rb.per_beta = 0.7
    calls, _ = _traced(lambda: per.td_update(q, B, t, dq, loss, w, val))
    assert [n for n, _ in calls] == ["curla_per_td", "curla_per_set"]
    td, st = calls[0][1], calls[1][1]
    assert td[:4] == (q.data_ptr(), B, t.data_ptr(), per.prob.data_ptr())
    assert td[4:8] == (0.7, 1e-6, 0.6, B) and td[8:12] == tuple(x.data_ptr() for x in (dq, loss, w, val))
    assert st[:8] == (rb._per_s.data_ptr(), rb._per_sums.data_ptr(), rb._per_max.data_ptr(), 16, per.rows.data_ptr(), 0,
                      val.data_ptr(), B)
    # a float u is required: rows cannot be injected into a prioritized buffer
    with pytest.raises(ValueError):
        _traced(lambda: rb.sample_cpc_refs(indices=(np.arange(B), ind[1])))
    with pytest.raises(ValueError):
        _traced(lambda: rb.sample_cpc_refs(indices=(np.full(B, 1.0), ind[1])))
    # two samples later the handle is stale
    for _ in range(rb.N_SAMPLE_SLOTS):
        _traced(lambda: rb.sample_cpc_refs(indices=ind))
    with pytest.raises(RuntimeError, match="stale"):
        _traced(lambda: per.td_update(q, B, t, dq, loss, w, val))


@pytest.mark.parametrize("dedup", [False, True])
def test_write_paths_launch_one_per_set_each(dedup, tmp_path):
    rb = _rb(prioritized=True, capacity=7, dedup_frames=dedup)
    o, a, r, n, d = _transitions(12)
    sets = lambda calls: [c[1][3:8] for c in calls if c[0] == "curla_per_set"]  # noqa: E731
    calls, _ = _traced(lambda: rb.add(o[0], a[0], r[0], n[0], d[0]))
    assert [c[0] for c in calls].count("curla_per_set") == 1
    assert sets(calls) == [(7, None, 0, None, 1)]  # capacity, no rows: the run from row 0, no values: the maximum, n = 1
    calls, _ = _traced(lambda: rb.add_batch(o[1:10], a[1:10], r[1:10], n[1:10], d[1:10]))
    # the frame store adds one by one; the plain ring writes the block at once, the run wrapping modulo the capacity
    assert sets(calls) == ([(7, None, k % 7, None, 1) for k in range(1, 10)] if dedup else [(7, None, 1, None, 9)])
    assert rb.idx == 3 and rb.full
    calls, _ = _traced(lambda: rb.add(o[10], a[10], r[10], n[10], d[10]))  # a wrapped add is a new transition
    assert sets(calls) == [(7, None, 3, None, 1)]
    # update_priorities is the same entry point with rows and values
    rows, vals = torch.tensor([1, 1, 5]), torch.tensor([2.0, 3.0, 0.5])
    calls, _ = _traced(lambda: rb.update_priorities(rows, vals))
    assert sets(calls) == [(7, rows.data_ptr(), 0, vals.data_ptr(), 3)]
    # load: one per chunk file (plain ring; the frame store's load is its add loop)
    src = _rb(capacity=16)
    for lo, hi in ((0, 5), (5, 12)):
        for t in range(lo, hi):
            src.add(o[t], a[t], r[t], n[t], d[t])
        src.save(str(tmp_path))
    fresh = _rb(prioritized=True, capacity=16, dedup_frames=dedup)
    calls, _ = _traced(lambda: fresh.load(str(tmp_path)))
    assert sets(calls) == ([(16, None, k, None, 1) for k in range(12)] if dedup else [(16, None, 0, None, 5), (16, None, 5, None, 7)])
    assert fresh.idx == 12
    # off: none of it
    plain = _rb(capacity=7, dedup_frames=dedup)
    calls, _ = _traced(lambda: (plain.add(o[0], a[0], r[0], n[0], d[0]), plain.add_batch(o[1:4], a[1:4], r[1:4], n[1:4], d[1:4])))
    assert not [c for c in calls if c[0] in NEW]


def test_off_launches_what_it_launched():
    """prioritized=False spelled out against a buffer constructed without the keywords: the same allocations, name by
    name, the same pinned bytes and the same launch trace for one sample (addresses relative to each buffer's tensors)."""
    from tests.test_nstep_host import _relative
    for kw in (dict(), dict(dedup_frames=True), dict(n_step=3)):
        default, off = _rb(**kw), _rb(prioritized=False, per_alpha=0.3, per_beta=1.0, per_eps=0.5, **kw)
        for rb in (default, off):
            rb.add_batch(*_transitions(12))
            rb._h_index_dev = [4096 * (k + 1) for k in range(rb._n_slots)]  # (stand-ins: the route of a device buffer)
        shapes = lambda rb: {k: (tuple(v.shape), v.dtype) for k, v in vars(rb).items()  # noqa: E731
                             if isinstance(v, (torch.Tensor, np.ndarray))}
        assert shapes(default) == shapes(off)
        ind = (np.array([0, 5, 11, 3]), np.zeros((6, B), dtype=np.int32))
        (t0, o0), (t1, o1) = _traced(lambda: default.sample_cpc_refs(indices=ind)), _traced(lambda: off.sample_cpc_refs(indices=ind))
        assert _relative(default, t0) == _relative(off, t1) and not [c for c in t1 if c[0] in NEW]
        assert t1[0][0] == ("curla_sample_stage_nstep" if kw.get("n_step") else "curla_sample_stage")
        lay = off.block_layout()
        end = lay.get("next_row", lay["nbytes"])  # (next_row is the device's to write: the host leaves it as allocated)
        assert torch.equal(default._h_index[0, :end], off._h_index[0, :end]) and o1[0].per is None


def test_the_agent_takes_the_unfused_loss_for_a_prioritized_minibatch_only():
    from tests.test_host_logic import HP, NullLogger
    curla_amd.set_seed_everywhere(1)
    agent = curla_amd.CurlSacAgent((C,) + CROP, (A,), "cpu", _aug(), hidden_dim=64, **HP)
    names = {}
    for prioritized in (False, True):
        rb = _rb(prioritized=prioritized)
        rb.add_batch(*_transitions(12))
        calls, _ = _traced(lambda: agent.update(rb, NullLogger(), 1))
        names[prioritized] = [n for n, _ in calls]
    off, on = names[False], names[True]
    assert not [n for n in off if n in NEW] and "curla_mlp_out_bwd_loss" in off and "curla_critic_td_loss" not in off
    assert "curla_mlp_out_bwd_loss" not in on[:on.index("curla_per_set")]
    i = on.index("curla_critic_td_loss")
    assert on[i:i + 4] == ["curla_critic_td_loss", "curla_per_td", "curla_per_set", "curla_mlp_out_bwd"]
    assert on.count("curla_per_td") == 1 and on.count("curla_per_set") == 1 and on.count("curla_per_sample") == 1
    ws = agent._ws(B)
    assert ws.per_w.shape == (B,) and ws.per_value.shape == (B,)
    # update graphs: refused as for any buffer that is not graph-replayable
    assert rb.graph_supported() is False


def test_abi_declares_and_binds_the_three_entry_points():
    text = open(os.path.join(ROOT, "include", "curla_hip.h")).read()
    assert re.search(r"#define\s+CURLA_ABI_VERSION\s+8\b", text) and _lib.ABI_VERSION == 8
    m = re.search(r"#define\s+CURLA_PER_CHUNK\s+(\d+)", text)
    assert m and int(m.group(1)) == ops.PER_CHUNK
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(curla_[a-z0-9_]+)\s*\(", code)))
    assert sorted(_lib.SIGNATURES) == declared and set(NEW) <= set(declared)
    assert [n for n in declared if n.startswith("curla_per_")] == sorted(NEW)
    ctype = {"int": _lib.c_int, "long long": _lib.c_ll, "float": _lib.c_float}
    for name in NEW:
        params = [p.strip() for p in re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, code).group(1).split(",")]
        assert len(params) == len(_lib.SIGNATURES[name])
        for p, t in zip(params, _lib.SIGNATURES[name]):
            assert t is (_lib.vp if "*" in p else ctype[p.rsplit(" ", 1)[0]]), (name, p)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NEW) and lib.curla_abi_version() == 8
    # the argument checks answer before any launch: no device is needed to be refused
    s, sums, vmax, blk = (ctypes_buf(n) for n in (64, 8, 4, 256))
    ok_set = [s, sums, vmax, 16, None, 0, None, 1, None]
    bad_sets = [(0, None), (1, None), (2, None), (0, s + 2), (1, sums + 4), (2, vmax + 1), (7, 0), (3, 0), (5, 16), (5, -1),
                (4, s + 4), (6, s + 2)]
    for i, v in bad_sets:
        args = list(ok_set)
        args[i] = v
        assert lib.curla_per_set(*args) == -1, (i, v)
    ok_sample = [s, sums, 16, blk, 16 * B, 24 * B, B, None]
    for i, v in [(0, None), (1, None), (3, None), (0, s + 2), (1, sums + 4), (3, blk + 4), (6, 0), (2, 0), (4, 16 * B + 4),
                 (5, 24 * B + 2), (4, 8 * B), (5, 8), (5, 16 * B + 8), (4, 1 << 30)]:
        args = list(ok_sample)
        args[i] = v
        assert lib.curla_per_sample(*args) == -1, (i, v)
    ok_td = [s, B, s, s, 0.4, 1e-6, 0.6, B, s, s, s, s, None]
    for i, v in [(0, None), (2, None), (3, None), (8, None), (9, None), (10, None), (11, None), (0, s + 2), (7, 0),
                 (1, B - 1), (4, -0.1), (4, 1.1), (5, 0.0), (6, -1.0), (4, float("nan"))]:
        args = list(ok_td)
        args[i] = v
        assert lib.curla_per_td(*args) == -1, (i, v)


_KEEP = []


def ctypes_buf(nbytes):
    """The address of a 16-byte aligned host buffer (never dereferenced: the calls above are refused first)."""
    import ctypes
    raw = ctypes.create_string_buffer(nbytes + 16)
    _KEEP.append(raw)
    return (ctypes.addressof(raw) + 15) & ~15
