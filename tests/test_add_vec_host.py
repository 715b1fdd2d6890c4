"""Host side of ``ReplayBuffer(n_envs=N)`` without a GPU (``device="cpu"`` buffers and the launch-trace hook, which
computes nothing): the per-lane continuity flags of add_vec / add_batch / load against N single-environment buffers,
the constructor's and the write paths' refusals, the launch schedule, and the C ABI's new entry points."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import curla_amd
from curla_amd import _lib
from curla_amd.utils import ReplayBuffer
from tests.test_nstep_host import SCRIPT, _relative, _traced, episodes, expected_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, HW, A, N = 9, (20, 20), 2, 3
# Three lanes of 12 steps whose episodes end at different steps and in different ways: lane 0 is test_nstep_host's
# SCRIPT (done after step 0, cut after 2, done after 7), lane 1 is cut after 3 and done after 6, lane 2 done after 5
# and cut after 6.
LANES = (SCRIPT, dict(lengths=(4, 3, 5), ends=("cut", "done", "open")),
         dict(lengths=(6, 1, 5), ends=("done", "cut", "open")))
NEW = ("curla_add_vec", "curla_nstep_compose_strided", "curla_sample_stage_nstep_strided", "curla_pos_walk_strided",
       "curla_sample_stage_pos_strided")


def streams(hw=HW):
    """The three lanes as episodes() returns them, and the same transitions stacked per vector step: obs [12][3]..."""
    lanes = [episodes(seed=e, hw=hw, **kw) for e, kw in enumerate(LANES)]
    assert all(len(l[0]) == 12 for l in lanes)
    vec = tuple(np.stack([l[j] for l in lanes], axis=1) for j in range(5))
    return lanes, vec


def _buffer(capacity, n_envs=N, n_step=3, B=4, **kw):
    aug = curla_amd.RandomCrop(HW, (16, 16))
    if n_step > 1:
        kw.setdefault("discount", 0.99)
    return ReplayBuffer((C,) + HW, (A,), capacity, B, "cpu", aug, n_step=n_step, n_envs=n_envs, **kw)


def _feed(rb, vec, lo=0, hi=12):
    for t in range(lo, hi):
        rb.add_vec(*(a[t] for a in vec))


def test_the_lanes_differ():
    """The fixture itself: every lane has its own links, with a cut and a done at different steps, so a rule that
    looked at the neighbouring row (stride 1) could not give these flags."""
    lanes, vec = streams()
    links = [l[5].tolist() for l in lanes]
    assert links[0] == [0, 1, 0, 1, 1, 1, 1, 0, 1, 1, 1, 1]
    assert links[1] == [1, 1, 1, 0, 1, 1, 0, 1, 1, 1, 1, 1]
    assert links[2] == [1, 1, 1, 1, 1, 0, 0, 1, 1, 1, 1, 1]
    for e, (t_cut, t_done) in enumerate(((2, 0), (3, 6), (6, 5))):
        obs, nxt, done = lanes[e][0], lanes[e][3], lanes[e][4]
        assert not done[t_cut] and not np.array_equal(nxt[t_cut], obs[t_cut + 1]) and done[t_done]
    assert vec[0].shape == (12, N, C) + HW and vec[1].shape == (12, N, A) and vec[4].shape == (12, N)
    # no lane's next_obs is another lane's obs: interleaving them through a stride-1 rule links nothing
    flat_o, flat_n = vec[0].reshape(36, -1), vec[3].reshape(36, -1)
    assert not any(np.array_equal(flat_n[j], flat_o[j + 1]) for j in range(35))


def test_flags_equal_three_single_environment_buffers():
    """H1: capacity 21 = 3 lanes of 7, 12 vector steps (the ring wraps).  After EVERY step lane e of the vector
    buffer's flags is the flag array of a capacity-7 buffer fed that lane alone by add(), the newest 3 rows carry 0, and
    the device array follows its mirror."""
    lanes, vec = streams()
    rb = _buffer(21)
    single = [_buffer(7, n_envs=1) for _ in range(N)]
    assert rb.n_envs == N and single[0].n_envs == 1
    for t in range(12):
        assert rb.idx == (t * N) % 21
        rb.add_vec(*(a[t] for a in vec))
        for e in range(N):
            obs, act, rew, nxt, done, link = lanes[e]
            single[e].add(obs[t], act[t], rew[t], nxt[t], done[t])
            assert np.array_equal(rb._cont_h[e::N], single[e]._cont_h), (t, e)
            assert np.array_equal(single[e]._cont_h, expected_flags(link, 7, t))
        first = (t * N) % 21
        assert not rb._cont_h[first:first + N].any()
        assert np.array_equal(rb._cont.numpy(), rb._cont_h)
    assert rb.idx == 36 % 21 and rb.full
    assert rb._cont_h.reshape(7, N).T.tolist() == [[0, 1, 1, 1, 0, 1, 1], [1, 1, 1, 1, 0, 1, 0], [1, 1, 1, 1, 0, 0, 0]]
    # pixels and scalars sit at (t * N + e) % capacity: the last 7 steps of every lane are in the ring
    for e in range(N):
        for t in range(5, 12):
            r = (t * N + e) % 21
            assert np.array_equal(rb.obses[r].permute(2, 0, 1).numpy(), lanes[e][0][t])
            assert np.array_equal(rb.next_obses[r].permute(2, 0, 1).numpy(), lanes[e][3][t])
            want = np.concatenate([lanes[e][1][t], [lanes[e][2][t], 1.0 - lanes[e][4][t]]]).astype(np.float32)
            assert np.array_equal(rb._sc[r].numpy(), want)


def test_a_step_that_is_not_the_next_one_links_nothing():
    """The first condition of the rule: the previous write must be the vector step directly before.  A buffer whose
    write head was moved (what load() of a shorter file set does) keeps the old step's flags at 0."""
    _, vec = streams()
    rb = _buffer(21)
    _feed(rb, vec, 0, 2)
    assert rb._cont_h[:3].tolist() == [0, 1, 1] and not rb._cont_h[3:].any()  # lane 0's first episode is done
    _feed(rb, vec, 2, 3)
    assert rb._cont_h[3:6].tolist() == [1, 1, 1]  # step 1 -> 2 links every lane
    rb2 = _buffer(21)
    _feed(rb2, vec, 1, 2)
    rb2.idx = 6
    _feed(rb2, vec, 2, 3)  # continues step 1 by its bytes, but is not written behind it
    assert not rb2._cont_h.any()


def test_add_batch_and_save_load_give_the_flags_of_the_add_vec_loop(tmp_path):
    """H2: add_batch in row order (step-major, environment-minor), cut inside episodes (a batch that starts
    mid-episode: steps 3..8 for lane 0's third episode, 9.. for all lanes) and wrapping the ring (steps 3..8 cross row
    21); then two saved chunks, the cut inside an episode, loaded into a fresh buffer."""
    lanes, vec = streams()
    flat = tuple(a.reshape((36,) + a.shape[2:]) for a in vec)
    loop, bulk = _buffer(21), _buffer(21)
    for lo, hi in ((0, 2), (2, 3), (3, 9), (9, 12)):
        _feed(loop, vec, lo, hi)
        if hi - lo == 1:
            bulk.add_vec(*(a[lo] for a in vec))
        else:
            bulk.add_batch(*(a[lo * N:hi * N] for a in flat))
        assert np.array_equal(bulk._cont_h, loop._cont_h), (lo, hi)
        assert np.array_equal(bulk._cont.numpy(), loop._cont_h)
        assert (bulk.idx, bulk.full) == (loop.idx, loop.full)
    assert bulk.idx == 15 and bulk.full
    assert torch.equal(bulk.obses, loop.obses) and torch.equal(bulk.next_obses, loop.next_obses)
    assert torch.equal(bulk._sc, loop._sc)
    # one call longer than the ring: rows written twice keep their last writer's flag
    once = _buffer(21)
    once.add_batch(*flat)
    assert np.array_equal(once._cont_h, loop._cont_h) and np.array_equal(once._cont.numpy(), loop._cont_h)
    # save -> load (the reference's files do not wrap: a ring that holds all 36 rows)
    rb = _buffer(48)
    for t in range(12):
        rb.add_vec(*(a[t] for a in vec))
        if t in (4, 11):
            rb.save(str(tmp_path))
    assert sorted(p.name for p in tmp_path.iterdir()) == ["0_15.pt", "15_36.pt"]
    fresh = _buffer(48)
    fresh.load(str(tmp_path))
    assert (fresh.idx, fresh.full) == (rb.idx, rb.full) == (36, False)
    assert np.array_equal(fresh._cont_h, rb._cont_h) and np.array_equal(fresh._cont.numpy(), rb._cont_h)
    for e in range(N):
        assert rb._cont_h[e:36:N].tolist() == lanes[e][5][:11].tolist() + [0]
    # ... and the stream goes on from a loaded buffer as from the one that saved it
    nxt = vec[3][11]
    for b in (rb, fresh):
        b.add_vec(nxt, vec[1][0], vec[2][0], vec[0][0], [False] * N)
    assert rb._cont_h[33:39].tolist() == fresh._cont_h[33:39].tolist() == [1, 1, 1, 0, 0, 0]
    # chunk borders must be whole vector steps
    odd = tmp_path / "odd"
    odd.mkdir()
    one = _buffer(48, n_envs=1)
    one.add_batch(*(a[:5] for a in flat))
    one.save(str(odd))
    with pytest.raises(ValueError, match="whole vector steps"):
        _buffer(48).load(str(odd))


def test_constructor_and_argument_errors():
    """H3."""
    aug = curla_amd.RandomCrop(HW, (16, 16))
    mk = lambda cap=21, **kw: ReplayBuffer((C,) + HW, (A,), cap, 4, "cpu", aug, **kw)  # noqa: E731
    for bad in (0, -1, True, False, 3.0, 2.5, None, "3"):
        with pytest.raises(ValueError, match="n_envs"):
            mk(n_envs=bad)
    with pytest.raises(ValueError, match="multiple of n_envs"):
        mk(20, n_envs=3)
    with pytest.raises(ValueError, match="dedup_frames"):
        mk(n_envs=3, dedup_frames=True)
    assert mk().n_envs == 1 and mk(n_envs=np.int64(3)).n_envs == 3
    rb = mk(n_envs=3, n_step=3, discount=0.99)
    with pytest.raises(AttributeError):
        rb.n_envs = 1
    _, vec = streams()
    o, a, r, n, d = (x[0] for x in vec)
    with pytest.raises(ValueError, match="add_vec"):
        rb.add(o[0], a[0], r[0], n[0], d[0])
    for bad in ((o[:2], a, r, n, d), (o, a[:2], r, n, d), (o, a, r[:2], n, d), (o, a, r, n[:2], d), (o, a, r, n, d[:2]),
                (o[0], a, r, n, d), (o, a.reshape(-1), r, n, d), (o, a, 0.5, n, d), (o[:, :3], a, r, n, d)):
        with pytest.raises(ValueError, match=r"\(3, 9, 20, 20\).*\(3, 2\).*\(3,\)"):
            rb.add_vec(*bad)
    assert rb.idx == 0 and not rb._cont_h.any()  # refused before anything was written
    flat = tuple(x.reshape((36,) + x.shape[2:]) for x in vec)
    for m in (1, 4, 35):
        with pytest.raises(ValueError, match="whole vector steps"):
            rb.add_batch(*(x[:m] for x in flat))
    assert rb.idx == 0
    # an n_envs=1 buffer takes add_vec of one transition and stores what add() stores
    v, s = _buffer(7, n_envs=1), _buffer(7, n_envs=1)
    lane = episodes(**SCRIPT)
    for t in range(9):
        v.add_vec(lane[0][t][None], lane[1][t][None], lane[2][t:t + 1], lane[3][t][None], lane[4][t:t + 1])
        s.add(lane[0][t], lane[1][t], lane[2][t], lane[3][t], lane[4][t])
    assert torch.equal(v._both, s._both) and torch.equal(v._sc, s._sc) and np.array_equal(v._cont_h, s._cont_h)
    assert (v.idx, v.full) == (s.idx, s.full) == (2, True)
    with pytest.raises(ValueError):
        v.add_vec(lane[0][:2], lane[1][:2], lane[2][:2], lane[3][:2], lane[4][:2])


def _filled(n_envs, capacity=21, **kw):
    _, vec = streams()
    rb = _buffer(capacity, n_envs=n_envs, **kw)
    _feed(rb, vec, 0, 4)
    rb._h_index_dev = [4096 * (k + 1) for k in range(rb._n_slots)]  # as in test_nstep_host: the staging route
    return rb, vec


IDX = (np.array([0, 5, 11, 3]), np.zeros((6, 4), dtype=np.int32))


@pytest.mark.parametrize("prioritized", [False, True])
def test_an_add_vec_is_one_launch(prioritized):
    """H4: one curla_add_vec per vector step -- frames, scalars and flags -- plus curla_per_set(first_row=idx, n=N)
    when prioritized.  (The pinned block's one async copy is a torch copy, not a library call: a CPU buffer has none.)"""
    rb, vec = _filled(N, prioritized=prioritized)
    first = rb.idx
    trace = _traced(lambda: rb.add_vec(*(a[4] for a in vec)))
    assert [n for n, _ in trace] == ["curla_add_vec"] + ["curla_per_set"] * prioritized
    a = trace[0][1]
    assert len(a) == len(_lib.SIGNATURES["curla_add_vec"])
    assert a[:5] == (rb._d_add.data_ptr(), rb.obses.data_ptr(), rb.next_obses.data_ptr(), rb._sc.data_ptr(),
                     rb._cont.data_ptr())
    assert a[5:13] == (21, first, 1, N, C, HW[0], HW[1], A) and first == 12
    if prioritized:
        p = trace[1][1]
        assert (p[3], p[4], p[5], p[6], p[7]) == (21, None, first, None, N)
    # the first step of a buffer has no previous run; a buffer without flags hands no flag array over
    fresh = _buffer(21, prioritized=prioritized)
    a = _traced(lambda: fresh.add_vec(*(x[0] for x in vec)))[0][1]
    assert (a[6], a[7]) == (0, 0)
    plain = _buffer(21, n_step=1)
    assert not hasattr(plain, "_cont")
    a = _traced(lambda: plain.add_vec(*(x[0] for x in vec)))[0][1]
    assert a[4] is None and a[7] == 0
    # the block: [N obs | N next_obs | pad to 16 | N x (A + 2) float32 | 2N flag bytes]
    fr = C * HW[0] * HW[1]
    assert rb._sc_off == (2 * N * fr + 15) // 16 * 16 and rb._cont_off == rb._sc_off + 4 * N * (A + 2)
    assert rb._d_add.numel() == rb._cont_off + 8 and plain._d_add.numel() == rb._cont_off


def test_a_vector_buffer_samples_through_the_strided_entry_points():
    """H4: n_envs=3, n_step=3, pos_offset=2 -- every route of _stage calls the _strided name with stride 3 behind the
    capacity; the same construction with n_envs=1 calls exactly the namesakes, with their argument lists."""
    rb, _ = _filled(N, pos_offset=2)
    lay = rb.block_layout()
    t = _traced(lambda: rb.sample_cpc_refs(indices=IDX))
    assert [n for n, _ in t] == ["curla_sample_stage_pos_strided"]
    a = t[0][1]
    assert len(a) == 19 and (a[8], a[9], a[10], a[11], a[12]) == (21, 3, 3, 0.99, 2)
    assert (a[3], a[4], a[7]) == (lay["next_row"], lay["pos_row"], rb._cont.data_ptr())
    _traced(lambda: rb.graph_block(0))
    tg = _traced(lambda: rb.graph_refs(0))  # a graph slot records the same launch
    assert [n for n, _ in tg] == ["curla_sample_stage_pos_strided"] and tg[0][1][9] == 3
    rb._h_index_dev = None  # the route by copy
    tc = _traced(lambda: rb.sample_cpc_refs(indices=IDX))
    assert [n for n, _ in tc] == ["curla_gather_transition_scalars", "curla_nstep_compose_strided", "curla_pos_walk_strided"]
    assert (tc[1][1][4], tc[1][1][5], tc[1][1][6]) == (21, 3, 3) and len(tc[1][1]) == 14
    assert (tc[2][1][5], tc[2][1][6], tc[2][1][7], tc[2][1][8]) == (21, 3, 2, 3) and len(tc[2][1]) == 11
    nstep, _ = _filled(N)  # n-step alone
    tn = _traced(lambda: nstep.sample_cpc_refs(indices=IDX))
    assert [n for n, _ in tn] == ["curla_sample_stage_nstep_strided"]
    assert (tn[0][1][6], tn[0][1][7], tn[0][1][8]) == (21, 3, 3) and len(tn[0][1]) == 16
    plain, _ = _filled(N, n_step=1)  # neither walk: nothing strided to call
    assert [n for n, _ in _traced(lambda: plain.sample_cpc_refs(indices=IDX))] == ["curla_sample_stage"]


@pytest.mark.parametrize("kw", [dict(), dict(pos_offset=2), dict(n_step=1), dict(n_step=1, pos_offset=2)])
def test_n_envs_1_is_the_buffer_as_it_was(kw):
    """H4: n_envs=1 spelled out against a buffer constructed without the keyword: the same allocations, the same block
    layout, and -- addresses relative to each buffer's own tensors -- the same launch trace by the existing names and
    argument counts, on both staging routes."""
    aug = curla_amd.RandomCrop(HW, (16, 16))
    kw = dict(dict(n_step=3), **kw)
    if kw["n_step"] > 1:
        kw["discount"] = 0.99
    default = ReplayBuffer((C,) + HW, (A,), 21, 4, "cpu", aug, **kw)
    one = ReplayBuffer((C,) + HW, (A,), 21, 4, "cpu", aug, n_envs=1, **kw)
    _, vec = streams()
    flat = tuple(x.reshape((36,) + x.shape[2:]) for x in vec)
    for rb in (default, one):
        for t in range(12):
            rb.add(*(x[t] for x in flat))
        rb._h_index_dev = [4096 * (k + 1) for k in range(rb._n_slots)]
    shapes = lambda rb: {k: (tuple(v.shape), v.dtype) for k, v in vars(rb).items()  # noqa: E731
                         if isinstance(v, (torch.Tensor, np.ndarray))}
    assert shapes(one) == shapes(default) and one.block_layout() == default.block_layout()
    fr = C * HW[0] * HW[1]
    keep = kw["n_step"] > 1 or kw.get("pos_offset", 0) > 1
    assert one._d_add.numel() == (2 * fr + 15) // 16 * 16 + 4 * (A + 2) + 4 * keep
    walk = kw["n_step"] > 1, kw.get("pos_offset", 0) > 0
    staged = {(True, False): ("curla_sample_stage_nstep", 15), (False, True): ("curla_sample_stage_pos", 18),
              (True, True): ("curla_sample_stage_pos", 18), (False, False): ("curla_sample_stage", 10)}[walk]
    copied = ([("curla_gather_transition_scalars", 8)] + [("curla_nstep_compose", 13)] * walk[0]
              + [("curla_pos_walk", 10)] * walk[1])
    for want in ([staged], copied):
        t1 = _traced(lambda: one.sample_cpc_refs(indices=IDX))
        td = _traced(lambda: default.sample_cpc_refs(indices=IDX))
        assert [(n, len(a)) for n, a in t1] == want
        assert _relative(one, t1) == _relative(default, td)
        one._h_index_dev = default._h_index_dev = None
    assert _traced(lambda: one.add_vec(*(x[12:13] for x in flat))) == []  # add(): a CPU buffer stores on the host


def test_the_graph_key_covers_n_envs():
    from tests.test_host_logic import HP
    agent = curla_amd.CurlSacAgent((C, 16, 16), (A,), "cpu", curla_amd.RandomCrop(HW, (16, 16)), hidden_dim=64, **HP)
    agent._graph_rb = _buffer(21, n_envs=1)
    k1 = agent._graph_key()
    agent._graph_rb = _buffer(21, n_envs=3)
    assert agent._graph_key() != k1 and agent._graph_rb_key() == (3, 0.99, 0, 3)


_KEEP = []


def _buf(nbytes):
    """The address of a 16-byte aligned host buffer (never dereferenced: the calls below are refused first)."""
    raw = ctypes.create_string_buffer(nbytes + 16)
    _KEEP.append(raw)
    return (ctypes.addressof(raw) + 15) & ~15


def test_abi_declares_and_binds_the_new_entry_points():
    """H5: declared in the header as additive (the version stays 8), each _strided signature its namesake's with
    ``long long stride`` behind ``capacity``, bound by the ctypes table, exported by the library -- and the argument
    checks answer before any launch, so no device is needed to be refused."""
    text = open(os.path.join(ROOT, "include", "curla_hip.h")).read()
    assert re.search(r"#define\s+CURLA_ABI_VERSION\s+8\b", text) and _lib.ABI_VERSION == 8
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(curla_[a-z0-9_]+)\s*\(", code)))
    assert sorted(_lib.SIGNATURES) == declared and set(NEW) <= set(declared)
    for name in NEW:  # the comment in front of the declaration says so
        comment = text[:text.index("int %s(" % name)].rsplit("/*", 1)[1]
        assert "Additive: CURLA_ABI_VERSION stays 8" in comment, name
    params = lambda name: [" ".join(p.split()) for p in  # noqa: E731
                           re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, code).group(1).split(",")]
    ctype = {"int": _lib.c_int, "long long": _lib.c_ll, "float": _lib.c_float}
    for name in NEW:
        assert len(params(name)) == len(_lib.SIGNATURES[name])
        for p, t in zip(params(name), _lib.SIGNATURES[name]):
            assert t is (_lib.vp if "*" in p else ctype[p.rsplit(" ", 1)[0]]), (name, p)
    for name in NEW[1:]:
        old, new = params(name[:-len("_strided")]), params(name)
        at = old.index("long long capacity") + 1
        assert new == old[:at] + ["long long stride"] + old[at:], name
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NEW) and lib.curla_abi_version() == 8
    f = ctypes.c_float
    blk, sc, cont, out = (_buf(n) for n in (4096, 4096, 64, 256))
    B = 4
    ok = {  # valid argument lists (capacity 18, stride 3); the index of `stride` in each
        "curla_nstep_compose_strided": ([blk, 256, sc, cont, 18, 3, 3, f(0.99), B, A, out, out, out, None], 5),
        "curla_sample_stage_nstep_strided": ([blk, blk, 512, 256, sc, cont, 18, 3, 3, f(0.99), B, A, out, out, out, None], 7),
        "curla_pos_walk_strided": ([blk, 320, -1, 256, cont, 18, 3, 2, 3, B, None], 6),
        "curla_sample_stage_pos_strided": ([blk, blk, 512, 256, 320, -1, sc, cont, 18, 3, 3, f(0.99), 2, B, A, out, out, out,
                                            None], 9),
    }
    for name, (args, at) in ok.items():
        for stride, cap in ((0, 18), (-3, 18), (4, 18), (5, 18), (36, 18), (3, 0)):
            bad = list(args)
            bad[at - 1], bad[at] = cap, stride
            assert getattr(lib, name)(*bad) == -1, (name, stride, cap)
        bad = list(args)
        bad[0] = None  # what the namesake refuses is still refused
        assert getattr(lib, name)(*bad) == -1, name
    ring = _buf(64)
    ok_add = [blk, ring, ring + 32, sc, cont, 18, 6, 1, 3, 9, 20, 20, A, None]
    for i, v in [(0, None), (1, None), (2, None), (3, None), (0, blk + 2), (3, sc + 2), (8, 0), (8, -3), (6, 7), (6, -3),
                 (6, 18), (6, 16), (5, 17), (5, 0), (4, None), (5, 3), (9, 0), (10, 0), (11, 0), (12, 0), (10, 1 << 16)]:
        bad = list(ok_add)
        bad[i] = v
        if (i, v) == (5, 3):  # capacity == N: the previous run is the new one
            bad[6] = 0
        if (i, v) == (10, 1 << 16):  # 2 N H W >= 2^31
            bad[11] = 1 << 14
        assert lib.curla_add_vec(*bad) == -1, (i, v)
