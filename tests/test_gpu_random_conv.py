"""``RandomConv`` on the MI355X: ``curla_random_conv`` (uint8 NHWC ring -> float NHWC) and ``curla_random_conv_nchw``
against ``RandomConv.conv``, the float64 NumPy statement of the formula; the replay buffer's routes; whole updates, eager
against captured graphs.  Every kernel output lies in a NaN-filled buffer with guard floats on either side that must
still be NaN afterwards (the helpers of tests/test_gpu_augment_edges.py); every ring carries 32 bytes of slack that must
still be zero.

EXACT cases (filters of zeros and ones: every product is x * 1 or x * 0, so any summation order is exact) are compared
with ``np.array_equal``.

THE BOUND of the general case, per element: |kernel - f64| <= g * sum_i |w_i| |x_i| with g = 27 u / (1 - 27 u), u = 2^-24
-- the standard forward-error bound of a 27-term float32 dot product in any order, with or without FMA (Higham, Accuracy
and Stability of Numerical Algorithms, section 3.1); the reference is ``RandomConv.conv`` in float64 on the float32
weights taken exactly, the sum is ``RandomConv.conv(x, |w|)``.  Derived, not measured.

Worst |kernel - f64| / bound seen on the MI355X, per C (this file's own printout, test_random_weights_against_float64;
not used by any assertion): NOT MEASURED YET.
"""
import numpy as np
import pytest
import torch

from tests.test_gpu_augment_edges import _guarded, _guards_intact, _nchw, _nhwc, _Ring

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
G = 27 * U / (1 - 27 * U)

_seen = {}  # C -> worst |kernel - f64| / bound of this run, printed as it grows


def _conv_cls():
    import curla_amd
    return curla_amd.RandomConv


def _one_hots():
    """The 81 one-hot filters, float32 [81, 3, 3, 3, 3], filter n = its own flat index."""
    w = np.zeros((81, 81), dtype=np.float32)
    w[np.arange(81), np.arange(81)] = 1.0
    return w.reshape(81, 3, 3, 3, 3)


def _identity(n):
    w = np.zeros((n, 3, 3, 3, 3), dtype=np.float32)
    for c in range(3):
        w[:, c, c, 1, 1] = 1.0
    return w


def _launch(ring, idx, weights, B):
    """curla_random_conv into a guarded output; returns the output on the host, float32 [B, H, W, C]."""
    from curla_amd import ops
    _, H, W, C = ring.shape
    buf, out = _guarded((B, H, W, C))
    ops.random_conv(ring, idx, torch.from_numpy(np.ascontiguousarray(weights, dtype=np.float32)).cuda(), B, out)
    return _guards_intact(buf, out).numpy()


def _ref_and_bound(batch_nhwc, weights):
    """(float64 reference, per-element bound), both NHWC, from the host."""
    conv = _conv_cls().conv
    imgs = _nchw(batch_nhwc)
    return _nhwc(conv(imgs, weights)), G * _nhwc(conv(imgs, np.abs(np.asarray(weights, dtype=np.float64))))


def _spaced_ring(batch, seed):
    """The B frames of ``batch`` in the odd rows of a ring of 2 B + 1 rows whose even rows hold 255 everywhere, and an
    index that picks them in a permuted order: a read across a frame boundary meets 255s that the reference lacks."""
    B = batch.shape[0]
    frames = np.full((2 * B + 1,) + batch.shape[1:], 255, dtype=np.uint8)
    perm = np.random.RandomState(seed).permutation(B)
    rows = 2 * perm + 1
    frames[rows] = batch
    return frames, rows


# ------------------------------------------------------------------------------------------------ 5. one-hot filters
@pytest.mark.parametrize("C", [3, 9])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 5), (2, 3), (7, 9)])
def test_one_hot_filters_are_exact(H, W, C):
    """All 81 one-hot filters, 27 samples a launch: ``out`` is ``RandomConv.conv`` bit for bit -- gathered rows of a ring
    whose other rows are 255, and idx = None."""
    filters = _one_hots()
    rs = np.random.RandomState(100 * H + 10 * W + C)
    for part in range(3):
        w = filters[27 * part:27 * part + 27]
        batch = rs.randint(1, 256, (27, H, W, C), dtype=np.uint8)
        want, _ = _ref_and_bound(batch, w)
        assert want.any()
        frames, rows = _spaced_ring(batch, part)
        spaced, plain = _Ring(frames), _Ring(batch)
        got = _launch(spaced.ring, torch.from_numpy(rows).cuda(), w, 27)
        assert np.array_equal(got.astype(np.float64), want), ("gathered", part)
        got = _launch(plain.ring, None, w, 27)
        assert np.array_equal(got.astype(np.float64), want), ("idx=None", part)
        spaced.untouched(frames)
        plain.untouched(batch)


# ------------------------------------------------------------------------------------------------ 6. identity
def test_identity_filter_returns_the_bytes():
    B, C, H, W = 5, 12, 5, 13
    batch = np.random.RandomState(6).randint(0, 256, (B, H, W, C), dtype=np.uint8)
    batch[0, 0, 0], batch[-1, -1, -1] = 255, 0
    frames, rows = _spaced_ring(batch, 6)
    ring = _Ring(frames)
    got = _launch(ring.ring, torch.from_numpy(rows).cuda(), _identity(B), B)
    assert np.array_equal(got, batch.astype(np.float32))
    plain = _Ring(batch)
    assert np.array_equal(_launch(plain.ring, None, _identity(B), B), batch.astype(np.float32))
    ring.untouched(frames)
    plain.untouched(batch)


# ------------------------------------------------------------------------------------------------ 7. random weights
def _mixed_bytes(rs, shape):
    """Seeded random bytes with runs of 0, 1, 127 and 255 mixed in (a quarter of the elements), 255 and 0 in the corners."""
    x = rs.randint(0, 256, shape, dtype=np.uint8)
    flat = x.reshape(-1)
    pick = rs.rand(flat.size) < 0.25
    flat[pick] = rs.choice(np.array([0, 1, 127, 255], dtype=np.uint8), int(pick.sum()))
    flat[0], flat[-1] = 255, 0
    return x


def _drawn_weights(seed, n):
    torch.manual_seed(seed)
    return _conv_cls()((1, 1)).draw_weights(n).numpy()


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("C", [3, 6, 9, 12])
@pytest.mark.parametrize("H,W", [(1, 1), (5, 13), (23, 29), (1, 257)])
def test_random_weights_against_float64(H, W, C, B):
    """Weights from ``draw_weights`` at a fixed seed; HW = 1, 65 (a wave and a lane), 667 (ten waves and a tail of 27) and
    257 in one row (a fifth wave of one lane); gathered rows with a repeat, and idx = None; every element within the
    derived bound."""
    rs = np.random.RandomState(1000 * H + 10 * C + B)
    frames = _mixed_bytes(rs, (B + 2, H, W, C))
    rows = rs.randint(0, B + 2, B)
    rows[-1] = rows[0]
    w = _drawn_weights(H * W + C, B)
    ring = _Ring(frames)
    for name, src, idx, batch in (("gathered", ring, torch.from_numpy(rows).cuda(), frames[rows]),
                                  ("idx=None", ring, None, frames[:B])):
        got = _launch(src.ring, idx, w, B)
        ref, bound = _ref_and_bound(batch, w)
        err = np.abs(got.astype(np.float64) - ref)
        ratio = float((err / np.maximum(bound, 1e-300)).max())
        _seen[C] = max(_seen.get(C, 0.0), ratio)
        print(f"C={C} B={B} {H}x{W} {name}: worst |kernel - f64| = {err.max():.3e}, worst / bound = {ratio:.3f} "
              f"(worst ratio for C={C} so far: {_seen[C]:.3f})")
        where = np.unravel_index(int((err - bound).argmax()), err.shape)
        assert bool((err <= bound).all()), (name, where, err[where], bound[where])
        if H * W > 64:  # (a real, unclamped result)
            assert float(ref.max()) > 1.0 and float(ref.min()) < -1.0 and float(got.min()) < -1.0
    ring.untouched(frames)


# ------------------------------------------------------------------------------------------------ 8. NCHW
@pytest.mark.parametrize("C", [3, 12])
@pytest.mark.parametrize("H,W", [(5, 13), (23, 29)])
def test_nchw_equals_nhwc(H, W, C):
    """``curla_random_conv_nchw`` on the float image of the same bytes: the NHWC kernel's output transposed -- within
    twice the bound of test 7, and in fact bit for bit (both run one fmaf chain per output in the same order)."""
    from curla_amd import ops
    B = 5
    rs = np.random.RandomState(H + C)
    batch = _mixed_bytes(rs, (B, H, W, C))
    w = _drawn_weights(H + C, B)
    ring = _Ring(batch)
    nhwc = _launch(ring.ring, None, w, B)
    x_host = torch.from_numpy(_nchw(batch).astype(np.float32))
    x = x_host.cuda()
    buf, out = _guarded(tuple(x.shape))
    ops.random_conv_nchw(x, torch.from_numpy(w).cuda(), out)
    got = _guards_intact(buf, out).numpy()
    assert torch.equal(x.cpu(), x_host)
    _, bound = _ref_and_bound(batch, w)
    assert bool((np.abs(got.astype(np.float64) - _nchw(nhwc).astype(np.float64)) <= 2 * _nchw(bound)).all())
    assert np.array_equal(got, _nchw(nhwc))
    ring.untouched(batch)


def test_training_augmentation_returns_a_new_tensor_and_aliasing_raises():
    import curla_amd
    from curla_amd import _lib, ops
    B, C, H, W = 3, 9, 7, 9
    rs = np.random.RandomState(8)
    imgs = _mixed_bytes(rs, (B, C, H, W))
    aug = curla_amd.RandomConv((H, W))
    w = _drawn_weights(8, B)
    x = torch.from_numpy(imgs.astype(np.float32)).cuda()
    x_before = x.clone()
    out = aug.training_augmentation(x, weights=torch.from_numpy(w))
    assert out is not x and out.data_ptr() != x.data_ptr() and out.shape == x.shape and out.dtype == torch.float32
    assert torch.equal(x, x_before)
    conv = curla_amd.RandomConv.conv
    assert bool((np.abs(out.cpu().numpy().astype(np.float64) - conv(imgs, w)) <= G * conv(imgs, np.abs(w.astype(np.float64)))).all())
    # without ``weights`` the filters come from draw_weights: torch's CPU generator, one draw
    torch.manual_seed(9)
    drawn = aug.training_augmentation(x)
    torch.manual_seed(9)
    assert torch.equal(drawn, aug.training_augmentation(x, weights=aug.draw_weights(B)))
    assert torch.equal(x, x_before)
    d_w = torch.from_numpy(w).cuda()
    with pytest.raises(_lib.CurlaHipError, match="overlaps"):
        ops.random_conv_nchw(x, d_w, x)
    store = torch.zeros(2 * x.numel(), device="cuda")
    a, b = store[:x.numel()].view(x.shape), store[4:x.numel() + 4].view(x.shape)
    with pytest.raises(_lib.CurlaHipError, match="overlaps"):
        ops.random_conv_nchw(a, d_w, b)
    assert _lib.load().curla_random_conv_nchw(x.data_ptr(), d_w.data_ptr(), B, C, H, W, x.data_ptr(), None) == -1
    torch.cuda.synchronize()
    assert torch.equal(x, x_before)


def test_entry_points_refuse_what_they_cannot_do():
    from curla_amd import _lib
    lib = _lib.load()
    ring = _Ring(np.zeros((1, 4, 4, 3), dtype=np.uint8))
    w = torch.zeros(81, device="cuda")
    out = torch.empty(64, device="cuda")
    args = lambda B, C, H, W: (ring.ring.data_ptr(), None, w.data_ptr(), B, C, H, W, out.data_ptr(), None)  # noqa: E731
    assert lib.curla_random_conv(*args(1, 4, 4, 4)) == -1      # C % 3
    assert lib.curla_random_conv(*args(0, 3, 4, 4)) == -1
    assert lib.curla_random_conv(*args(1, 3, 1 << 15, 1 << 15)) == -3  # a frame of 3 * 2^30 bytes: before any launch
    assert lib.curla_random_conv(*args(1, 12, 1, 4000)) == -3          # a row too long for the LDS tile
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 9. buffer routes
def _filled(dedup, staged):
    import curla_amd
    from tests.test_gpu_graph_aug import _episode
    C, hw, B = 9, (12, 10), 4
    aug = curla_amd.RandomConv(hw)
    kw = dict(staged_aug=True) if staged else {}
    rb = curla_amd.ReplayBuffer((C,) + hw, (2,), 32, B, torch.device("cuda"), aug, dedup_frames=dedup, **kw)
    rb.add_batch(*_episode(24, C // 3, hw, 9))
    return rb, aug


@pytest.mark.parametrize("staged", [False, True], ids=["default", "staged"])
@pytest.mark.parametrize("dedup", [False, True], ids=["plain", "dedup"])
def test_buffer_routes(dedup, staged, monkeypatch):
    """``sample_cpc`` and ``sample_cpc_refs`` of a small buffer with injected weights: obs, next_obs and pos are
    ``RandomConv.conv`` of the stored stacks at the drawn indices, each with ITS weight set (pos: not obs's), within the
    bound; the handles decode to the tensors ``sample_cpc`` returns, bit for bit."""
    rb, aug = _filled(dedup, staged)
    assert rb.staged_aug is staged
    B = rb.batch_size
    recorded = [torch.from_numpy(_drawn_weights(90 + j, B)) for j in range(3)]
    queue = []
    monkeypatch.setattr(aug, "draw_weights", lambda n: queue.pop(0).clone())
    np.random.seed(9)
    idxs, offs = rb.draw_indices()
    assert not offs.any()
    stored = rb.stacks(0, 24, 0), rb.stacks(0, 24, 1)
    conv = _conv_cls().conv
    queue[:] = recorded
    obs, act, rew, nxt, nd, kw = rb.sample_cpc(indices=(idxs, offs))
    assert not queue and kw["obs_anchor"] is obs
    got = [t.cpu().numpy().astype(np.float64) for t in (obs, nxt, kw["obs_pos"])]
    for j, (name, src) in enumerate((("obs", stored[0]), ("next_obs", stored[1]), ("pos", stored[0]))):
        imgs, w = src[idxs], recorded[j].numpy()
        bound = G * conv(imgs, np.abs(w.astype(np.float64)))
        assert got[j].shape == imgs.shape and bool((np.abs(got[j] - conv(imgs, w)) <= bound).all()), name
    # pos went through its own filters: it is not obs's result
    wrong = G * conv(stored[0][idxs], np.abs(recorded[0].numpy().astype(np.float64)))
    assert not bool((np.abs(got[2] - conv(stored[0][idxs], recorded[0].numpy())) <= wrong).all())
    assert not torch.equal(recorded[0], recorded[2])
    queue[:] = recorded
    r_obs, r_act, r_rew, r_nxt, r_nd, r_kw = rb.sample_cpc_refs(indices=(idxs, offs))
    assert not queue
    for ref, t in ((r_obs, obs), (r_nxt, nxt), (r_kw["obs_pos"], kw["obs_pos"])):
        assert tuple(ref.src.shape) == (B, 12, 10, 9) and torch.equal(ref.src.permute(0, 3, 1, 2), t)
    assert torch.equal(r_obs.pair[0].src[:B], r_obs.src) and torch.equal(r_obs.pair[0].src[B:], r_nxt.src)
    assert torch.equal(r_act, act) and torch.equal(r_rew, rew) and torch.equal(r_nd, nd)


# ------------------------------------------------------------------------------------------------ 10. whole updates
def test_graph_replay_is_the_eager_update_bit_for_bit():
    """The geometry and the 14 mixed steps of tests/test_gpu_graph_aug.py (0, 5, 10 log and run eagerly; 1, 2 warm up;
    3, 4, 6, 7 capture; 8, 9, 11, 12, 13 replay) on a ``staged_aug=True`` RandomConv buffer: parameters, targets, Adam
    moments, losses and all random streams end where the eager run ends; a replayed step launches nothing from the host;
    the guard bytes around the graph slots' float buffers are intact."""
    from tests.test_gpu_graph_aug import _run
    setup = dict(aug="random_conv", staged_aug=True)
    eager, calls_e, logs_e, _, _ = _run(False, **setup)
    graph, calls_g, logs_g, agent, rb = _run(True, **setup)
    replayed = [8, 9, 11, 12, 13]
    assert all(calls_e[s].get("curla_random_conv") == 3 for s in range(14))
    assert [sum(calls_g[s].values()) for s in replayed] == [0] * len(replayed), calls_g
    assert all(calls_g[s].get("curla_random_conv") == 3 for s in (0, 1, 2, 3, 4, 5, 6, 7, 10)), calls_g
    assert len(agent._graphs) == 2 and all(len(r) == 2 and all(g["graph"] is not None for g in r)
                                           for r in agent._graphs.values())
    assert logs_e == logs_g and logs_e
    for k in eager:
        assert torch.equal(eager[k], graph[k]), k
    assert float(eager["critic_steps"][0]) == 14
    blocks = rb._graph_blocks
    assert len(blocks) == 4
    for g in blocks.values():
        assert len(g["guards"]) == 3  # | both | pos |
        for guard in g["guards"]:
            assert guard.numel() >= rb.GUARD and bool((guard == rb.GUARD_BYTE).all())
        assert bool(g["both_f32"].ne(0).any()) and bool(g["pos_f32"].ne(0).any())
        assert float(g["both_f32"].min()) < 0.0  # (convolved, unclamped frames, not an empty buffer)


def test_an_unstaged_buffer_is_refused_by_enable_update_graphs():
    import curla_amd
    from tests.test_gpu_graph_aug import _build
    agent, rb = _build("random_conv")
    assert isinstance(rb.augmentor, curla_amd.RandomConv) and not rb.staged_aug and not rb.graph_supported()
    with pytest.raises(ValueError, match="RandomConv.*staged_aug=True"):
        agent.enable_update_graphs(rb)
    assert _build("random_conv", staged_aug=True)[1].graph_supported()
