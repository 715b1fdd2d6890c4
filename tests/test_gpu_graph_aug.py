"""Update graphs for the float augmentations (``ReplayBuffer(..., staged_aug=True)``) and the de-duplicated frame
store, and the NoisyCover kernel that draws its own noise (``curla_noisy_cover_rng``).

Whatever must be bit-identical is compared with ``torch.equal``; the only tolerances are the one of the NumPy
restatement of Philox4x32-10 + Box-Muller (float32 transcendentals of another library) and the derived sampling
bounds of a mean and a standard deviation."""
import collections

import numpy as np
import pytest
import torch

from tests.test_gpu_agent import HP, NullLogger

pytestmark = pytest.mark.gpu

SETUPS = {
    "color_jiggle+staged": dict(aug="color_jiggle", staged_aug=True),
    "noisy_cover+staged": dict(aug="noisy_cover", staged_aug=True),
    "random_crop+dedup": dict(aug="random_crop", dedup_frames=True),
    "color_jiggle+staged+dedup": dict(aug="color_jiggle", staged_aug=True, dedup_frames=True),
}
AUG_KERNELS = ("curla_color_jiggle", "curla_noisy_cover", "curla_noisy_cover_rng", "curla_sample_stage",
               "curla_gather_stacks")


def _episode(n, k, hw, seed):
    """n frame-stacked transitions of one long run of episodes (an episode ends every 7th step): obs[t + 1] is
    next_obs[t] inside an episode, so the de-duplicating store finds the shared frames."""
    rs = np.random.RandomState(seed)
    obs, nxt, done = [], [], []
    stack = None
    for t in range(n):
        if stack is None:
            stack = [rs.randint(0, 256, (3,) + hw, dtype=np.uint8)] * k
        new = stack[1:] + [rs.randint(0, 256, (3,) + hw, dtype=np.uint8)]
        obs.append(np.concatenate(stack)), nxt.append(np.concatenate(new))
        d = t % 7 == 6
        done.append(d)
        stack = None if d else new
    return (np.stack(obs), rs.uniform(-1, 1, (n, 2)).astype(np.float32), rs.randn(n).astype(np.float32), np.stack(nxt),
            np.array(done))


def _build(aug, staged_aug=False, dedup_frames=False, B=64, seed=5):
    import curla_amd
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    np.random.seed(seed)
    dev = torch.device("cuda")
    C, in_hw = 9, (40, 44)
    augmentor = curla_amd.make_augmentor(aug, in_hw, (32, 36) if aug == "random_crop" else None)
    out_hw = tuple(augmentor.output_shape)
    agent = curla_amd.CurlSacAgent((C,) + out_hw, (2,), dev, augmentor, hidden_dim=64, **{**HP, "log_interval": 5})
    kw = dict(staged_aug=True) if staged_aug else {}
    rb = curla_amd.ReplayBuffer((C,) + in_hw, (2,), 512, B, dev, augmentor, dedup_frames=dedup_frames, **kw)
    rb.add_batch(*_episode(400, C // 3, in_hw, 6))
    return agent, rb


def _state(agent, rb):
    dev = agent.device
    state = {"critic": agent._critic_flat, "target": agent._target_flat, "actor": agent._actor_flat,
             "log_alpha": agent.log_alpha.detach(), "rng_device": torch.cuda.get_rng_state(dev),
             "rng_torch_cpu": torch.get_rng_state(), "scalars": agent._ws(rb.batch_size).scalars}
    for name, opt in (("critic", agent.critic_optimizer), ("actor", agent.actor_optimizer),
                      ("encoder", agent.encoder_optimizer), ("cpc", agent.cpc_optimizer)):
        state[name + "_m"], state[name + "_v"] = opt._m, opt._v
        state[name + "_steps"] = torch.tensor(opt._steps)
    la = agent.log_alpha_optimizer.state[agent.log_alpha]
    state["la_m"], state["la_v"], state["la_step"] = la["exp_avg"], la["exp_avg_sq"], la["step"]
    state = {k: v.detach().cpu().clone() for k, v in state.items()}
    np_state = np.random.get_state()
    state["numpy_keys"] = torch.from_numpy(np_state[1].astype(np.int64))
    state["numpy_pos"] = torch.tensor([np_state[2], np_state[3]])
    return state


def _run(graphs, steps=14, **setup):
    import curla_amd.ops as ops_mod
    import curla_amd.optim as optim_mod
    from curla_amd import _lib
    agent, rb = _build(**setup)
    if graphs:
        agent.enable_update_graphs(rb)
    real_call, counter, per_step = _lib.call, collections.Counter(), []

    def traced(name, *a):
        counter[name] += 1
        return real_call(name, *a)
    for m in (ops_mod, optim_mod):
        m.call = traced
    L = NullLogger()
    try:
        for step in range(steps):
            counter.clear()
            agent.update(rb, L, step)
            per_step.append(dict(counter))
        torch.cuda.synchronize()
    finally:
        for m in (ops_mod, optim_mod):
            m.call = real_call
    return _state(agent, rb), per_step, dict(L.scalars), agent, rb


@pytest.mark.parametrize("name", list(SETUPS))
def test_graph_replay_is_the_eager_update_bit_for_bit(name):
    """14 mixed even / odd steps (0, 5, 10 log and run eagerly; 1, 2 warm up; 3, 4, 6, 7 capture; 8, 9, 11, 12, 13
    replay): parameters, targets, Adam moments, step counts, log_alpha and all three random streams (device generator,
    torch's CPU generator, NumPy) end where the eager run ends; a replayed step makes no kernel call from the host, in
    particular no jitter / cover / staging / gather launch and no parameter copy."""
    setup = SETUPS[name]
    eager, calls_e, logs_e, _, _ = _run(False, **setup)
    graph, calls_g, logs_g, agent, rb = _run(True, **setup)
    replayed = [8, 9, 11, 12, 13]
    assert all(sum(calls_e[s].values()) > 15 for s in range(14))
    assert [sum(calls_g[s].values()) for s in replayed] == [0] * len(replayed), calls_g
    assert all(sum(calls_g[s].values()) > 15 for s in (0, 1, 2, 3, 4, 5, 6, 7, 10)), calls_g
    # the eager steps of both runs launch the minibatch kernels from the host, the replayed ones do not
    used = [k for k in AUG_KERNELS if calls_e[8].get(k)]
    assert "curla_sample_stage" in used and len(used) >= 2, calls_e[8]
    assert all(calls_g[s].get(k, 0) == 0 for s in replayed for k in AUG_KERNELS)
    assert len(agent._graphs) == 2 and all(len(r) == 2 and all(g["graph"] is not None for g in r)
                                           for r in agent._graphs.values())
    assert logs_e == logs_g
    for k in eager:
        assert torch.equal(eager[k], graph[k]), k
    assert float(eager["critic_steps"][0]) == 14 and float(eager["actor_steps"][0]) == 7
    # guard bytes around the graph slots' minibatch buffers: untouched by captures and replays
    blocks = rb._graph_blocks
    assert len(blocks) == 4 and all(len(g["guards"]) >= 2 for g in blocks.values())
    for g in blocks.values():
        for guard in g["guards"]:
            assert guard.numel() >= rb.GUARD and bool((guard == rb.GUARD_BYTE).all())
        if "mb_u8" in g:  # (the 32 bytes of loader slack behind the stacks are read, never written)
            assert not bool(g["mb_u8"][-32:].any())


def test_guard_bytes_around_the_graph_slot_buffers_after_a_replay():
    """The per-graph-slot minibatch buffers (uint8 stacks of the de-duplicated store, float [2B] + [B] tensors of the
    augmentation) are written in full and nowhere else: after captures and replays every buffer has been filled
    (NoisyCover output is never exactly the zero it was initialised with everywhere) and every guard byte in front of,
    between and behind them still holds the fill pattern."""
    _, calls, _, agent, rb = _run(True, steps=12, aug="noisy_cover", staged_aug=True, dedup_frames=True)
    assert sum(calls[11].values()) == 0  # step 11 replayed
    for g in rb._graph_blocks.values():
        assert len(g["guards"]) == 5  # | stacks | and | both | pos |
        for guard in g["guards"]:
            assert bool((guard == rb.GUARD_BYTE).all())
        assert bool(g["both_f32"].ne(0).any()) and bool(g["pos_f32"].ne(0).any()) and bool(g["mb_u8"].any())
        assert float(g["both_f32"].min()) >= 0.0 and float(g["both_f32"].max()) <= 255.0


def test_staged_color_jiggle_eager_is_the_default_buffer_bit_for_bit():
    """Same seeds, 3 updates: the float minibatches a ``staged_aug`` buffer hands to the learner and the parameters
    after the updates equal the default buffer's (per-call pinned block + copy), and so do all host streams."""
    outs = []
    for staged in (False, True):
        agent, rb = _build("color_jiggle", staged_aug=staged)
        assert rb.staged_aug is staged
        batches = []
        real = rb.sample_cpc_refs

        def spy(*a, **k):
            s = real(*a, **k)
            batches.append([s[0].pair[0].src.clone(), s[5]["obs_pos"].src.clone()])
            return s
        rb.sample_cpc_refs = spy
        L = NullLogger()
        for step in range(3):
            agent.update(rb, L, step)
        torch.cuda.synchronize()
        outs.append((batches, _state(agent, rb)))
    (b0, s0), (b1, s1) = outs
    assert len(b0) == len(b1) == 3
    for x, y in zip(b0, b1):
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
        assert float(x[0].max()) > 1.0  # (a real [0, 255] minibatch, not an empty buffer)
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k


def test_default_float_buffers_stay_refused_and_the_error_names_the_flag():
    import curla_amd
    agent, rb = _build("noisy_cover")
    assert not rb.graph_supported()
    with pytest.raises(ValueError, match="staged_aug=True"):
        agent.enable_update_graphs(rb)
    assert _build("noisy_cover", staged_aug=True)[1].graph_supported()
    assert _build("random_crop", dedup_frames=True)[1].graph_supported()
    assert isinstance(rb.augmentor, curla_amd.NoisyCover)


# ---------------------------------------------------------------------------------------------------- the kernel
def _philox_normals(seed, offset, n):
    """NumPy restatement of the stream (include/curla_hip.h): element i = Box-Muller, in float32, on outputs
    (i % 4) & 2, + 1 of Philox4x32-10 with key ``seed`` and counter ``offset + i // 4``; cos for even i, sin for odd."""
    m = (n + 3) // 4
    ctr = np.uint64(offset) + np.arange(m, dtype=np.uint64)
    mask = np.uint64(0xFFFFFFFF)
    c0, c1 = ctr & mask, ctr >> np.uint64(32)
    c2, c3 = np.zeros(m, np.uint64), np.zeros(m, np.uint64)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        n0, n2 = (p1 >> np.uint64(32)) ^ c1 ^ k0, (p0 >> np.uint64(32)) ^ c3 ^ k1
        c1, c3, c0, c2 = p1 & mask, p0 & mask, n0, n2
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & mask, (k1 + np.uint64(0xBB67AE85)) & mask
    r = np.stack([c0, c1, c2, c3], 1)
    out = np.empty((m, 4), np.float32)
    for h in range(2):
        a, b = r[:, 2 * h] >> np.uint64(8), r[:, 2 * h + 1] >> np.uint64(8)
        u1 = (a.astype(np.float32) + np.float32(1)) * np.float32(1.0 / 16777216.0)
        u2 = b.astype(np.float32) * np.float32(1.0 / 16777216.0)
        rad = np.sqrt(np.float32(-2) * np.log(u1))
        ang = np.float32(6.283185307179586) * u2
        out[:, 2 * h], out[:, 2 * h + 1] = rad * np.cos(ang), rad * np.sin(ang)
    return out.reshape(-1)[:n]


def _head_normals(ops, seed, offset, n):
    """The policy head's in-kernel draw of the first n numbers of the stream (ops.actor_head_fwd, rng=)."""
    A = 8
    B = (n + A - 1) // A
    nz = torch.full((B, A), float("nan"), device="cuda")
    ops.actor_head_fwd(torch.zeros(B, 2 * A, device="cuda"), nz, B, A, -10.0, 2.0, pi=torch.empty(B, A, device="cuda"),
                       log_pi=torch.empty(B, 1, device="cuda"), rng=(seed, offset))
    return nz.flatten()[:n]


# worst |head kernel - NumPy restatement| over 2^20 numbers, measured on the MI355X (see the docstring below)
HEAD_VS_NUMPY = 4.76837158203125e-07  # = 2^-21


def _ring(n, C, H, W, seed):
    frames = np.random.RandomState(seed).randint(0, 256, (n, H, W, C), dtype=np.uint8)
    store = torch.zeros(frames.size + 32, dtype=torch.uint8, device="cuda")
    ring = store[:frames.size].view(n, H, W, C)
    ring.copy_(torch.from_numpy(frames))
    return ring


@pytest.mark.parametrize("C", [3, 6, 9, 12])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("form", ["by_value", "device"])
def test_noisy_cover_rng_equals_the_explicit_noise_kernel(C, B, form):
    """curla_noisy_cover_rng against curla_noisy_cover on odd H / W (groups of four elements straddle samples and
    leave the dword grid), gathered rows, by-value and device-memory (rng_dev / colors_dev) forms: the output IS the
    explicit-noise kernel's output on ``noise_out`` (cover rows and clamping are pinned through that kernel to
    tests/golden/noisy_cover.npz, tests/test_gpu_augment.py); ``noise_out`` is std times the policy head's draw of the
    same (seed, offset), bit for bit, and matches the NumPy restatement of Philox4x32-10 + Box-Muller.

    Bound of the restatement: there was no such comparison for the head, so the EXISTING head kernel was measured
    against the same restatement first -- worst |difference| over 2^20 numbers: 4.77e-07 (HEAD_VS_NUMPY; float32
    log / sin / cos of two libraries) -- and the bound is twice that, times std."""
    from curla_amd import ops
    H, W, std, top, bottom = 21, 23, 10.0, 7, 5
    seed, off = 0x1234_5678_9ABC_DEF1, 2 ** 33 + 77
    colors = [17.0, 203.0, 99.0]
    ring = _ring(9, C, H, W, 10 * C + B)
    idx = torch.from_numpy(np.random.RandomState(B).randint(0, 9, B)).cuda()
    n = B * H * W * C
    store = torch.full((n + 8,), float("nan"), device="cuda")  # (+ a view that starts off the 16-byte grid)
    for out in (store[:n].view(B, H, W, C), store[1:n + 1].view(B, H, W, C)):
        store.fill_(float("nan"))
        nz = torch.full((B, H, W, C), float("nan"), device="cuda")
        if form == "by_value":
            ops.noisy_cover_rng(ring, idx, std, (seed, off), colors, top, bottom, B, out, noise_out=nz)
        else:
            ctl = torch.zeros(32, dtype=torch.uint8, device="cuda")
            ctl[:12].view(torch.float32).copy_(torch.tensor(colors))
            ctl[16:].view(torch.int64).copy_(torch.from_numpy(np.array([seed, off], np.uint64).view(np.int64)))
            ops.noisy_cover_rng(ring, idx, std, (1, 2, ctl.data_ptr() + 16), ctl.data_ptr(), top, bottom, B, out, noise_out=nz)
        ref = torch.full((B, H, W, C), float("nan"), device="cuda")
        ops.noisy_cover(ring, idx, nz, colors, top, bottom, B, ref)
        assert torch.equal(out, ref)
        assert bool(torch.isnan(store[n + 1:]).all())  # nothing behind the tensor
        # without noise_out (production): the same output
        out2 = torch.full((B, H, W, C), float("nan"), device="cuda")
        ops.noisy_cover_rng(ring, idx, std, (seed, off), colors, top, bottom, B, out2)
        assert torch.equal(out2, ref)
    assert float(ref.min()) == 0.0 and float(ref.max()) == 255.0  # (both clamps were exercised)
    assert torch.equal(nz.flatten(), std * _head_normals(ops, seed, off, n))
    want = std * _philox_normals(seed, off, n)
    worst = float(np.abs(nz.flatten().cpu().numpy() - want).max())
    print(f"noisy_cover_rng noise_out vs NumPy restatement C={C} B={B}: worst |diff| = {worst:.3e}")
    assert worst <= 2 * HEAD_VS_NUMPY * std


def test_existing_head_draw_against_the_numpy_restatement():
    """The measurement HEAD_VS_NUMPY comes from: the policy head's draw (unchanged by this module) against the NumPy
    restatement, 2^20 numbers -- printed, and held to the recorded figure so that the bound derived from it stays
    honest (measured on the MI355X: 4.77e-07)."""
    from curla_amd import ops
    n = 1 << 20
    got = _head_normals(ops, 4242, 10 ** 12, n).cpu().numpy()
    worst = float(np.abs(got - _philox_normals(4242, 10 ** 12, n)).max())
    print(f"head kernel vs NumPy restatement: worst |diff| = {worst:.3e}")
    assert worst <= HEAD_VS_NUMPY


def test_noisy_cover_rng_noise_statistics_and_disjoint_counters():
    """n = 1.8 M numbers at std 10: |mean| <= 6 std / sqrt(n) and |s / std - 1| <= 6 / sqrt(2 n) (six standard errors
    of a normal sample's mean and standard deviation; tests/test_graph_aug_host.py checks both bounds against NumPy's
    own normals).  Counters: a draw of n numbers uses [off, off + ceil(n / 4)); the next tensor's draw, at the offset
    the buffer assigns, shares none of them."""
    from curla_amd import ops
    B, H, W, C, std = 25, 85, 85, 10, 10.0   # n = 1 806 250: not a multiple of 4
    n = B * H * W * C
    ring = _ring(B, C, H, W, 3)

    def draw(seed, off):
        nz = torch.empty((B, H, W, C), device="cuda")
        ops.noisy_cover_rng(ring, None, std, (seed, off), [0, 0, 0], 0, 0, B, torch.empty_like(nz), noise_out=nz)
        return nz.flatten()
    a = draw(99, 1000)
    x = a.double()
    mean, s = float(x.mean()), float(x.std())
    print(f"noise_out statistics: n = {n} mean = {mean:.3e} (bound {6 * std / n ** 0.5:.3e}) "
          f"s/std - 1 = {s / std - 1:.3e} (bound {6 / (2 * n) ** 0.5:.3e})")
    assert n >= 10 ** 6 and abs(mean) <= 6 * std / n ** 0.5 and abs(s / std - 1) <= 6 / (2 * n) ** 0.5
    cnt = (n + 3) // 4
    b = draw(99, 1000 + cnt)  # the next tensor's range [1000 + cnt, 1000 + 2 cnt)
    assert not bool((a == b).any())
    # one counter further = the stream shifted by four numbers: counter off + j is used by elements 4 j .. 4 j + 3 only
    c = draw(99, 1001)
    assert torch.equal(c[:n - 4], a[4:])
    # ... and so the last counter of the first range is not the first of the second
    assert not torch.equal(b[:4], draw(99, 1000 + cnt - 1)[:4])


def test_buffer_assigns_consecutive_disjoint_counter_ranges():
    """The ranges [counter, counter + ceil(n / 4)) of obs, next_obs, pos and the two policy draws of an update, as the
    staged NoisyCover buffer and the agent take them from the device generator, are disjoint and consecutive."""
    agent, rb = _build("noisy_cover", staged_aug=True)
    gen = torch.cuda.default_generators[torch.cuda.current_device()]
    start = gen.get_offset()
    draws = rb.draw_aug()
    c, h, w = rb.obs_shape
    cnt = (rb.batch_size * c * h * w + 3) // 4
    ctrs = [d[2] for d in draws]
    assert ctrs == [start // 4 + j * cnt for j in range(3)]
    assert all(d[1] == gen.initial_seed() for d in draws)
    assert gen.get_offset() == start + 3 * 4 * cnt
    # an eager update continues behind them: 3 more tensors, then the critic- and actor-phase policy draws
    agent.update(rb, NullLogger(), 2)  # (an even step: critic and actor phase)
    pol = 4 * ((rb.batch_size * 2 + 3) // 4)
    assert gen.get_offset() == start + 6 * 4 * cnt + 2 * pol


def test_noisy_cover_rng_refuses_what_it_cannot_number():
    from curla_amd import _lib
    lib = _lib.load()
    ring = _ring(1, 3, 4, 4, 0)
    out = torch.empty(64, device="cuda")
    args = lambda B, H, W: (ring.data_ptr(), None, 1.0, 1, 0, None, 0.0, 0.0, 0.0, None, 0, 0, B, 3, H, W,  # noqa: E731
                            out.data_ptr(), None, None)
    assert lib.curla_noisy_cover_rng(*args(65536, 256, 128)) == -3  # B H W C = 3 * 2^31 >= 2^32: before any launch
    assert lib.curla_noisy_cover_rng(*args(0, 4, 4)) == -1
    torch.cuda.synchronize()
