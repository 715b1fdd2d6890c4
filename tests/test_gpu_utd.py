"""CurlSacAgent(utd_ratio=G) on the MI355X.  The contract: a call with ``utd_ratio = G`` leaves, bit for
bit, the state of a twin agent with ``utd_ratio = 1`` that makes G-1 critic-only ``update()`` calls -- at a ``step``
without actor and CURL phase and with the same soft-update decision -- and then the ordinary call.  State: parameters,
targets, every Adam moment and step count, log_alpha, priorities, the device generator and NumPy's stream.  Both agents
start from the same seeds, each with its own identically filled buffer.  Geometry and batch size are
tests/test_gpu_graph.py's; the critics carry LayerNorm and dropout 0.1, so the masks take part."""
import collections
import socket

import numpy as np
import pytest
import torch

from tests.test_gpu_agent import HP, NullLogger

pytestmark = pytest.mark.gpu

B, HIDDEN, C, IN_HW, OUT_HW = 256, 64, 9, (40, 44), (32, 36)
# actor and CURL phase every 4th step: every other step is a critic-only update; LOG_AT: one logging step in each run
LOG_AT = 5
FREQ = dict(actor_update_freq=4, cpc_update_freq=4, log_interval=LOG_AT)
DROQ = dict(critic_layer_norm=True, critic_dropout=0.1)


def _lead_step(step, freq):
    """A step whose update is critic-only, with the soft-update decision of ``step``, that logs nothing."""
    s = 2 if step % freq == 0 and freq == 2 else 1
    assert s % 4 and s % LOG_AT and (s % freq == 0) == (step % freq == 0)
    return s


class Foreign:
    """A buffer that is not this package's: ``sample_cpc()`` and nothing else."""

    def __init__(self, rb):
        self.rb, self.batch_size = rb, rb.batch_size

    def sample_cpc(self):
        return self.rb.sample_cpc()


def _episodes(n, seed):
    """n frame-stacked transitions of consecutive episodes (one ends every 7th step): next_obs[t] is obs[t + 1] inside
    an episode, as an environment's frame stack gives them -- what a dedup_frames buffer's frame store expects."""
    rs = np.random.RandomState(seed)
    frame = lambda: rs.randint(0, 256, (3,) + IN_HW, dtype=np.uint8)  # noqa: E731
    obs, nxt, stack = [], [], None
    for t in range(n):
        if stack is None:
            stack = [frame()] * (C // 3)
        new = stack[1:] + [frame()]
        obs.append(np.concatenate(stack)), nxt.append(np.concatenate(new))
        stack = None if t % 7 == 6 else new
    return (np.stack(obs), rs.uniform(-1, 1, (n, 2)).astype(np.float32), rs.randn(n).astype(np.float32), np.stack(nxt),
            (np.arange(n) % 7) == 6)


def _build(G, rb_kw=None, aug="crop", foreign=False, clip=None, hp=None):
    import curla_amd
    torch.manual_seed(5)
    np.random.seed(5)
    dev = torch.device("cuda")
    if aug == "crop":
        augmentor, out_hw = curla_amd.RandomCrop(IN_HW, OUT_HW), OUT_HW
    else:
        augmentor, out_hw = (curla_amd.RandomConv if aug == "conv" else curla_amd.RandomShift)(IN_HW), IN_HW
    agent = curla_amd.CurlSacAgent((C,) + out_hw, (2,), dev, augmentor, hidden_dim=HIDDEN, utd_ratio=G, **DROQ,
                                   **{**HP, **FREQ, **(hp or {})})
    if clip is not None:
        agent.set_max_grad_norm(clip)
    rb = curla_amd.ReplayBuffer((C,) + IN_HW, (2,), 512, B, dev, augmentor, **(rb_kw or {}))
    rb.add_batch(*_episodes(400, 6))
    torch.manual_seed(11)
    np.random.seed(11)
    return agent, (Foreign(rb) if foreign else rb), rb


def _state(agent, rb):
    torch.cuda.synchronize()
    state = {"critic": agent._critic_flat, "target": agent._target_flat, "actor": agent._actor_flat,
             "log_alpha": agent.log_alpha.detach(), "rng": torch.cuda.get_rng_state(agent.device),
             "torch_cpu": torch.get_rng_state(), "numpy": torch.from_numpy(np.random.get_state()[1].astype(np.int64)),
             "numpy_pos": torch.tensor(np.random.get_state()[2])}
    for name, opt in (("critic", agent.critic_optimizer), ("actor", agent.actor_optimizer),
                      ("encoder", agent.encoder_optimizer), ("cpc", agent.cpc_optimizer)):
        state[name + "_m"], state[name + "_v"] = opt._m, opt._v
        state[name + "_steps"] = torch.tensor(opt._steps)
        sd = opt.state_dict()["state"]
        state[name + "_sd_steps"] = torch.tensor([float(v["step"]) for v in sd.values()])
    la = agent.log_alpha_optimizer.state[agent.log_alpha]
    if la:
        state["la_m"], state["la_v"], state["la_step"] = la["exp_avg"], la["exp_avg_sq"], la["step"]
    if getattr(rb, "prioritized", False):
        state["priorities"] = torch.as_tensor(rb.priorities())
    return {k: v.detach().cpu().clone() for k, v in state.items()}


def _contract(G, steps, freq=2, **kw):
    """(state after the calls of a utd_ratio = G agent, state after the twin's G-1 critic-only calls + 1 per call)."""
    hp = dict(critic_target_update_freq=freq)
    agent, buf, rb = _build(G, hp=hp, **kw)
    L = NullLogger()
    for step in steps:
        agent.update(buf, L, step)
    got = _state(agent, rb), dict(L.scalars)
    twin, buf, rb = _build(1, hp=hp, **kw)
    L = NullLogger()
    for step in steps:
        for _ in range(G - 1):
            twin.update(buf, NullLogger(), _lead_step(step, freq))
        twin.update(buf, L, step)
    want = _state(twin, rb), dict(L.scalars)
    return got, want, agent


def _assert_same(got, want):
    assert got[0].keys() == want[0].keys()
    for k in want[0]:
        assert torch.equal(got[0][k], want[0][k]), k
    assert got[1] == want[1]  # what the logging steps logged


@pytest.mark.parametrize("freq", [1, 2])
@pytest.mark.parametrize("start", [4, 5], ids=["even", "odd"])
def test_contract_bit_for_bit(start, freq):
    steps = [start, start + 1, start + 2]
    got, want, agent = _contract(3, steps, freq)
    _assert_same(got, want)
    assert float(got[0]["critic_steps"][0]) == 9 and float(got[0]["actor_steps"][0]) == sum(s % 4 == 0 for s in steps)
    assert "train_critic/loss" in got[1] and bool(torch.isfinite(got[0]["critic"]).all())
    # the targets moved with every sub-step whose step says so: not what one soft update per call leaves
    one, _, _ = _contract(1, steps, freq)
    assert not torch.equal(one[0]["target"], got[0]["target"])


@pytest.mark.parametrize("name,kw", [
    ("prioritized", dict(rb_kw=dict(prioritized=True))),
    ("n_step", dict(rb_kw=dict(n_step=3, discount=HP["discount"]))),
    ("dedup_frames", dict(rb_kw=dict(dedup_frames=True))),
    ("staged RandomConv", dict(rb_kw=dict(staged_aug=True), aug="conv")),
    ("RandomShift", dict(aug="shift")),  # (leading sub-steps: the scratch launch of n = 2B)
    ("RandomShift, pos_offset", dict(aug="shift", rb_kw=dict(pos_offset=2))),
    ("dedup_frames, pos_offset", dict(rb_kw=dict(dedup_frames=True, pos_offset=2))),
    ("max_grad_norm", dict(clip=0.5)),
    ("foreign buffer", dict(foreign=True)),
], ids=lambda v: v if isinstance(v, str) else "")
def test_contract_on_further_buffers(name, kw):
    G = 2 if name == "foreign buffer" else 3
    got, want, agent = _contract(G, [4, 5, 6], 2, **kw)
    _assert_same(got, want)
    assert ("priorities" in got[0]) == (name == "prioritized")
    if name == "max_grad_norm":
        assert float(agent.grad_clip_stats[0, 1]) < 1.0  # (the critic's gradient really was clipped)


# --------------------------------------------------------------------------------------------------------------- graphs
def _graph_run(graphs, edit_at=None, calls=12):
    """``calls`` updates with G = 3 from step 1 on, HP's own frequencies (actor phase on even steps, CURL on all):
    the even and the odd kind, and in front of each its critic-only kind with / without a soft update."""
    import curla_amd.ops as ops_mod
    import curla_amd.optim as optim_mod
    from curla_amd import _lib
    agent, rb, _ = _build(3, hp=dict(actor_update_freq=2, cpc_update_freq=1, log_interval=10 ** 9))
    if graphs:
        agent.enable_update_graphs(rb, warm=1, depth=2)
    real_call, counter, per_call = _lib.call, collections.Counter(), []

    def traced(name, *a):
        counter[name] += 1
        return real_call(name, *a)
    mods = (ops_mod, optim_mod)
    for m in mods:
        m.call = traced
    L = NullLogger()
    try:
        for step in range(1, 1 + calls):
            counter.clear()
            if step == edit_at:
                agent.utd_ratio = 2
            agent.update(rb, L, step)
            per_call.append(sum(counter.values()))
    finally:
        for m in mods:
            m.call = real_call
    return _state(agent, rb), per_call, agent


@pytest.mark.parametrize("edit_at", [None, 8], ids=["G = 3", "G = 3, then 2"])
def test_graph_replays_are_the_eager_sub_steps_bit_for_bit(edit_at):
    eager, calls_e, _ = _graph_run(False, edit_at)
    graph, calls_g, agent = _graph_run(True, edit_at)
    for k in eager:
        assert torch.equal(eager[k], graph[k]), k
    assert min(calls_e) > 2 * 15  # every eager sub-step makes its launches from the host
    # four kinds: (actor, soft, CURL) of even and odd steps and the critic-only kind in front of each; every one has
    # been used more often than warm + 2 depth = 5 times, so both of its blocks were captured, replayed and rewritten
    kinds = {(True, True, True), (False, False, True), (False, True, False), (False, False, False)}
    assert set(agent._graphs) == kinds
    assert all(len(r) == 2 and all(g["graph"] is not None for g in r) for r in agent._graphs.values())
    assert all(agent._graph_seen[k] > 1 + 2 * 2 for k in kinds), agent._graph_seen
    # leading sub-steps in front of the six even / the six odd calls; edited: G = 3 up to step 7, G = 2 from step 8 on
    lead = (12, 12) if edit_at is None else (3 * 2 + 3 * 1, 4 * 2 + 2 * 1)
    assert (agent._graph_seen[(False, True, False)], agent._graph_seen[(False, False, False)]) == lead
    assert calls_g[-4:] == [0, 0, 0, 0], calls_g  # the late calls replay: no kernel call from the host
    assert float(eager["critic_steps"][0]) == (36 if edit_at is None else 7 * 3 + 5 * 2)


# -------------------------------------------------------------------------------------------------------- data parallel
@pytest.fixture(scope="module")
def nccl_world1():
    import torch.distributed as dist
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    yield dist
    dist.destroy_process_group()


def _dp_run(mode, steps=(3, 4, 5)):
    agent, rb, _ = _build(2)
    checks = []
    if mode is not None:
        agent.enable_data_parallel(single_rank_collectives=True, **mode)
        real = agent.check_replicas
        agent.check_replicas = lambda: (checks.append(1), real())[1]
    L = NullLogger()
    for step in steps:
        agent.update(rb, L, step)
    assert not agent._dp_pending
    return _state(agent, rb), dict(L.scalars), len(checks)


def test_one_rank_data_parallel_sub_steps_are_the_single_gpu_ones(nccl_world1):
    dist = nccl_world1
    base = _dp_run(None)
    calls, real = [], dist.all_reduce

    def spy(t, **k):
        calls.append(t.numel())
        return real(t, **k)
    dist.all_reduce = spy
    try:
        block = _dp_run(dict(overlap=False, check_every=1))
        n_block = len(calls)
        over = _dp_run(dict(overlap=True, check_every=0))
        n_over = len(calls) - n_block
    finally:
        dist.all_reduce = real
    for name, other in (("blocking", block), ("overlapped", over)):
        for k in base[0]:
            assert torch.equal(base[0][k], other[0][k]), (name, k)
        assert base[1] == other[1], name
    assert block[2] == 3 and over[2] == 0  # the replicas are checked once per call, not once per sub-step
    # steps 3, 4, 5: six critic buckets (one per sub-step), one actor and one CURL bucket (step 4) -- whole when
    # blocking (+ the three replica checks), the critic's and the CURL one in two pieces when overlapped
    assert n_block == 6 + 1 + 1 + 3 and n_over == 2 * 6 + 1 + 2, (n_block, n_over)
