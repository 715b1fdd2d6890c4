"""CurlSacAgent.reset_networks() and the reset schedule on the MI355X.  The shrink-and-perturb kernel
alone against its NumPy float32 restatement, bit for bit (three IEEE float32 operations per element: the tolerance is
zero): every size around a float4 and a workgroup, every split position, every misalignment of the three arrays,
NaN-filled guard bands, keep 0 / 1 by selection.  The agent: the state a reset leaves, that a reset agent goes on exactly
as a newly built one given its parameters, recovery from NaN, captured update graphs across a scheduled reset, one-rank
data parallel, prioritized / n-step buffers, and a checkpoint across a reset boundary."""
import itertools
import socket

import numpy as np
import pytest
import torch

from tests.test_gpu_critic_ln import HP, NullLogger

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 16
IN_HW, OUT_HW, HIDDEN, B, CAP = (34, 40), (28, 34), 96, 16, 64
KEEPS = (0.0, 0.5, 0.8, 1.0)


# ------------------------------------------------------------------------------------------------ 1. the kernel alone
def _ref(old, fresh, split, ka, kb):
    """The definition in NumPy float32: two products and a sum, each rounding once; keep 0 selects ``fresh``; keep 1
    leaves the element alone; 1 - keep formed in double and rounded to float32 once."""
    out = old.copy()
    for lo, hi, k in ((0, split, ka), (split, old.size, kb)):
        if k == 1.0:
            continue
        if k == 0.0:
            out[lo:hi] = fresh[lo:hi]
            continue
        k32, n32 = np.float32(k), np.float32(1.0 - k)
        out[lo:hi] = (k32 * old[lo:hi]) + (n32 * fresh[lo:hi])
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class _Arrays:
    """param / target / fresh of one size on the device, each in a NaN-filled buffer with GUARD + 0..3 floats in front
    and GUARD behind; ``run`` resets them from the host images, launches and returns the whole buffers."""

    def __init__(self, n, seed):
        rs = np.random.RandomState(seed)
        self.n = n
        self.host = {k: rs.randn(n).astype(np.float32) for k in ("param", "target", "fresh")}
        self.dev = {k: torch.empty(n + 2 * GUARD + 3, device="cuda") for k in self.host}
        self.img = {k: np.full(n + 2 * GUARD + 3, NAN, np.float32) for k in self.host}

    def run(self, offs, split, ka, kb, with_target=True, values=None):
        from curla_amd import ops
        views = {}
        for (k, h), o in zip(self.host.items(), offs):
            img = self.img[k]
            img[:] = NAN
            img[GUARD + o:GUARD + o + self.n] = h if values is None or k not in values else values[k]
            self.dev[k].copy_(torch.from_numpy(img))
            views[k] = self.dev[k][GUARD + o:GUARD + o + self.n]
            assert views[k].data_ptr() % 16 == 4 * o
        ops.shrink_perturb2(views["param"], views["target"] if with_target else None, views["fresh"], split, ka, kb)
        return {k: self.dev[k].cpu().numpy() for k in self.dev}

    def expect(self, offs, split, ka, kb, with_target=True, values=None):
        v = {k: (h if values is None or k not in values else values[k]) for k, h in self.host.items()}
        want = {}
        for (k, _), o in zip(self.host.items(), offs):
            img = np.full(self.n + 2 * GUARD + 3, NAN, np.float32)
            new = v[k] if k == "fresh" or (k == "target" and not with_target) else _ref(v[k], v["fresh"], split, ka, kb)
            img[GUARD + o:GUARD + o + self.n] = new
            want[k] = img
        return want

    def check(self, offs, split, ka, kb, with_target=True, values=None):
        got = self.run(offs, split, ka, kb, with_target, values)
        want = self.expect(offs, split, ka, kb, with_target, values)
        for k in want:  # the whole buffers: the guard bands are still the NaNs they were
            assert np.array_equal(_bits(got[k]), _bits(want[k])), (k, self.n, offs, split, ka, kb, with_target)
        return got


@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 257, 1025, 4099])
def test_kernel_against_numpy_bit_for_bit(n):
    """n = 1, 3: no whole float4; 4, 5: one, with and without a tail; 255 / 257: one workgroup's threads, one short and
    one over; 1025: a second workgroup of float4s with a tail; 4099: several.  Every split position, every misalignment
    of the three arrays on its own, with and without a target; the sixteen keep pairs rotate through them, and all
    sixteen run on the all-aligned (16-byte accesses) and on a misaligned (element-wise) placement."""
    arr = _Arrays(n, seed=n)
    splits = sorted({0, 1, n - 1, n})
    pairs = list(itertools.product(KEEPS, KEEPS))
    turn = 0
    for split in splits:
        for with_target in (True, False):
            for offs in itertools.product(range(4), repeat=3):
                ka, kb = pairs[turn % len(pairs)]
                turn += 5  # (coprime to 16: every pair comes up under varied placements)
                arr.check(offs, split, ka, kb, with_target)
            for offs in ((0, 0, 0), (1, 2, 3)):
                for ka, kb in pairs:
                    arr.check(offs, split, ka, kb, with_target)
    first = arr.run((0, 0, 0), n // 2, 0.8, 0.5)
    again = arr.run((0, 0, 0), n // 2, 0.8, 0.5)
    assert all(np.array_equal(_bits(first[k]), _bits(again[k])) for k in first), "a rerun changed bits"


@pytest.mark.parametrize("n,offs", [(5, (0, 0, 0)), (1025, (0, 0, 0)), (1025, (3, 1, 2)), (257, (0, 2, 0))])
def test_keep_zero_selects_and_keep_one_touches_nothing(n, offs):
    specials = np.array([NAN, np.inf, -np.inf, 1e-45, -1e-42, -0.0, 0.0, 3e38], np.float32)  # (1e-45, -1e-42: denormals)
    payload = np.array([0x7FC01234, 0xFFC00001, 0x7F800001, 0x00000001, 0x807FFFFF, 0x80000000], np.uint32)  # NaNs with
    # payloads, quiet and signalling; the smallest and the largest denormal; -0.0
    old_bits = np.resize(np.concatenate([specials.view(np.uint32), payload]), n)
    old = old_bits.view(np.float32).copy()
    arr = _Arrays(n, seed=n + 1)
    values = dict(param=old, target=old[::-1].copy())
    # keep == 0 over NaN / +-Inf / denormal old values: exactly fresh, in both arrays
    got = arr.check(offs, n, 0.0, 0.0, True, values)
    o_p, o_t = offs[0], offs[1]
    fresh_bits = _bits(arr.host["fresh"])
    assert np.array_equal(_bits(got["param"][GUARD + o_p:GUARD + o_p + n]), fresh_bits)
    assert np.array_equal(_bits(got["target"][GUARD + o_t:GUARD + o_t + n]), fresh_bits)
    # keep == 1 over -0.0, NaN payloads and denormals: every byte as it was (1 * p + 0 * f would lose -0.0 and NaNs'
    # payloads could change); also with a NaN / Inf fresh value, which is not read
    bad_fresh = np.resize(np.array([NAN, np.inf, -np.inf, 1.0], np.float32), n)
    values = dict(param=old, target=old[::-1].copy(), fresh=bad_fresh)
    got = arr.check(offs, n // 2, 1.0, 1.0, True, values)
    assert np.array_equal(_bits(got["param"][GUARD + o_p:GUARD + o_p + n]), old_bits)
    assert np.array_equal(_bits(got["target"][GUARD + o_t:GUARD + o_t + n]), old_bits[::-1])
    # the two sides of a split on their own: keep 1 in front of keep 0 and the other way round
    values = dict(param=old, target=old[::-1].copy())
    for split in sorted({1, n // 2, n - 1} - {0}):
        arr.check(offs, split, 1.0, 0.0, True, values)
        arr.check(offs, split, 0.0, 1.0, True, values)


# ---------------------------------------------------------------------------------------------------------- 2. the agent
def _seed(s):
    np.random.seed(s)
    torch.manual_seed(s)
    torch.cuda.manual_seed_all(s)


def make(seed=0, clip=None, **kw):
    import curla_amd
    aug = curla_amd.RandomCrop(IN_HW, OUT_HW)
    _seed(seed)
    agent = curla_amd.CurlSacAgent((9,) + OUT_HW, (2,), torch.device("cuda"), aug, hidden_dim=HIDDEN, **{**HP, **kw})
    if clip is not None:
        agent.set_max_grad_norm(clip)
    return agent, aug


def ring(aug, seed=1, n=40, **kw):
    import curla_amd
    rb = curla_amd.ReplayBuffer((9,) + IN_HW, (2,), CAP, B, torch.device("cuda"), aug, **kw)
    rs = np.random.RandomState(seed)
    rb.add_batch(rs.randint(0, 256, (n, 9) + IN_HW, dtype=np.uint8), rs.uniform(-1, 1, (n, 2)).astype(np.float32),
                 rs.randn(n).astype(np.float32), rs.randint(0, 256, (n, 9) + IN_HW, dtype=np.uint8), (np.arange(n) % 7) == 6)
    return rb


FLAT_OPTS = ("critic", "actor", "encoder", "cpc")


def _state(agent, rb=None):
    torch.cuda.synchronize()
    state = {"critic": agent._critic_flat, "target": agent._target_flat, "actor": agent._actor_flat,
             "log_alpha": agent.log_alpha.detach()}
    for name in FLAT_OPTS:
        opt = agent._optimizers()[name]
        state[name + "_m"], state[name + "_v"], state[name + "_steps"] = opt._m, opt._v, torch.tensor(opt._steps)
    la = agent.log_alpha_optimizer.state[agent.log_alpha]
    if la:
        state["la_m"], state["la_v"], state["la_step"] = la["exp_avg"], la["exp_avg_sq"], la["step"]
    if rb is not None and getattr(rb, "prioritized", False):
        state["priorities"] = torch.as_tensor(rb.priorities())
    return {k: v.detach().cpu().clone() for k, v in state.items()}


def _assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
        assert torch.equal(a[k].reshape(-1).view(torch.uint8), b[k].reshape(-1).view(torch.uint8)), k  # (bits: NaN == NaN)


def _fresh_draws(agent, count):
    """``count`` consecutive draws of the reset stream, made here by the recipe: torch's CPU generator at the seed, then
    per reset an Actor, a Critic and a rand(z, z), constructed as the agent's constructor constructs them."""
    from curla_amd.networks import Actor, Critic
    obs, act, hidden, feat, lo, hi, layers, filters = (9,) + OUT_HW, (2,), HIDDEN, HP["encoder_feature_dim"], \
        HP["actor_log_std_min"], HP["actor_log_std_max"], HP["num_layers"], HP["num_filters"]
    q_kw = dict(quantiles=agent.critic_quantiles) if agent.critic_quantiles else {}
    out = []
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(agent.reset_seed)
        for _ in range(count):
            actor = Actor(obs, act, hidden, feat, lo, hi, layers, filters)
            critic = Critic(obs, act, hidden, feat, layers, filters, layer_norm=agent.critic_layer_norm, **q_kw)
            out.append((actor, critic, torch.rand(feat, feat)))
    return out


def _named(agent):
    """name -> live tensor, for every parameter a reset may touch (the tied actor convs are the critic's)."""
    out = {"W": agent.CURL.W}
    out.update({"critic." + n: p for n, p in agent.critic.named_parameters()})
    out.update({"target." + n: p for n, p in agent.critic_target.named_parameters()})
    out.update({"actor." + n: p for n, p in agent.actor.named_parameters() if ".convs." not in n})
    return out


def _fresh_named(agent, draw):
    """The same names -> the fresh values in the layout the live tensors are held in (fc columns in (y, x, c) order)."""
    actor, critic, W = draw
    c = agent.critic.encoder.num_filters
    h, w = agent.critic.encoder.out_dim

    def yxc(n, p):
        p = p.detach()
        return p.reshape(p.shape[0], c, h, w).permute(0, 2, 3, 1).reshape(p.shape[0], -1) if n == "encoder.fc.weight" else p
    out = {"W": W}
    for n, p in critic.named_parameters():
        out["critic." + n] = out["target." + n] = yxc(n, p)
    out.update({"actor." + n: yxc(n, p) for n, p in actor.named_parameters() if ".convs." not in n})
    return {k: v.contiguous().numpy() for k, v in out.items()}


def _is_head(name):
    return ".Q1." in name or ".Q2." in name or name.startswith("actor.trunk")


@pytest.mark.parametrize("kw", [{}, dict(critic_layer_norm=True, critic_quantiles=5)], ids=["plain", "ln_tqc"])
def test_state_after_a_reset(kw):
    agent, aug = make(seed=2, reset_seed=3, **kw)
    rb, L = ring(aug), NullLogger()
    draws = _fresh_draws(agent, 4)
    ptrs = {k: v.data_ptr() for k, v in _named(agent).items()}
    init_la = float(np.log(HP["init_temperature"]))
    for i, k in enumerate((1.0, 0.8, 0.0)):
        for step in range(2 * i + 1, 2 * i + 3):
            agent.update(rb, L, step)
        torch.cuda.synchronize()
        assert agent.log_alpha.item() != init_la and agent.critic_optimizer._steps[0] > 0
        old = {n: p.detach().cpu().numpy().copy() for n, p in _named(agent).items()}
        agent.reset_networks(encoder_keep=k)
        torch.cuda.synchronize()
        fresh = _fresh_named(agent, draws[i])
        live = _named(agent)
        assert set(live) == set(fresh) == set(old)
        for n, p in live.items():
            got = p.detach().cpu().numpy()
            if _is_head(n):
                want = fresh[n]
            else:
                want = _ref(old[n].reshape(-1), fresh[n].reshape(-1), old[n].size, k, k).reshape(old[n].shape)
                if k == 1.0:
                    assert np.array_equal(_bits(want), _bits(old[n]))
            assert np.array_equal(_bits(got), _bits(want)), (k, n)
            assert p.data_ptr() == ptrs[n], n
        assert not agent._target_flat[:agent._lay["w"][1]].any()  # the target's unused W slot is not written
        for mine, theirs in zip(agent.actor.encoder.convs, agent.critic.encoder.convs):
            assert mine.weight is theirs.weight and mine.bias is theirs.bias
        for n in ("Q1", "Q2"):  # the target's Q functions are the critic's
            for a, b in zip(getattr(agent.critic, n).parameters(), getattr(agent.critic_target, n).parameters()):
                assert torch.equal(a, b)
        st = _state(agent)
        for name in FLAT_OPTS:
            assert not st[name + "_m"].any() and not st[name + "_v"].any() and not st[name + "_steps"].any(), name
            sd = agent._optimizers()[name].state_dict()["state"]
            assert all(float(s["step"]) == 0.0 for s in sd.values())
        assert not st["la_m"].any() and not st["la_v"].any() and float(st["la_step"]) == 0.0
        assert not agent._critic_gflat.any() and not agent._actor_gbucket.any() and float(agent.log_alpha.grad) == 0.0
        assert agent.log_alpha.item() == init_la and agent.reset_count == i + 1
    # alpha=False: log_alpha and its optimizer are left alone
    for step in (7, 8):
        agent.update(rb, L, step)
    before = _state(agent)
    agent.reset_networks(alpha=False)
    after = _state(agent)
    for k in ("log_alpha", "la_m", "la_v", "la_step"):
        assert torch.equal(before[k], after[k]), k
    assert float(after["la_step"]) > 0 and float(after["log_alpha"]) != init_la and not after["actor_m"].any()
    want = _fresh_named(agent, draws[3])["critic.Q1.trunk.0.weight"]
    assert np.array_equal(_bits(agent.critic.Q1.trunk[0].weight.detach().cpu().numpy()), _bits(want))


def _reset_then_fresh(kw, rb_kw=None, clip=None, pre=6, post=(7, 8, 9, 10), keep=0.8):
    """Agent A: ``pre`` updates, a reset, the ``post`` updates.  Agent A': the same up to the reset -- bit for bit A's
    state and its buffer's at that point --; agent B is then newly constructed, given A' parameters, targets and
    log_alpha, and makes the ``post`` updates on A' buffer.  The same global seeds in front of the ``post`` updates."""
    def upto_reset():
        agent, aug = make(seed=4, clip=clip, reset_seed=9, **kw)
        rb = ring(aug, **(rb_kw or {}))
        _seed(21)
        for step in range(1, pre + 1):
            agent.update(rb, NullLogger(), step)
        agent.reset_networks(encoder_keep=keep)
        return agent, rb, aug

    def go_on(agent, rb):
        _seed(33)
        L = NullLogger()
        for step in post:
            agent.update(rb, L, step)
        return _state(agent, rb), dict(L.scalars)
    a, rb_a, _ = upto_reset()
    a2, rb_a2, _ = upto_reset()
    _assert_same(_state(a, rb_a), _state(a2, rb_a2))
    b, _ = make(seed=77, clip=clip, **kw)
    with torch.no_grad():
        b._critic_flat.copy_(a2._critic_flat)
        b._target_flat.copy_(a2._target_flat)
        b._actor_flat.copy_(a2._actor_flat)
        b.log_alpha.copy_(a2.log_alpha)
    got, want = go_on(a, rb_a), go_on(b, rb_a2)
    return got, want, a


CONFIGS = [("plain", {}, None), ("ln_dropout", dict(critic_layer_norm=True, critic_dropout=0.01), None),
           ("tqc", dict(critic_quantiles=5), None), ("detach_encoder", dict(detach_encoder=True), None),
           ("clip_weight_decay", dict(weight_decay=1e-2), 1e-3)]


@pytest.mark.parametrize("name,kw,clip", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_a_reset_agent_goes_on_as_a_newly_built_one(name, kw, clip):
    got, want, agent = _reset_then_fresh(kw, clip=clip)
    _assert_same(got[0], want[0])
    assert got[1] == want[1] and "train_critic/loss" in got[1] and "train/curl_loss" in got[1]
    assert all(np.isfinite(v) for v in got[1].values())
    assert int(got[0]["critic_steps"][-1]) == 4 and int(got[0]["actor_steps"][0]) == 2 and float(got[0]["la_step"]) == 2.0
    if clip is not None:
        assert float(agent.grad_clip_stats[0, 1]) < 1.0  # (the critic's gradient really was clipped)


@pytest.mark.parametrize("name,rb_kw", [("prioritized", dict(prioritized=True)),
                                        ("n_step_pos_offset", dict(n_step=3, discount=HP["discount"], pos_offset=2))],
                         ids=["prioritized", "n_step_pos_offset"])
def test_other_buffers(name, rb_kw):
    got, want, _ = _reset_then_fresh({}, rb_kw=rb_kw, pre=3, post=(4, 5))
    _assert_same(got[0], want[0])
    assert got[1] == want[1] and all(np.isfinite(v) for v in got[1].values())
    if name == "prioritized":
        assert "priorities" in got[0] and float(got[0]["priorities"].max()) > 0


def test_recovery_from_nan():
    agent, aug = make(seed=5)
    rb, L = ring(aug), NullLogger()
    for step in (1, 2):
        agent.update(rb, L, step)
    lay = agent._lay
    q0, q1 = lay["q"]
    trunk0 = (agent.actor.trunk[0].weight.data_ptr() - agent._actor_flat.data_ptr()) // 4
    with torch.no_grad():
        agent._critic_flat[q0:q1].fill_(NAN)
        agent._target_flat[q0:q1].fill_(NAN)
        agent._actor_flat[trunk0:].fill_(NAN)
        for opt in (agent.critic_optimizer, agent.actor_optimizer):
            opt._m.fill_(NAN)
            opt._v.fill_(NAN)
        agent._critic_gflat.fill_(NAN)
        agent._actor_gbucket.fill_(NAN)
    agent.reset_networks()
    L = NullLogger()
    for step in (3, 4):
        agent.update(rb, L, step)
    st = _state(agent)
    assert all(np.isfinite(v) for v in L.scalars.values()) and len(L.scalars) >= 6, L.scalars
    for k in ("critic", "target", "actor", "log_alpha", "critic_m", "critic_v", "actor_m", "actor_v"):
        assert bool(torch.isfinite(st[k]).all()), k


# ------------------------------------------------------------------------------------------- 3. graphs, DP, checkpoints
@pytest.mark.parametrize("G", [1, 3])
def test_update_graphs_survive_a_scheduled_reset(G):
    steps = list(range(1, 15))
    hp = dict(reset_interval=10, reset_encoder_keep=0.8, reset_seed=2, log_interval=10 ** 9, utd_ratio=G,
              critic_target_update_freq=2)

    def run(graphs):
        agent, aug = make(seed=6, **hp)
        rb = ring(aug)
        _seed(12)
        if graphs:
            agent.enable_update_graphs(rb, warm=1, depth=2)
        L, seen = NullLogger(), {}
        for step in steps:
            if graphs and step == 10:
                torch.cuda.synchronize()
                seen = dict(graphs=agent._graphs, key=agent._graph_key(), at=agent._graph_key_at_capture,
                            ids=[id(st["graph"]) for r in agent._graphs.values() for st in r])
                assert seen["ids"] and all(st["graph"] is not None for r in agent._graphs.values() for st in r)
                assert len(agent._graphs) == (4 if G > 1 else 2)
            agent.update(rb, L, step)
        if graphs:
            assert agent._graphs is seen["graphs"] and agent._graph_key() == seen["key"]
            assert agent._graph_key_at_capture == seen["at"]
            assert [id(st["graph"]) for r in agent._graphs.values() for st in r] == seen["ids"]  # nothing captured again
        assert agent.reset_count == 1 and agent._reset_epoch == 1
        return _state(agent, rb)
    eager, graphed = run(False), run(True)
    _assert_same(eager, graphed)
    assert int(eager["critic_steps"][0]) == 5 * G and bool(torch.isfinite(eager["critic"]).all())


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


def test_one_rank_data_parallel(nccl_world1):
    def run(dp):
        agent, aug = make(seed=7, reset_interval=3, reset_encoder_keep=0.5)
        rb = ring(aug)
        _seed(13)
        if dp:
            agent.enable_data_parallel(single_rank_collectives=True, overlap=False, check_every=1)
        L = NullLogger()
        for step in (1, 2, 3, 4):
            agent.update(rb, L, step)
        if dp:
            agent.check_replicas()
        assert agent.reset_count == 1
        return _state(agent, rb), dict(L.scalars)
    plain, dp = run(False), run(True)
    _assert_same(plain[0], dp[0])
    assert plain[1] == dp[1]


def test_checkpoint_across_a_reset_boundary(tmp_path):
    hp = dict(reset_interval=10, reset_encoder_keep=0.8, reset_seed=4)
    agent, aug = make(seed=8, **hp)
    rb, L = ring(aug), NullLogger()
    _seed(14)
    for step in range(6, 10):
        agent.update(rb, L, step)
    ck = str(tmp_path / "reset.pt")
    agent.save_checkpoint(ck, 9)
    for step in (10, 11, 12):
        agent.update(rb, L, step)
    assert agent.reset_count == 1
    want = _state(agent, rb), dict(L.scalars)

    other, aug2 = make(seed=99, **{**hp, "reset_seed": 1234})  # another process state: the stream comes from the file
    rb2, L2 = ring(aug2), NullLogger()
    _seed(99)
    assert other.load_checkpoint(ck) == 9 and other.reset_count == 0 and other._reset_epoch == 0
    for step in (10, 11, 12):
        other.update(rb2, L2, step)
    assert other.reset_count == 1
    got = _state(other, rb2), dict(L2.scalars)
    _assert_same(got[0], want[0])
    assert got[1] == want[1]
