"""Acting on a batch of observations on the MI355X: ``ops.stage_frames`` (curla_stage_frames_u8: N planar uint8 frames
into N NHWC ring slots, centre window fused) bit for bit against NumPy, and ``CurlSacAgent.select_actions`` /
``sample_actions`` against the reference's recorded outputs, the oracle's actor forward, the single-frame calls, each
other over the input routes -- all at the project's parity bar (tests/_util.RTOL, norm-relative) -- and against an
agent that never acts (training must not notice)."""
import numpy as np
import pytest
import torch

from tests._util import RTOL, load, rel_err, sub

pytestmark = pytest.mark.gpu


def check(name, got, ref, tol=RTOL):
    """Every figure goes to the test's output (``pytest -s`` shows it) before it is asserted."""
    e = rel_err(got, ref)
    print(f"{name}: rel err {e:.3e}")
    assert np.isfinite(e) and e <= tol, f"{name}: rel err {e:.3e} > {tol:.1e}"
    return e


HP = dict(discount=0.99, init_temperature=0.1, alpha_lr=1e-4, alpha_beta=0.5, actor_lr=1e-3, actor_beta=0.9,
          actor_log_std_min=-10, actor_log_std_max=2, actor_update_freq=2, critic_lr=1e-3, critic_beta=0.9,
          critic_tau=0.01, critic_target_update_freq=2, encoder_feature_dim=50, encoder_lr=1e-3, encoder_tau=0.05,
          num_layers=4, num_filters=32, log_interval=1)
DEV = "cuda"


def _t(x):
    return torch.as_tensor(np.asarray(x)).cuda()


def _u8(shape, seed):
    return np.random.RandomState(seed).randint(0, 256, shape, dtype=np.uint8)


# ---------------------------------------------------------------------------------------------- the staging kernel
def _guarded_ring(slots, Hd, Wd, C):
    """A ring of ``slots`` slots plus the loader's 32 bytes of slack, filled with a pattern."""
    n = slots * Hd * Wd * C + 32
    flat = torch.from_numpy(((np.arange(n) * 7 + 3) % 251).astype(np.uint8)).cuda()
    return flat, flat[:n - 32].view(slots, Hd, Wd, C)


def _stage_and_compare(ops, src, N, C, Hs, Ws, top, left, Hd, Wd, first_slot, src_dev=None):
    flat, ring = _guarded_ring(first_slot + N + 2, Hd, Wd, C)
    before = flat.cpu().numpy().copy()
    ops.stage_frames(_t(src) if src_dev is None else src_dev, ring, first_slot, top, left)
    torch.cuda.synchronize()
    after = flat.cpu().numpy()
    want = np.ascontiguousarray(src[:, :, top:top + Hd, left:left + Wd].transpose(0, 2, 3, 1))
    slot = Hd * Wd * C
    lo, hi = first_slot * slot, (first_slot + N) * slot
    tag = f"C{C} N{N} {Hs}x{Ws}->{Hd}x{Wd}@({top},{left}) slot {first_slot}"
    assert np.array_equal(after[lo:hi].reshape(want.shape), want), tag
    assert np.array_equal(after[:lo], before[:lo]) and np.array_equal(after[hi:], before[hi:]), tag + ": guard bytes moved"


STAGE_CASES = [  # Hs, Ws, top, left, Hd, Wd, first_slot
    (34, 40, 3, 3, 28, 34, 0), (84, 84, 4, 4, 76, 76, 2), (90, 160, 7, 12, 76, 135, 1),  # the centre windows
    (35, 43, 1, 3, 29, 33, 0), (35, 43, 3, 7, 29, 33, 1), (35, 43, 5, 9, 29, 33, 2),      # odd sizes, odd origins
    (28, 34, 0, 0, 28, 34, 3), (31, 45, 0, 0, 31, 45, 1),                                 # whole-frame windows
]


@pytest.mark.parametrize("N", [1, 3, 17])
@pytest.mark.parametrize("C", [3, 6, 9, 12])
def test_stage_frames_bit_exact(C, N):
    from curla_amd import ops
    for i, (Hs, Ws, top, left, Hd, Wd, first_slot) in enumerate(STAGE_CASES):
        if (Hs, Ws, Hd, Wd) in ((34, 40, 28, 34), (84, 84, 76, 76), (90, 160, 76, 135)):
            assert (top, left) == ((Hs - Hd) // 2, (Ws - Wd) // 2)
        src = _u8((N, C, Hs, Ws), 100 * C + N + i)
        _stage_and_compare(ops, src, N, C, Hs, Ws, top, left, Hd, Wd, first_slot)


@pytest.mark.parametrize("C,N,misalign", [(9, 3, 1), (3, 5, 3), (12, 2, 2), (4, 3, 0), (5, 2, 0), (1, 4, 0), (7, 3, 1)])
def test_stage_frames_bytewise_path_gives_the_same_bytes(C, N, misalign):
    """Other channel counts, and sources off a dword boundary, take the byte-by-byte kernel: same contract."""
    from curla_amd import ops
    Hs, Ws, top, left, Hd, Wd = 35, 43, 3, 5, 29, 33
    src = _u8((N, C, Hs, Ws), 7 * C + N)
    holder = torch.zeros(src.size + 8, dtype=torch.uint8, device=DEV)
    view = holder[misalign:misalign + src.size].view(N, C, Hs, Ws)
    view.copy_(_t(src))
    assert view.data_ptr() % 4 == misalign % 4
    _stage_and_compare(ops, src, N, C, Hs, Ws, top, left, Hd, Wd, 1, src_dev=view)


def test_stage_frames_refuses_windows_outside_the_source():
    from curla_amd import _lib, ops
    N, C, Hs, Ws, Hd, Wd = 3, 9, 34, 40, 28, 34
    src = _t(_u8((N, C, Hs, Ws), 1))
    flat, ring = _guarded_ring(N + 2, Hd, Wd, C)
    before = flat.cpu().numpy().copy()
    for top, left, first in ((7, 3, 0), (3, 7, 0), (-1, 3, 0), (3, -1, 0), (3, 3, -1), (3, 3, 3), (3, 3, N + 2)):
        with pytest.raises(_lib.CurlaHipError):
            ops.stage_frames(src, ring, first, top, left)
    with pytest.raises(_lib.CurlaHipError):
        ops.stage_frames(src[:, :6], ring, 0, 3, 3)  # (channel count of the ring, and a non-contiguous source)
    torch.cuda.synchronize()
    assert np.array_equal(flat.cpu().numpy(), before)


# ---------------------------------------------------------------------------------------------- the agent's calls
def make_agent(obs_shape, in_hw, hidden, **kw):
    import curla_amd
    aug = curla_amd.RandomCrop(in_hw, obs_shape[1:]) if in_hw is not None else curla_amd.IdentityAugmentation(obs_shape[1:])
    torch.manual_seed(0)
    return curla_amd.CurlSacAgent(obs_shape, (2,), torch.device(DEV), aug, hidden_dim=hidden, **{**HP, **kw}), aug


@pytest.fixture(scope="module")
def tiny():
    return load("tiny.npz")


def _tiny_agent(g):
    agent, aug = make_agent((9, 28, 34), (34, 40), 64)
    critic = sub(g, "state0/critic/")
    agent.critic.load_state_dict(critic)
    agent.actor.load_state_dict({**{k: v for k, v in critic.items() if ".convs." in k}, **sub(g, "state0/actor/")})
    agent.critic_target.load_state_dict(sub(g, "state0/critic_target/"))
    return agent, aug


def _tiny_batch(g, N=5):
    batch = np.concatenate([g["act/obs"][None], _u8((N - 1, 9, 34, 40), 3)])
    noise = np.concatenate([g["act/noise"], np.random.RandomState(4).randn(N - 1, 2).astype(np.float32)])
    return batch, torch.from_numpy(noise)


def _centre(batch, out_hw):
    h, w = out_hw
    top, left = (batch.shape[2] - h) // 2, (batch.shape[3] - w) // 2
    return batch[:, :, top:top + h, left:left + w]


def _oracle(agent, cropped_u8, noise, layers=4):
    from oracle import curla_oracle as O
    actor = {k: v.detach().cpu() for k, v in agent.actor.state_dict().items()}
    critic = {k: v.detach().cpu() for k, v in agent.critic.state_dict().items()}
    x = torch.from_numpy(np.ascontiguousarray(cropped_u8)).float()
    mu, pi, _, _ = O.actor_forward(actor, critic, x, noise, num_layers=layers, log_std_min=-10, log_std_max=2,
                                   compute_log_pi=False)
    return mu, pi


def test_actions_vs_reference_and_oracle(tiny):
    g = tiny
    agent, aug = _tiny_agent(g)
    batch, noise = _tiny_batch(g)
    mu = agent.select_actions(batch)
    pi = agent.sample_actions(batch, noise=noise.cuda())
    assert mu.shape == (5, 2) and pi.shape == (5, 2) and mu.dtype == np.float32 and pi.dtype == np.float32
    check("select_actions row 0 vs the reference's recorded output", mu[0], g["act/select"])
    check("sample_actions row 0 vs the reference's recorded output", pi[0], g["act/sample"])
    mu_o, pi_o = _oracle(agent, _centre(batch, (28, 34)), noise)
    check("select_actions vs oracle.actor_forward", mu, mu_o)
    check("sample_actions vs oracle.actor_forward", pi, pi_o)
    for i in range(5):
        check(f"select_actions row {i} vs oracle", mu[i], mu_o[i])
        check(f"sample_actions row {i} vs oracle", pi[i], pi_o[i])


def test_rows_agree_with_the_single_frame_calls(tiny):
    agent, aug = _tiny_agent(tiny)
    batch, noise = _tiny_batch(tiny)
    noise = noise.cuda()
    mu, pi = agent.select_actions(batch), agent.sample_actions(batch, noise=noise)
    worst = 0.0
    for i in range(len(batch)):
        worst = max(worst, check(f"row {i} vs sample_action", pi[i], agent.sample_action(batch[i], noise=noise[i:i + 1])))
        worst = max(worst, check(f"row {i} vs select_action", mu[i],
                                 agent.select_action(aug.evaluation_augmentation(batch[i]))))
    print(f"largest error between a batched row and the single-frame call: {worst:.3e}")
    # pre-cropped frames: the same staged bytes, the same launches
    cropped = np.ascontiguousarray(_centre(batch, (28, 34)))
    assert np.array_equal(agent.select_actions(cropped), mu)
    assert np.array_equal(agent.sample_actions(cropped, noise=noise), pi)


def test_input_routes_agree(tiny):
    agent, _ = _tiny_agent(tiny)
    batch, noise = _tiny_batch(tiny)
    noise = noise.cuda()
    for name, call in (("select", lambda o, **k: agent.select_actions(o, **k)),
                       ("sample", lambda o, **k: agent.sample_actions(o, noise=noise, **k))):
        a = call(batch)
        assert np.array_equal(call(list(batch)), a), name + ": list of frames"
        assert np.array_equal(call(tuple(batch[i] for i in range(len(batch)))), a), name + ": tuple of frames"
        assert np.array_equal(call(_t(batch)), a), name + ": CUDA uint8 tensor"
        assert np.array_equal(call(torch.from_numpy(batch)), a), name + ": CPU uint8 tensor"
        check(name + ": float32 array route", call(batch.astype(np.float32)), a)
        check(name + ": float32 CUDA tensor route", call(_t(batch).float()), a)
        # as_tensor: a CUDA tensor equal to the NumPy result, and still so after another acting call has run
        t = call(batch, as_tensor=True)
        assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == a.shape and not t.requires_grad
        other = call(_u8(batch.shape, 11), as_tensor=True)
        agent.select_actions(_u8((7,) + batch.shape[1:], 12))  # (another N: the staging blocks grow)
        torch.cuda.synchronize()
        assert np.array_equal(t.cpu().numpy(), a), name + ": as_tensor result changed under later calls"
        assert not np.array_equal(other.cpu().numpy(), a)


def test_noise_contract(tiny):
    agent, _ = _tiny_agent(tiny)
    batch, _ = _tiny_batch(tiny)
    torch.manual_seed(7)
    a = agent.sample_actions(batch)
    torch.manual_seed(7)
    nz = torch.randn((5, 2), device=DEV)
    assert np.array_equal(agent.sample_actions(batch, noise=nz), a)
    torch.manual_seed(8)
    assert not np.array_equal(agent.sample_actions(batch), a)
    # select_actions draws nothing
    state = torch.cuda.get_rng_state(torch.device(DEV))
    agent.select_actions(batch)
    assert torch.equal(torch.cuda.get_rng_state(torch.device(DEV)), state)


def test_grad_mode_builds_no_graph(tiny):
    agent, _ = _tiny_agent(tiny)
    batch, noise = _tiny_batch(tiny)
    with torch.enable_grad():
        t = agent.sample_actions(batch, noise=noise.cuda(), as_tensor=True)
        m = agent.select_actions(batch, as_tensor=True)
    assert not t.requires_grad and t.grad_fn is None and not m.requires_grad and m.grad_fn is None
    with torch.no_grad():
        assert np.array_equal(agent.select_actions(batch), m.cpu().numpy())


GEOMETRIES = [  # name, obs_shape, pre-crop size (None: identity), hidden, agent keywords
    ("84_to_76_hidden_1024", (9, 76, 76), (84, 84), 1024, {}),
    ("90x160_to_76x135", (9, 76, 135), (90, 160), 64, {}),
    ("12x64x64_identity_6_layers", (12, 64, 64), None, 64, dict(num_layers=6)),
    ("filters_16_generic_path", (9, 32, 36), (40, 44), 64, dict(num_filters=16)),
    ("3_channels_odd_sizes", (3, 31, 45), (37, 51), 64, dict(num_layers=3)),
    ("6_channels", (6, 33, 29), (39, 35), 64, dict(num_layers=2)),
]


@pytest.mark.parametrize("N", [3, 17])
@pytest.mark.parametrize("name,obs_shape,in_hw,hidden,kw", GEOMETRIES, ids=[g[0] for g in GEOMETRIES])
def test_geometries_vs_oracle(name, obs_shape, in_hw, hidden, kw, N):
    agent, _ = make_agent(obs_shape, in_hw, hidden, **kw)
    src_hw = in_hw if in_hw is not None else obs_shape[1:]
    batch = _u8((N, obs_shape[0]) + tuple(src_hw), 20 + N)
    noise = torch.from_numpy(np.random.RandomState(21).randn(N, 2).astype(np.float32))
    mu = agent.select_actions(batch)
    pi = agent.sample_actions(batch, noise=noise.cuda())
    mu_o, pi_o = _oracle(agent, _centre(batch, obs_shape[1:]), noise, layers=kw.get("num_layers", 4))
    check(f"{name} N={N} select_actions vs oracle", mu, mu_o)
    check(f"{name} N={N} sample_actions vs oracle", pi, pi_o)


# ---------------------------------------------------------------------------------------------- beside training
class NullLogger:
    def log(self, *a, **k):
        pass


def _train(acting, graphs, steps):
    import curla_amd
    torch.manual_seed(5)
    np.random.seed(5)
    dev = torch.device(DEV)
    B, C, in_hw, out_hw = 256, 9, (40, 44), (32, 36)
    aug = curla_amd.RandomCrop(in_hw, out_hw)
    agent = curla_amd.CurlSacAgent((C,) + out_hw, (2,), dev, aug, hidden_dim=64, **{**HP, "log_interval": 5})
    rb = curla_amd.ReplayBuffer((C,) + in_hw, (2,), 512, B, dev, aug)
    rs = np.random.RandomState(6)
    n = 400
    rb.add_batch(rs.randint(0, 256, (n, C) + in_hw, dtype=np.uint8), rs.uniform(-1, 1, (n, 2)).astype(np.float32),
                 rs.randn(n).astype(np.float32), rs.randint(0, 256, (n, C) + in_hw, dtype=np.uint8),
                 (np.arange(n) % 7) == 6)
    if graphs:
        agent.enable_update_graphs(rb)
    L = NullLogger()
    acted = []
    for step in range(steps):
        if acting:
            acted.append(agent.select_actions(_u8((8, C) + in_hw, 50 + step)))
        agent.update(rb, L, step)
    torch.cuda.synchronize()
    state = {"critic": agent._critic_flat, "target": agent._target_flat, "actor": agent._actor_flat,
             "log_alpha": agent.log_alpha.detach(), "rng": torch.cuda.get_rng_state(dev)}
    for name, opt in (("critic", agent.critic_optimizer), ("actor", agent.actor_optimizer),
                      ("encoder", agent.encoder_optimizer), ("cpc", agent.cpc_optimizer)):
        state[name + "_m"], state[name + "_v"] = opt._m, opt._v
        state[name + "_steps"] = torch.tensor(opt._steps)
    la = agent.log_alpha_optimizer.state[agent.log_alpha]
    state["la_m"], state["la_v"], state["la_step"] = la["exp_avg"], la["exp_avg_sq"], torch.as_tensor(la["step"])
    return {k: v.detach().cpu().clone() for k, v in state.items()}, acted, agent


@pytest.mark.parametrize("graphs,steps", [(False, 4), (True, 4), (True, 12)],
                         ids=["eager", "update graphs enabled", "update graphs replaying"])
def test_acting_does_not_disturb_training(graphs, steps):
    """Two agents from the same seed on the same ring contents; one calls select_actions (N = 8) before every update.
    Parameters, targets, log_alpha, Adam state and the generator must end bit-identical.  (With update graphs
    enabled the first replay comes at the ninth update: the 12-step case puts acting calls between replays too.)"""
    plain, _, _ = _train(False, graphs, steps)
    acted, actions, agent = _train(True, graphs, steps)
    for k in plain:
        assert torch.equal(plain[k], acted[k]), k
    assert all(a.shape == (8, 2) and np.isfinite(a).all() for a in actions)
    if graphs and steps >= 12:
        assert sum(len(r) for r in agent._graphs.values()) == 4  # the graphs were captured and are in use


def test_back_to_back_calls_without_a_sync(tiny):
    """More calls in a row than there are pinned blocks, different frames each, nothing waited for in between: every
    result must be the one a call on its own gives (a block is rewritten only after its copy has executed)."""
    agent, _ = _tiny_agent(tiny)
    batches = [_u8((6, 9, 34, 40), 30 + i) for i in range(5)]
    noise = torch.from_numpy(np.random.RandomState(31).randn(6, 2).astype(np.float32)).cuda()
    alone = [agent.sample_actions(b, noise=noise) for b in batches]
    torch.cuda.synchronize()
    outs = [agent.sample_actions(b, noise=noise, as_tensor=True) for b in batches]
    torch.cuda.synchronize()
    for i, (o, a) in enumerate(zip(outs, alone)):
        assert np.array_equal(o.cpu().numpy(), a), i
    assert len({a.tobytes() for a in alone}) == len(alone)
    # the staging blocks were made once (for the largest N seen) and reused by every call since
    st = agent._act_batch_stage[(9, 34, 40)]
    ptrs = (st["ring"].data_ptr(), st["src"].data_ptr(), [p[0].data_ptr() for p in st["pins"]])
    agent.sample_actions(batches[0][:4], noise=noise[:4])
    st = agent._act_batch_stage[(9, 34, 40)]
    assert ptrs == (st["ring"].data_ptr(), st["src"].data_ptr(), [p[0].data_ptr() for p in st["pins"]])
