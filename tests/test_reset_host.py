"""CurlSacAgent.reset_networks() and the reset schedule on the host, under the launch-trace hook: nothing
is computed on a device.  The three keywords and their validation; that ``reset_interval=0`` is the agent without the
keyword; the epochs of the schedule; that a reset leaves torch's and NumPy's global streams alone and draws from a stream
a checkpoint carries; the staging buffers against a flat image built here from the documented layout; the C entry point
(declared, bound, exported, argument checks); checkpoints from before the keywords."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import curla_amd
from curla_amd import _lib
from curla_amd.networks import Actor, Critic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, IN_HW, OUT_HW, B, CAP = 9, (34, 40), (28, 34), 8, 32
NET = dict(hidden_dim=64, num_layers=2, num_filters=8)
NEW_KEYS = {"reset_rng", "reset_epoch", "reset_count", "reset_interval", "reset_encoder_keep", "reset_seed"}
# what save_checkpoint wrote before the keywords
OLD_KEYS = {"format", "step", "actor", "critic", "critic_target", "curl", "log_alpha", "optimizers", "rng", "critic_dropout",
            "utd_ratio", "critic_quantiles", "critic_drop_quantiles"}


def make(seed=1, **kw):
    aug = curla_amd.RandomCrop(IN_HW, OUT_HW)
    curla_amd.set_seed_everywhere(seed)
    agent = curla_amd.CurlSacAgent((C,) + OUT_HW, (2,), "cpu", aug, **{**NET, **dict(log_interval=1000), **kw})
    rb = curla_amd.ReplayBuffer((C,) + IN_HW, (2,), CAP, B, "cpu", aug)
    rs = np.random.RandomState(3)
    for _ in range(12):
        f = rs.randint(0, 256, (C,) + IN_HW, dtype=np.uint8)
        rb.add(f, [0.1, -0.2], 0.5, f, False)
    curla_amd.set_seed_everywhere(seed + 10)
    return agent, rb


class Log:
    def log(self, *a, **k):
        pass


def _shape(args):
    """A traced call's arguments with the addresses reduced to given / NULL (two agents' buffers differ)."""
    return tuple(a if a is None or isinstance(a, float) or abs(a) < 2 ** 20 else "ptr" for a in args)


def traced(fn):
    calls = []
    _lib.set_trace_hook(lambda name, args: calls.append((name, _shape(args))))
    try:
        fn()
    finally:
        _lib.set_trace_hook(None)
    return calls


def _resets(calls):
    return [n for n, _ in calls].count("curla_shrink_perturb2")


def _staged(agent):
    return {k: v["host"].numpy().tobytes() for k, v in agent._reset_stage.items()}


# ------------------------------------------------------------------------------------------------ keywords, validation
def test_keyword_positions_and_defaults():
    init = list(inspect.signature(curla_amd.CurlSacAgent.__init__).parameters)
    assert init[-1] == "pixel_sac" and not {"reset_interval", "reset_encoder_keep", "reset_seed"} & set(init)
    call = inspect.signature(curla_amd.CurlSacAgent).parameters
    names = list(call)
    for k, default in (("reset_interval", 0), ("reset_encoder_keep", 1.0), ("reset_seed", 0)):
        assert call[k].default == default and type(call[k].default) is type(default)
        assert call[k].kind is inspect.Parameter.KEYWORD_ONLY
        assert names.index(k) < names.index("critic_quantiles")
    assert names[-2] == "critic_layer_norm" and names[-3] == "critic_dropout"
    off, _ = make()
    assert (off.reset_interval, off.reset_encoder_keep, off.reset_seed, off.reset_count) == (0, 1.0, 0, 0)
    on, _ = make(reset_interval=np.int64(10), reset_encoder_keep=0.5, reset_seed=7)
    assert (on.reset_interval, on.reset_encoder_keep, on.reset_seed) == (10, 0.5, 7) and type(on.reset_interval) is int


@pytest.mark.parametrize("kw", [dict(reset_interval=-1), dict(reset_interval=True), dict(reset_interval=2.0),
                                dict(reset_interval="10"), dict(reset_interval=None),
                                dict(reset_encoder_keep=-0.1), dict(reset_encoder_keep=1.5), dict(reset_encoder_keep=True),
                                dict(reset_encoder_keep=float("nan")), dict(reset_encoder_keep="0.5"),
                                dict(reset_encoder_keep=None),
                                dict(reset_seed=1.0), dict(reset_seed=False), dict(reset_seed="0"), dict(reset_seed=None)])
def test_rejected_values(kw):
    with pytest.raises(ValueError):
        curla_amd.CurlSacAgent((C,) + OUT_HW, (2,), "cpu", None, **NET, **kw)


def test_edited_attributes_are_checked_again():
    agent, rb = make(reset_interval=10)
    agent.reset_interval = 2.5
    with pytest.raises(ValueError):
        traced(lambda: agent.update(rb, Log(), 1))
    agent.reset_interval = 10
    agent.reset_encoder_keep = 2.0
    with pytest.raises(ValueError):
        traced(lambda: agent.reset_networks())
    with pytest.raises(ValueError):
        traced(lambda: agent.reset_networks(encoder_keep=float("nan")))
    assert agent.reset_count == 0


def test_a_cpu_agent_without_the_trace_hook_refuses():
    agent, _ = make()
    with pytest.raises(RuntimeError):
        agent.reset_networks()


@pytest.mark.parametrize("step", [1, 2])
def test_interval_zero_is_the_agent_without_the_keyword(step, tmp_path):
    plain, rb_p = make()
    zero, rb_z = make(reset_interval=0, reset_encoder_keep=1.0, reset_seed=0)
    a = traced(lambda: plain.update(rb_p, Log(), step))
    b = traced(lambda: zero.update(rb_z, Log(), step))
    assert a == b and _resets(a) == 0 and len(a) > 10
    assert zero._graph_key() == plain._graph_key() and zero._reset_stage is None
    assert list(zero.critic.state_dict()) == list(plain.critic.state_dict())
    keys = []
    for agent, name in ((plain, "p.pt"), (zero, "z.pt")):
        agent.save_checkpoint(str(tmp_path / name), step)
        keys.append(set(torch.load(str(tmp_path / name), weights_only=False)))
    assert keys[0] == keys[1] and keys[0] - NEW_KEYS == OLD_KEYS and NEW_KEYS <= keys[0]


# -------------------------------------------------------------------------------------------------------------- epochs
def test_epochs_of_the_schedule():
    agent, rb = make(reset_interval=10)
    for step in range(1, 10):
        assert _resets(traced(lambda: agent.update(rb, Log(), step))) == 0
    assert agent.reset_count == 0
    calls = traced(lambda: agent.update(rb, Log(), 10))
    names = [n for n, _ in calls]
    assert _resets(calls) == 3 and names[:3] == ["curla_shrink_perturb2"] * 3  # the reset's launches, then the update's
    assert (agent.reset_count, agent._reset_epoch) == (1, 1)
    assert _resets(traced(lambda: agent.update(rb, Log(), 10))) == 0    # the epoch has had its reset
    assert _resets(traced(lambda: agent.update(rb, Log(), 19))) == 0
    assert _resets(traced(lambda: agent.update(rb, Log(), 35))) == 3    # steps 20 .. 34 skipped: ONE reset
    assert (agent.reset_count, agent._reset_epoch) == (2, 3)
    assert _resets(traced(lambda: agent.update(rb, Log(), 36))) == 0


def test_the_launches_of_a_reset():
    """[W] alone (the target has no W), [encoder | Q1 | Q2] with the target, [fc, ln | trunk]: keep for the encoder
    side, 0 for the heads, 1 - keep formed in double."""
    agent, _ = make(reset_encoder_keep=0.8)
    calls = traced(lambda: agent.reset_networks())
    assert [n for n, _ in calls] == ["curla_shrink_perturb2"] * 3
    lay = agent._lay
    (w0, w1), (e0, e1), (q0, q1) = lay["w"], lay["enc"], lay["q"]
    new = 1.0 - 0.8
    assert calls[0][1] == ("ptr", None, "ptr", w1 - w0, w1 - w0, 0.8, new, 0.8, new, 0)
    assert calls[1][1] == ("ptr", "ptr", "ptr", q1 - e0, e1 - e0, 0.8, new, 0.0, 1.0, 0)
    n_act = agent._actor_flat.numel()
    trunk = sum((p.numel() + 3) & ~3 for n, p in agent.actor.named_parameters() if ".convs." not in n and "trunk" not in n)
    assert calls[2][1] == ("ptr", None, "ptr", n_act, trunk, 0.8, new, 0.0, 1.0, 0)
    heads_only = traced(lambda: agent.reset_networks(encoder_keep=1.0))
    assert [c[1][5:9] for c in heads_only] == [(1.0, 0.0, 1.0, 0.0), (1.0, 0.0, 0.0, 1.0), (1.0, 0.0, 0.0, 1.0)]


def test_under_a_utd_ratio_the_reset_precedes_the_first_minibatch():
    agent, rb = make(reset_interval=10, utd_ratio=3, critic_target_update_freq=1)
    names = [n for n, _ in traced(lambda: agent.update(rb, Log(), 10))]
    first_other = next(i for i, n in enumerate(names) if n != "curla_shrink_perturb2")
    assert first_other == 3 and names.count("curla_shrink_perturb2") == 3
    staging = [i for i, n in enumerate(names) if n in ("curla_sample_stage", "curla_gather_transition_scalars")]
    assert len(staging) == 3 and min(staging) >= 3  # three minibatches, all behind the reset
    assert agent.reset_count == 1


def test_state_after_a_reset():
    """The host side of a reset on a CPU agent (torch's own Adams): moments zero, step counts 0, log_alpha back,
    caches cleared, no tensor replaced."""
    agent, rb = make(init_temperature=0.1)
    ptrs = [p.data_ptr() for p in (*agent.critic.parameters(), *agent.critic_target.parameters(),
                                   *agent.actor.parameters(), agent.CURL.W, agent.log_alpha)]
    with torch.no_grad():
        agent.log_alpha.fill_(0.3)
    for opt in agent._optimizers().values():
        for g in opt.param_groups:
            for p in g["params"]:
                opt.state[p] = {"step": torch.tensor(4.0), "exp_avg": torch.full_like(p, float("nan")),
                                "exp_avg_sq": torch.ones_like(p)}
    agent._critic_gflat.fill_(float("nan"))
    agent._anchor_cache = agent._pos_cache = object()
    agent._pos_fc_done = True
    moments = [st[k] for opt in agent._optimizers().values() for st in opt.state.values() for k in ("exp_avg", "exp_avg_sq")]
    traced(lambda: agent.reset_networks(alpha=False))
    assert agent.log_alpha.item() == 0.3
    la =agent.log_alpha_optimizer.state[agent.log_alpha]
    assert float(la["step"]) == 4.0 and bool(la["exp_avg"].isnan())
    traced(lambda: agent.reset_networks())
    assert agent.log_alpha.item() == float(np.log(0.1))
    for opt in agent._optimizers().values():
        for st in opt.state.values():
            assert float(st["step"]) == 0.0 and not st["exp_avg"].any() and not st["exp_avg_sq"].any()
    assert all(a is b for a, b in zip(moments, [st[k] for opt in agent._optimizers().values() for st in opt.state.values()
                                                for k in ("exp_avg", "exp_avg_sq")]))
    assert not agent._critic_gflat.any() and not agent._actor_gbucket.any() and float(agent.log_alpha.grad) == 0.0
    assert agent._anchor_cache is None and agent._pos_cache is None and agent._pos_fc_done is False
    assert ptrs == [p.data_ptr() for p in (*agent.critic.parameters(), *agent.critic_target.parameters(),
                                           *agent.actor.parameters(), agent.CURL.W, agent.log_alpha)]
    assert agent.reset_count == 2


def test_flat_adam_reset_state():
    from curla_amd.optim import FlatAdam
    flat, gflat = torch.zeros(24), torch.zeros(24)
    ps = [torch.nn.Parameter(flat[0:8]), torch.nn.Parameter(flat[8:20].view(3, 4))]
    ps[0].grad, ps[1].grad = gflat[0:8], gflat[8:20].view(3, 4)
    opt = FlatAdam(ps, flat, gflat, lr=1e-3)
    traced(lambda: (opt.step(), opt.step()))
    opt._m.fill_(float("nan"))
    opt._v.fill_(2.0)
    m_ptr, v_ptr, plans = opt._m.data_ptr(), opt._v.data_ptr(), dict(opt._plans)
    assert opt._steps == [2, 2] and plans
    opt.reset_state()
    assert opt._steps == [0, 0] and not opt._m.any() and not opt._v.any()
    assert (opt._m.data_ptr(), opt._v.data_ptr()) == (m_ptr, v_ptr) and opt._plans == plans
    sd = opt.state_dict()["state"]
    assert all(float(st["step"]) == 0.0 and not st["exp_avg"].any() for st in sd.values()) and len(sd) == 2
    assert opt.state[ps[0]]["exp_avg"].data_ptr() == m_ptr
    calls = traced(opt.step)
    assert opt._steps == [1, 1] and calls[0][1][9] == 1  # the next launch is step 1 again


# ------------------------------------------------------------------------------------------------------- RNG isolation
def _global_streams():
    s = np.random.get_state()
    return torch.get_rng_state().clone(), (s[1].copy(), s[2], s[3], s[4])


def _same_streams(a, b):
    return torch.equal(a[0], b[0]) and np.array_equal(a[1][0], b[1][0]) and a[1][1:] == b[1][1:]


@pytest.mark.parametrize("kw", [{}, dict(critic_layer_norm=True, critic_quantiles=5)])
def test_a_reset_leaves_the_global_streams_alone(kw):
    agent, _ = make(**kw)
    before = _global_streams()
    traced(lambda: agent.reset_networks())
    traced(lambda: agent.reset_networks(encoder_keep=0.5))
    assert _same_streams(before, _global_streams())


def test_the_reset_stream_is_the_agents_own():
    a, _ = make(seed=1, reset_seed=5)
    b, _ = make(seed=2, reset_seed=5)    # another global seed: other parameters, the same fresh values
    c, _ = make(seed=1, reset_seed=6)
    assert not torch.equal(a._critic_flat, b._critic_flat)
    for agent in (a, b, c):
        traced(lambda: agent.reset_networks())
    first = _staged(a)
    assert first == _staged(b) and first["critic"] != _staged(c)["critic"] and first["actor"] != _staged(c)["actor"]
    traced(lambda: a.reset_networks())
    second = _staged(a)
    assert second["critic"] != first["critic"] and second["actor"] != first["actor"]  # the stream has moved on
    traced(lambda: b.reset_networks())
    assert _staged(b) == second


def test_a_checkpoint_carries_the_stream(tmp_path):
    a, _ = make(seed=1, reset_seed=5, reset_interval=10)
    traced(lambda: a.reset_networks())
    a._reset_epoch = 4
    a.save_checkpoint(str(tmp_path / "ck.pt"), 47)
    ck = torch.load(str(tmp_path / "ck.pt"), weights_only=False)
    assert ck["reset_count"] == 1 and ck["reset_epoch"] == 4 and ck["reset_interval"] == 10
    assert ck["reset_encoder_keep"] == 1.0 and ck["reset_seed"] == 5
    traced(lambda: a.reset_networks())
    want = _staged(a)
    b, rb = make(seed=3, reset_seed=99, reset_interval=10)
    assert b.load_checkpoint(str(tmp_path / "ck.pt")) == 47
    assert (b.reset_count, b._reset_epoch, b.reset_seed) == (1, 4, 99)  # the settings stay the agent's own
    traced(lambda: b.reset_networks())
    assert _staged(b) == want
    assert _resets(traced(lambda: b.update(rb, Log(), 49))) == 0 and _resets(traced(lambda: b.update(rb, Log(), 50))) == 3


def test_checkpoints_from_before_the_keywords(tmp_path):
    a, _ = make()
    a.save_checkpoint(str(tmp_path / "new.pt"), 50)
    ck = torch.load(str(tmp_path / "new.pt"), weights_only=False)
    for k in NEW_KEYS:
        del ck[k]
    torch.save(ck, str(tmp_path / "old.pt"))
    b, rb = make(reset_interval=20, reset_seed=3)
    stream = b._reset_stream().clone()
    assert b.load_checkpoint(str(tmp_path / "old.pt")) == 50
    assert b._reset_epoch == 2 and b.reset_count == 0 and torch.equal(b._reset_stream(), stream)
    assert _resets(traced(lambda: b.update(rb, Log(), 51))) == 0     # no catching up
    assert _resets(traced(lambda: b.update(rb, Log(), 60))) == 3
    off, _ = make()
    off.load_checkpoint(str(tmp_path / "old.pt"))
    assert off._reset_epoch == 0


# ------------------------------------------------------------------------------------------------------ staging layout
def _slots(tensors):
    """The flat image of a list of tensors: each on a 4-float slot, zeros between."""
    out = []
    for t in tensors:
        v = t.detach().reshape(-1)
        out += [v, torch.zeros((-v.numel()) % 4)]
    return torch.cat(out)


def _fc_yxc(w, c, h, wd):
    """An encoder fc weight's input columns from (c, y, x) to (y, x, c) order."""
    return w.detach().reshape(w.shape[0], c, h, wd).permute(0, 2, 3, 1).reshape(w.shape[0], -1)


@pytest.mark.parametrize("kw", [{}, dict(critic_layer_norm=True, critic_quantiles=5)])
@pytest.mark.parametrize("seed", [0, 11])
def test_staging_buffers_are_the_flat_images_of_freshly_constructed_networks(kw, seed):
    agent, _ = make(reset_seed=seed, **kw)
    traced(lambda: agent.reset_networks())
    # the recipe, on its own: torch's generator at the seed, then Actor, Critic, rand -- the constructor's order
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        obs, act, F = (C,) + OUT_HW, (2,), 50
        actor = Actor(obs, act, NET["hidden_dim"], F, -10, 2, NET["num_layers"], NET["num_filters"])
        q_kw = dict(quantiles=kw["critic_quantiles"]) if kw else {}
        critic = Critic(obs, act, NET["hidden_dim"], F, NET["num_layers"], NET["num_filters"],
                        layer_norm=bool(kw), **q_kw)
        W = torch.rand(F, F)
    enc = critic.encoder
    yxc = (NET["num_filters"],) + tuple(enc.out_dim)
    enc_t = [_fc_yxc(p, *yxc) if n == "fc.weight" else p for n, p in enc.named_parameters()]
    image = _slots([W] + enc_t + list(critic.Q1.parameters()) + list(critic.Q2.parameters()))
    got = agent._reset_stage["critic"]["host"]
    assert got.numel() == image.numel() == agent._critic_flat.numel()
    assert got.numpy().tobytes() == image.numpy().tobytes()
    if kw:
        assert critic.Q1.trunk[-1].weight.shape == (5, NET["hidden_dim"]) and len(list(critic.Q1.parameters())) == 10
    aenc = actor.encoder
    a_image = _slots([_fc_yxc(aenc.fc.weight, *yxc), aenc.fc.bias, aenc.ln.weight, aenc.ln.bias] + list(actor.trunk.parameters()))
    assert agent._reset_stage["actor"]["host"].numpy().tobytes() == a_image.numpy().tobytes()
    # and the live agent, built from the same seed, IS that image: the staging layout is the flat layout (but for W,
    # which the constructor draws behind the target critic as well)
    torch.manual_seed(seed)
    twin = curla_amd.CurlSacAgent((C,) + OUT_HW, (2,), "cpu", None, **NET, **kw)
    e0 = twin._lay["enc"][0]
    assert e0 == F * F and twin._critic_flat[e0:].numpy().tobytes() == image[e0:].numpy().tobytes()
    assert twin._actor_flat.numpy().tobytes() == a_image.numpy().tobytes()


def test_staging_buffers_are_allocated_once():
    agent, _ = make()
    traced(lambda: agent.reset_networks())
    ptrs = [(v["host"].data_ptr(), v["dev"].data_ptr()) for v in agent._reset_stage.values()]
    traced(lambda: agent.reset_networks())
    assert ptrs == [(v["host"].data_ptr(), v["dev"].data_ptr()) for v in agent._reset_stage.values()]
    assert agent._reset_stage["critic"]["dev"].numel() == agent._critic_flat.numel()
    assert torch.equal(agent._reset_stage["critic"]["dev"], agent._reset_stage["critic"]["host"])


# --------------------------------------------------------------------------------------------------------------- C ABI
def test_entry_point_is_declared_bound_and_exported():
    from curla_amd import ops
    name = "curla_shrink_perturb2"
    text = open(os.path.join(ROOT, "include", "curla_hip.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int %s\(([^;]*)\);" % name, text, flags=re.S)
    assert m, "include/curla_hip.h does not declare %s behind a comment" % name
    assert "Additive: CURLA_ABI_VERSION stays 8" in " ".join(m.group(1).replace("*", " ").split())
    params = [p.strip() for p in m.group(2).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == ["param", "target", "fresh", "n", "split", "keep_a", "new_a",
                                                          "keep_b", "new_b", "stream"]
    assert len(params) == len(_lib.SIGNATURES[name])
    for p, t in zip(params, _lib.SIGNATURES[name]):
        want = _lib.vp if "*" in p else _lib.c_size_t if p.startswith("size_t") else _lib.c_float
        assert t is want, (name, p)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert _lib.ABI_VERSION == 8 and _lib.load().curla_abi_version() == 8 and callable(ops.shrink_perturb2)
    kernels = open(os.path.join(ROOT, "curla_amd", "csrc", "optim.h")).read()
    assert kernels.index("soft_update2_kernel(") < kernels.index("shrink_perturb2_kernel(") < kernels.index("adam_one(")


def test_entry_point_checks_its_arguments_before_any_launch():
    """CURLA_ERR_ARG (-1) on a NULL param or fresh, n == 0, split > n and a keep outside [0, 1] or NaN -- all decided
    on the host, so a machine without a GPU sees them too (the pointers are never dereferenced)."""
    lib = _lib.load()
    p = 4096  # a non-NULL, aligned, never dereferenced address

    def sp(param=p, target=p, fresh=p, n=8, split=4, ka=0.5, kb=0.0):
        return lib.curla_shrink_perturb2(param, target, fresh, n, split, ka, 1.0 - ka, kb, 1.0 - kb, None)
    nan = float("nan")
    for bad in (dict(param=None), dict(fresh=None), dict(n=0, split=0), dict(split=9), dict(ka=-0.25), dict(ka=1.5),
                dict(kb=-1e-3), dict(kb=1.0 + 1e-3), dict(ka=nan), dict(kb=nan), dict(ka=float("inf")),
                dict(param=None, target=None)):
        assert sp(**bad) == -1, bad


def test_ops_wrapper_forms_one_minus_keep_in_double():
    from curla_amd import ops
    p, t, f = torch.zeros(16), torch.zeros(16), torch.zeros(16)
    calls = traced(lambda: ops.shrink_perturb2(p, t, f, 4, np.float32(0.8), 0.5))
    (name, args), = calls
    assert name == "curla_shrink_perturb2"
    assert args[3:9] == (16, 4, float(np.float32(0.8)), 1.0 - float(np.float32(0.8)), 0.5, 0.5)
    calls = traced(lambda: ops.shrink_perturb2(p, None, f, 16, 1.0, 0.0))
    assert calls[0][1][1] is None and calls[0][1][5:9] == (1.0, 0.0, 0.0, 1.0)
