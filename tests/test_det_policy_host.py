"""CurlSacAgent(policy="deterministic", policy_std=..., policy_std_clip=..., policy_std_schedule=...) on the host
(DESIGN.md 7m): the float64 reference (tests/_det_policy_ref.py) against plain loops and a finite difference, the
keywords' defaults and validation, what a seed reproduces and the state-dict contract, the std schedule, the launch list
of an update under the trace hook, log_alpha left alone, checkpoints, resets, and the new C entry points (declared,
bound, exported, argument checks).  No GPU: nothing here launches a kernel."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import _det_policy_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("curla_det_head_fwd", "curla_det_head_fwd_rng", "curla_mlp_out_det_head_fwd",
                "curla_mlp_out_det_head_fwd_rng", "curla_det_head_bwd", "curla_det_policy_head_bwd")
GAUSS_HEADS = ("curla_mlp_out_head_fwd", "curla_mlp_out_head_fwd_rng", "curla_actor_head_fwd", "curla_actor_head_fwd_rng",
               "curla_actor_head_bwd", "curla_policy_head_bwd")
A_, H_ = 2, 96
DET = dict(policy="deterministic")


def make_agent(seed=1, hidden=H_, **kw):
    import curla_amd
    torch.manual_seed(seed)
    return curla_amd.CurlSacAgent((9, 32, 36), (A_,), torch.device("cpu"), None, hidden_dim=hidden, num_layers=2,
                                  num_filters=8, **kw)


# ------------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("clip", [None, 0.0, 0.3, 5.0])
def test_reference_against_plain_loops(clip):
    g = torch.Generator().manual_seed(3)
    o, n = 2.0 * torch.randn(7, 3, generator=g), 2.0 * torch.randn(7, 3, generator=g)
    o[0, 0], o[1, 1], n[2, 2] = 20.0, -20.0, 0.0
    ref = R.forward(o, n, 0.7, clip)
    mu, pi = R.forward_loops(o.numpy(), n.numpy(), 0.7, clip)
    assert np.abs(ref["mu"].numpy() - np.array(mu)).max() <= 1e-15
    assert np.abs(ref["pi"].numpy() - np.array(pi)).max() <= 1e-15
    assert float(ref["pi"].abs().max()) <= R.LIM and not ref["log_pi"].any() and ref["log_pi"].shape == (7, 1)
    assert torch.equal(ref["log_std"], torch.full((7, 3), np.log(float(np.float32(0.7))), dtype=torch.float64))
    if clip == 0.0:
        assert torch.equal(ref["pi"], ref["mu"].clamp(-R.LIM, R.LIM))
    assert R.forward(o, None, 0.7, clip)["pi"] is None
    assert R.LIM == float(np.float32(1.0) - np.float32(1e-6)) == float(np.float32(0.999999))


def test_reference_gradient_against_a_central_finite_difference():
    """Off the clamps' kinks (|m + e| well inside lim): d sum(w pi) / d o and d sum(v mu) / d o by central differences in
    float64, h = 1e-6 (truncation ~h^2, rounding ~1e-16 / h: both far below the 1e-8 asked)."""
    g = torch.Generator().manual_seed(5)
    o = torch.randn(5, 3, generator=g, dtype=torch.float64)
    n = torch.randn(5, 3, generator=g)
    w, v = torch.randn(5, 3, generator=g, dtype=torch.float64), torch.randn(5, 3, generator=g, dtype=torch.float64)
    s, c, h = 0.05, 0.3, 1e-6
    assert float((torch.tanh(o) + s * n.double()).abs().max()) < 0.99

    def f(x):
        mu, pi = R.policy(x, n, s, c)
        return float((w * pi).sum() + (v * mu).sum())
    fd = torch.zeros_like(o)
    for i in range(o.numel()):
        d = torch.zeros(o.numel(), dtype=torch.float64)
        d[i] = h
        fd.view(-1)[i] = (f(o + d.view_as(o)) - f(o - d.view_as(o))) / (2 * h)
    want = R.grad_o(o, dpi=w, dmu=v)
    assert float((fd - want).abs().max()) <= 1e-8
    x = o.clone().requires_grad_(True)
    mu, pi = R.policy(x, n, s, c)
    ((w * pi).sum() + (v * mu).sum()).backward()
    assert float((x.grad - want).abs().max()) <= 1e-14
    # straight through the outer clamp: where it binds the gradient is still (1 - m^2) times the upstream one
    x = torch.tensor([[3.0, -3.0]], dtype=torch.float64, requires_grad=True)
    R.policy(x, torch.tensor([[4.0, -4.0]]), 0.5, None)[1].sum().backward()
    assert float((x.grad - (1 - torch.tanh(x.detach()) ** 2)).abs().max()) <= 1e-15 and float(x.grad.min()) > 9e-3


# ------------------------------------------------------------------------------------------------ keywords, validation
def test_keywords_and_defaults():
    import curla_amd
    from curla_amd.curl_sac import Actor
    init = list(inspect.signature(curla_amd.CurlSacAgent.__init__).parameters)
    assert init[-1] == "pixel_sac" and not any(k.startswith("policy") for k in init)
    call = inspect.signature(curla_amd.CurlSacAgent).parameters
    for k, default in (("policy", "gaussian"), ("policy_std", 0.2), ("policy_std_clip", 0.3), ("policy_std_schedule", None)):
        assert call[k].default == default and call[k].kind is inspect.Parameter.KEYWORD_ONLY
    p = inspect.signature(Actor).parameters["deterministic"]
    assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert "deterministic" not in inspect.signature(Actor.__init__).parameters
    off = make_agent()
    assert off.policy == "gaussian" and off.policy_std is None and off.actor.deterministic is False
    assert off.actor.trunk[-1].out_features == 2 * A_
    on = make_agent(**DET)
    assert on.policy == "deterministic" and on.policy_std == 0.2 and on.policy_std_clip == 0.3
    assert on.policy_std_schedule is None and on.actor.deterministic is True and on.actor.std_clip == 0.3
    assert on.actor.trunk[-1].out_features == A_
    assert on.actor.std.dtype == torch.float32 and on.actor.std.shape == (1,) and float(on.actor.std) == float(np.float32(0.2))
    assert "std" not in dict(on.actor.named_buffers()) and "std" not in on.actor.state_dict()
    on = make_agent(policy="deterministic", policy_std=np.float32(0.5), policy_std_clip=None, policy_std_schedule=[1, 0.1, 100])
    assert type(on.policy_std) is float and on.policy_std == 1.0 and on.policy_std_clip is None  # (the schedule at step 0)
    assert on.policy_std_schedule == (1.0, 0.1, 100.0) and on.actor.std_clip is None
    for text in (curla_amd.CurlSacAgent.__doc__, open(os.path.join(ROOT, "README.md")).read()):
        assert all(k in text for k in ("policy=\"deterministic\"", "policy_std", "policy_std_clip", "policy_std_schedule"))
    assert "7m" in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_an_agent_with_the_gaussian_policy_is_the_agent_without_the_keyword():
    plain, off = make_agent(), make_agent(policy="gaussian")
    assert sorted(plain.__dict__) == sorted(off.__dict__)
    assert sorted(plain.actor.__dict__) == sorted(off.actor.__dict__)
    assert plain._graph_key() == off._graph_key()
    assert list(plain.actor.state_dict()) == list(off.actor.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(plain._actor_flat.split(1), off._actor_flat.split(1)))
    on = make_agent(**DET)
    assert set(on.__dict__) - set(plain.__dict__) == {"policy", "_policy_std", "policy_std_clip", "policy_std_schedule",
                                                      "_dla_scratch"}
    assert set(on.actor.__dict__) - set(plain.actor.__dict__) == {"deterministic", "std", "std_clip"}
    k = on._graph_key()
    assert k[-1] == ("policy", "deterministic", 0.3) and k[:-1] == plain._graph_key()
    on.set_policy_std(0.9)  # std is data: not in the key
    assert on._graph_key() == k
    on.policy_std_clip = None
    assert on._graph_key()[-1] == ("policy", "deterministic", None)
    on.policy_std_clip = -1.0
    with pytest.raises(ValueError, match="policy_std_clip"):
        on._graph_key()


@pytest.mark.parametrize("bad", ["Gaussian", "td3", None, 1, True])
def test_policy_validation(bad):
    with pytest.raises(ValueError, match="policy: .* is not 'gaussian' or 'deterministic'"):
        make_agent(policy=bad)


@pytest.mark.parametrize("bad", [0, 0.0, -0.1, float("inf"), float("nan"), "0.2", None, True])
def test_policy_std_validation(bad):
    with pytest.raises(ValueError, match="policy_std: .* is not a finite number > 0"):
        make_agent(policy="deterministic", policy_std=bad)
    agent = make_agent(**DET)
    with pytest.raises(ValueError, match="policy_std"):
        agent.set_policy_std(bad)
    assert agent.policy_std == 0.2


@pytest.mark.parametrize("bad", [-0.1, float("inf"), float("nan"), "0.3", True])
def test_policy_std_clip_validation(bad):
    with pytest.raises(ValueError, match="policy_std_clip: .* is not a finite number >= 0 or None"):
        make_agent(policy="deterministic", policy_std_clip=bad)
    assert make_agent(policy="deterministic", policy_std_clip=0).policy_std_clip == 0.0


@pytest.mark.parametrize("bad", [(1.0, 0.1), (1.0, 0.1, 0.0), (0.0, 0.1, 10), (1.0, -0.1, 10), (1.0, float("nan"), 10),
                                 (float("inf"), 0.1, 10), 3.0, "abc", (1.0, 0.1, 10, 2)])
def test_policy_std_schedule_validation(bad):
    with pytest.raises(ValueError, match="policy_std_schedule"):
        make_agent(policy="deterministic", policy_std_schedule=bad)


@pytest.mark.parametrize("kw", [dict(policy_std=0.5), dict(policy_std_clip=None), dict(policy_std_clip=0.1),
                                dict(policy_std_schedule=(1.0, 0.1, 10))])
def test_the_keywords_need_the_deterministic_policy(kw):
    name = next(iter(kw))
    for extra in ({}, dict(policy="gaussian")):
        with pytest.raises(ValueError, match=name + " = .* needs policy='deterministic'"):
            make_agent(**kw, **extra)
    assert make_agent(policy="gaussian", policy_std=0.2, policy_std_clip=0.3, policy_std_schedule=None).policy == "gaussian"
    with pytest.raises(ValueError, match="set_policy_std needs policy='deterministic'"):
        make_agent().set_policy_std(0.3)


# ------------------------------------------------------------------------------------------ seeds, state dicts, resets
@pytest.mark.parametrize("kw", [{}, dict(critic_layer_norm=True), dict(critic_quantiles=5)])
def test_a_seed_reproduces_every_tensor_but_the_actors_last_layer(kw):
    off, on = make_agent(**kw), make_agent(**DET, **kw)
    a, b = off.actor.state_dict(), on.actor.state_dict()
    assert list(a) == list(b) and "trunk.4.weight" in a
    for k in a:
        if k.startswith("trunk.4."):
            assert tuple(b[k].shape) == ((A_, H_) if k.endswith("weight") else (A_,)) and tuple(a[k].shape)[0] == 2 * A_
        else:
            assert torch.equal(a[k], b[k]), k
    w = b["trunk.4.weight"]  # weight_init: orthogonal rows, zero bias
    assert float((w @ w.T - torch.eye(A_)).abs().max()) < 1e-5 and not b["trunk.4.bias"].any()
    for name in ("critic", "critic_target", "CURL"):
        x, y = getattr(off, name).state_dict(), getattr(on, name).state_dict()
        assert list(x) == list(y) and all(torch.equal(x[k], y[k]) for k in x), name
    assert torch.equal(off.log_alpha, on.log_alpha)
    torch.manual_seed(1)
    make_agent(**DET, **kw)
    after_on = torch.rand(3)
    torch.manual_seed(1)
    make_agent(**kw)
    assert torch.equal(after_on, torch.rand(3))
    with pytest.raises(RuntimeError, match="size mismatch"):
        on.actor.load_state_dict(off.actor.state_dict())
    # the flat layout follows the narrower layer: the data-parallel bucket is the flat gradient and the f64 words
    from curla_amd import ops
    assert on._actor_flat.numel() < off._actor_flat.numel()
    assert on._actor_gbucket.numel() == on._actor_flat.numel() + ops.F64_WORDS


def test_a_bare_actor_takes_the_keyword():
    from curla_amd.curl_sac import Actor
    torch.manual_seed(0)
    a = Actor((9, 32, 36), (3,), 64, 50, -10, 2, 2, 8, deterministic=True)
    assert a.deterministic and a.trunk[4].weight.shape == (3, 64) and list(a.state_dict())[-2:] == ["trunk.4.weight", "trunk.4.bias"]
    assert float(a.std) == float(np.float32(0.2)) and a.std_clip == 0.3
    torch.manual_seed(0)
    g = Actor((9, 32, 36), (3,), 64, 50, -10, 2, 2, 8)
    assert not g.deterministic and "std" not in g.__dict__ and torch.equal(g.trunk[2].weight, a.trunk[2].weight)


def test_reset_networks_draws_an_actor_of_the_same_kind():
    agent = make_agent(**DET)
    actor, _, _ = agent._draw_fresh()
    assert actor.deterministic and actor.trunk[-1].weight.shape == (A_, H_)
    assert dict(actor.named_parameters()).keys() == dict(agent.actor.named_parameters()).keys()
    assert not make_agent()._draw_fresh()[0].deterministic
    agent._stage_fresh()  # (every fresh tensor fits its live namesake's slot)


def test_redo_follows_the_narrower_last_layer():
    from curla_amd.mlp import _linears
    agent = make_agent(**DET, redo_interval=4)
    assert [tuple(m.weight.shape) for m in _linears(agent.actor.trunk)] == [(H_, 50), (H_, H_), (A_, H_)]


# ------------------------------------------------------------------------------------------------------- the schedule
def test_the_schedule_is_drq_v2s_linear():
    s = (1.0, 0.1, 100)
    assert R.linear(s, 0) == 1.0 and R.linear(s, 100) == pytest.approx(0.1, abs=1e-15) and R.linear(s, 10 ** 6) == R.linear(s, 100)
    assert R.linear(s, 50) == pytest.approx(0.55, abs=1e-15) and R.linear((0.2, 0.2, 1), 7) == 0.2
    from curla_amd.curl_sac import _linear_schedule
    for step in (0, 1, 37, 50, 99, 100, 101, 5000):
        assert _linear_schedule((1.0, 0.1, 100.0), step) == R.linear(s, step)


# --------------------------------------------------------------------------------------------------------- launch list
class _Log:
    def __init__(self):
        self.keys = []

    def log(self, key, *a, **k):
        self.keys.append(key)


def _traced_update(steps, prioritized=False, n_step=1, log_interval=100, **kw):
    """The launch lists of update() calls of a CPU agent under the trace hook (nothing is computed)."""
    import curla_amd
    from curla_amd import _lib
    aug = curla_amd.RandomCrop((34, 40), (28, 34))
    curla_amd.set_seed_everywhere(1)
    agent = curla_amd.CurlSacAgent((9, 28, 34), (2,), "cpu", aug, hidden_dim=64, log_interval=log_interval, **kw)
    rb = curla_amd.ReplayBuffer((9, 34, 40), (2,), 32, 8, "cpu", aug, **(dict(prioritized=True) if prioritized else {}),
                                **(dict(n_step=n_step, discount=agent.discount) if n_step > 1 else {}))
    for _ in range(12):
        rb.add(np.zeros((9, 34, 40), np.uint8), [0, 0], 0.0, np.zeros((9, 34, 40), np.uint8), False)
    log, out = _Log(), []
    for step in steps:
        calls = []
        _lib.set_trace_hook(lambda name, args: calls.append((name, args)))
        try:
            agent.update(rb, log, step)
        finally:
            _lib.set_trace_hook(None)
        out.append(calls)
    return agent, out, log


@pytest.mark.parametrize("step", [2, 1])
@pytest.mark.parametrize("kw", [{}, dict(critic_layer_norm=True, critic_dropout=0.1), dict(critic_quantiles=5),
                                dict(critic_bins=5, critic_value_range=(-4.0, 6.0)), dict(prioritized=True), dict(n_step=3)],
                         ids=["plain", "ln_dropout", "tqc", "hlg", "per", "n_step"])
def test_launch_list_swaps_the_heads_and_nothing_else(step, kw):
    """An even (critic + actor + CURL) and an odd update: the deterministic agent launches the deterministic head where
    the Gaussian agent launches its own -- fused into the last layer, so no launch more --, the deterministic backward in
    place of actor_head_bwd, and every other launch is the Gaussian agent's, name for name; policy='gaussian' launches
    what no keyword launches."""
    _, (off,), _ = _traced_update([step], **kw)
    _, (off0,), _ = _traced_update([step], policy="gaussian", **kw)
    assert [n for n, _ in off] == [n for n, _ in off0]
    agent, (on,), _ = _traced_update([step], **DET, **kw)
    names_off, names_on = [n for n, _ in off], [n for n, _ in on]
    assert not any(n in ENTRY_POINTS for n in names_off) and not any(n in GAUSS_HEADS for n in names_on)
    assert len(names_on) == len(names_off)
    swap = {"curla_mlp_out_head_fwd": "curla_mlp_out_det_head_fwd", "curla_actor_head_bwd": "curla_det_head_bwd"}
    assert [swap.get(n, n) for n in names_off] == names_on
    even = step % 2 == 0
    assert names_on.count("curla_mlp_out_det_head_fwd") == (2 if even else 1)
    assert names_on.count("curla_det_head_bwd") == (1 if even else 0)
    B, A, F = 8, 2, 50
    ws = agent._ws(B)
    assert ws.a_out.shape == ws.a_dout.shape == (B, A)
    heads = [a for n, a in on if n == "curla_mlp_out_det_head_fwd"]
    for a in heads:  # (h, W, bias, trunk_out, B, A, K, noise, std, clip, mu, pi, log_pi, log_std, pi_xa, xa_ld, stream)
        assert a[3] == ws.a_out.data_ptr() and a[4:7] == (B, A, 64) and a[7] == ws.noise.data_ptr()
        assert a[8] == agent.actor.std.data_ptr() and a[9] == 0.3 and a[12] == ws.log_pi.data_ptr()
    if even:
        a = heads[1]  # the actor phase: mu for the backward, the action columns of xa, no pi
        assert a[10] == ws.mu.data_ptr() and a[11] is None and a[13] == ws.log_std.data_ptr()
        assert a[14] == ws.xa.data_ptr() + 4 * F and a[15] == F + A
        a = dict(on)["curla_det_head_bwd"]  # (gpi, gpi2, gpi_ld, mu, B, A, dtrunk_out, stream)
        assert a[0] == ws.dxa.data_ptr() + 4 * F and a[1] == a[0] + 4 * B * (F + A) and a[2] == F + A
        assert a[3] == ws.mu.data_ptr() and a[4:6] == (B, A) and a[6] == ws.a_dout.data_ptr()


@pytest.mark.parametrize("kw", [{}, dict(critic_quantiles=5), dict(critic_bins=5, critic_value_range=(-4.0, 6.0))],
                         ids=["plain", "tqc", "hlg"])
def test_the_actor_loss_leaves_log_alphas_gradient_in_a_scratch_word(kw):
    """Every form of the actor loss -- the fields of the loss-in-backward launch and the loss kernels on their own --
    is handed the scratch float64 as dlog_alpha; log_alpha.grad is never a launch's argument."""
    from curla_amd import _lib
    for det in (True, False):
        agent, _, _ = _traced_update([2], **(DET if det else {}), **kw)
        want = agent._dla_scratch if det else agent.log_alpha.grad
        assert want.dtype == torch.float64 and want.shape == ()
        fields, launch = agent._actor_loss(agent._ws(8))
        if fields is not None:
            assert fields["dlog_alpha"] is want
        calls = []
        _lib.set_trace_hook(lambda name, args: calls.append((name, args)))
        try:
            launch()
        finally:
            _lib.set_trace_hook(None)
        (name, args), = calls
        assert "actor_loss" in name and args[-2] == want.data_ptr()
        if det:
            assert agent.log_alpha.grad.data_ptr() not in [x for x in args if isinstance(x, int)]
            assert not agent.log_alpha.grad.any()


def test_policy_std_clip_none_is_passed_as_infinity_and_an_edit_is_seen_by_the_next_update():
    agent, (a, b), _ = _traced_update([1, 3], policy="deterministic", policy_std_clip=None)
    assert dict(a)["curla_mlp_out_det_head_fwd"][9] == float("inf")
    agent, (a,), _ = _traced_update([1], policy="deterministic", policy_std_clip=0)
    assert dict(a)["curla_mlp_out_det_head_fwd"][9] == 0.0


def test_logging_keys():
    _, _, off = _traced_update([2], log_interval=1)
    _, _, on = _traced_update([2], log_interval=1, **DET)
    gone = {"train_actor/entropy", "train_actor/target_entropy", "train_alpha/loss", "train_alpha/value"}
    assert set(off.keys) - set(on.keys) == gone and set(on.keys) - set(off.keys) == {"train_actor/std"}
    assert "train_actor/loss" in on.keys and "train_critic/loss" in on.keys


def test_the_schedule_moves_std_at_the_top_of_update_and_only_when_it_changes():
    agent, _, _ = _traced_update([], policy="deterministic", policy_std_schedule=(1.0, 0.5, 10))
    assert agent.policy_std == 1.0 and float(agent.actor.std) == 1.0
    fills = []
    real = agent.actor.std.fill_

    class Std:  # counts the fills of the device scalar
        def __getattr__(self, k):
            return getattr(real.__self__, k)

        def fill_(self, v):
            fills.append(v)
            return real(v)
    from curla_amd import _lib
    std = agent.actor.std
    agent.actor.std = Std()
    agent.set_policy_std(1.0)
    assert fills == []
    agent.set_policy_std(0.75)
    agent.set_policy_std(0.75)
    assert fills == [0.75] and float(std) == 0.75 and agent.policy_std == 0.75
    agent.actor.std = std
    _lib.set_trace_hook(lambda *a: None)
    try:
        import curla_amd
        aug = curla_amd.RandomCrop((34, 40), (28, 34))
        rb = curla_amd.ReplayBuffer((9, 34, 40), (2,), 32, 8, "cpu", aug)
        for _ in range(12):
            rb.add(np.zeros((9, 34, 40), np.uint8), [0, 0], 0.0, np.zeros((9, 34, 40), np.uint8), False)
        for step, want in ((0, 1.0), (5, 0.75), (10, 0.5), (11, 0.5), (1000, 0.5)):
            agent.update(rb, _Log(), step)
            assert agent.policy_std == want and float(std) == float(np.float32(want)), step
    finally:
        _lib.set_trace_hook(None)


def test_log_alpha_and_its_adam_state_are_left_alone():
    """A CPU agent's optimizers are torch's own and really step under the trace hook: log_alpha.grad stays all zeros, so
    Adam's step with zero gradient and zero moments leaves the value bit for bit where construction put it."""
    agent, _, _ = _traced_update([], **DET)
    la0 = agent.log_alpha.detach().clone()
    agent2, _, _ = _traced_update([0, 1, 2, 3, 4], **DET)
    assert torch.equal(agent2.log_alpha.detach(), la0) and agent2.log_alpha.dtype == torch.float64
    assert not agent2.log_alpha.grad.any()
    st = agent2.log_alpha_optimizer.state[agent2.log_alpha]
    assert float(st["step"]) == 3 and not st["exp_avg"].any() and not st["exp_avg_sq"].any()
    gauss, _, _ = _traced_update([0], policy="gaussian")
    assert torch.equal(gauss.log_alpha.detach(), la0)


def test_refusals_stay_where_they_are():
    for kw in (dict(critic_quantiles=5), dict(critic_bins=5, critic_value_range=(-4.0, 6.0))):
        with pytest.raises(ValueError, match="prioritized"):
            _traced_update([1], prioritized=True, **DET, **kw)
    with pytest.raises(ValueError, match="aug_views"):
        make_agent(aug_views=2, critic_quantiles=5, **DET)


# --------------------------------------------------------------------------------------------------------- checkpoints
def test_checkpoint_carries_the_policy(tmp_path):
    agent = make_agent(policy="deterministic", policy_std=0.4, policy_std_clip=None, policy_std_schedule=(0.4, 0.1, 50))
    agent.set_policy_std(0.33)
    ck = tmp_path / "det.pt"
    agent.save_checkpoint(str(ck), 7)
    saved = torch.load(str(ck), map_location="cpu", weights_only=False)
    assert saved["policy"] == "deterministic" and saved["policy_std"] == 0.33 and saved["policy_std_clip"] is None
    assert saved["policy_std_schedule"] == (0.4, 0.1, 50.0)
    other = make_agent(seed=2, **DET)
    assert other.load_checkpoint(str(ck)) == 7
    assert other.policy_std == 0.33 and float(other.actor.std) == float(np.float32(0.33)) and other.policy_std_clip is None
    assert other.policy_std_schedule == (0.4, 0.1, 50.0)
    for k, v in agent.actor.state_dict().items():
        assert torch.equal(v, other.actor.state_dict()[k]), k
    with pytest.raises(RuntimeError, match="size mismatch"):
        make_agent().load_checkpoint(str(ck))
    plain = tmp_path / "plain.pt"
    make_agent().save_checkpoint(str(plain), 1)
    assert not any(k.startswith("policy") for k in torch.load(str(plain), map_location="cpu", weights_only=False))
    with pytest.raises(RuntimeError, match="size mismatch"):
        make_agent(**DET).load_checkpoint(str(plain))


# -------------------------------------------------------------------------------------------------------- entry points
def test_entry_points_are_declared_bound_and_exported():
    import __graft_entry__ as ge
    ge.build()
    from curla_amd import _lib, ops
    text = open(os.path.join(ROOT, "include", "curla_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        m = re.search(r"\bint %s\(([^;]*)\);" % name, text)
        assert m, f"include/curla_hip.h does not declare {name}"
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        assert len(params) == len(_lib.SIGNATURES[name]), name
        for p, t in zip(params, _lib.SIGNATURES[name]):
            want = (_lib.vp if "*" in p else _lib.c_u64 if p.startswith("unsigned long long") else _lib.c_float
                    if p.startswith("float") else _lib.c_int)
            assert t is want, (name, p)
        assert hasattr(lib, name)
    assert "Additive: CURLA_ABI_VERSION stays 8" in text[text.index("deterministic policy head"):text.index("int curla_det_head_fwd(")]
    assert _lib.ABI_VERSION == 8 and _lib.load().curla_abi_version() == 8
    for f in ("det_head_fwd", "mlp_out_det_head_fwd", "det_head_bwd", "det_policy_head_bwd"):
        assert callable(getattr(ops, f))
    kernels = open(os.path.join(ROOT, "curla_amd", "csrc", "mlp_out.h")).read()
    assert all(k in kernels for k in ("det_head_one", "det_head_fwd_kernel", "det_head_bwd_kernel", "det_policy_head_bwd_kernel"))
    assert "atomic" not in kernels and "asm" not in kernels


def test_entry_points_check_their_arguments_before_any_launch():
    """CURLA_ERR_ARG (-1) on A < 1 or A > 8, B < 1, a NULL required pointer, clip < 0 or NaN -- all decided on the host,
    so a machine without a GPU sees them too (the pointers are never dereferenced)."""
    from curla_amd import _lib
    lib = _lib.load()
    p = 4096  # a non-NULL, aligned, never dereferenced address
    nan = float("nan")

    def fwd(o=p, n=p, std=p, clip=0.3, B=4, A=2, mu=p, pi=p, lp=p, ls=p, xa=None, ld=0):
        return lib.curla_det_head_fwd(o, n, std, clip, B, A, mu, pi, lp, ls, xa, ld, None)

    def fwd_rng(o=p, nz=p, dev=None, std=p, clip=0.3, B=4, A=2, pi=p):
        return lib.curla_det_head_fwd_rng(o, nz, 1, 2, dev, std, clip, B, A, p, pi, p, p, None, 0, None)

    def fused(h=p, W=p, o=p, n=p, std=p, clip=0.3, B=4, A=2, K=64, pi=p):
        return lib.curla_mlp_out_det_head_fwd(h, W, p, o, B, A, K, n, std, clip, p, pi, p, p, None, 0, None)

    def fused_rng(h=p, W=p, o=p, nz=p, std=p, clip=0.3, B=4, A=2, K=64):
        return lib.curla_mlp_out_det_head_fwd_rng(h, W, p, o, B, A, K, nz, 1, 2, None, std, clip, p, p, p, p, None, 0, None)

    def bwd(g=p, g2=None, ld=2, mu=p, B=4, A=2, d=p):
        return lib.curla_det_head_bwd(g, g2, ld, mu, B, A, d, None)

    def gen(dmu=p, dpi=p, mu=p, B=4, A=2, d=p):
        return lib.curla_det_policy_head_bwd(dmu, dpi, mu, B, A, d, None)
    common = (dict(A=0), dict(A=-1), dict(A=9), dict(B=0), dict(B=-3), dict(std=None), dict(clip=-0.1), dict(clip=nan),
              dict(clip=-float("inf")), dict(o=None))
    for bad in common + (dict(pi=None), dict(xa=p, ld=1), dict(xa=p, n=None, ld=4)):
        assert fwd(**bad) == -1, bad
    for bad in common + (dict(nz=None), dict(dev=4100), dict(pi=None)):
        assert fwd_rng(**bad) == -1, bad
    for bad in common + (dict(h=None), dict(W=None), dict(K=0), dict(h=4100), dict(pi=None)):
        assert fused(**bad) == -1, bad
    for bad in common + (dict(h=None), dict(W=None), dict(nz=None)):
        assert fused_rng(**bad) == -1, bad
    assert fused(K=66) == -3  # CURLA_ERR_UNSUPPORTED: K % 4
    for bad in (dict(g=None), dict(mu=None), dict(d=None), dict(B=0), dict(A=0), dict(A=9), dict(ld=1)):
        assert bwd(**bad) == -1, bad
    for bad in (dict(mu=None), dict(d=None), dict(B=0), dict(A=0), dict(A=9)):
        assert gen(**bad) == -1, bad
