"""CurlSacAgent(cpc_objective="predictive", predictor_hidden=H) on the host: the float64 reference of the
loss (tests/_pred_ref.py) against the closed form of its gradient, the keywords' defaults and validation, what a seed
reproduces, the flat layout, the C entry point (declared, bound, exported, argument checks), the launch list of an update
under the trace hook and every refusal -- each before any launch or write.  No GPU: nothing here launches a kernel."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import _pred_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F_, A_, H_ = 50, 2, 64
B_ = 8


def make_agent(seed=1, aug=None, **kw):
    import curla_amd
    torch.manual_seed(seed)
    return curla_amd.CurlSacAgent((9, 28, 34), (A_,), "cpu", aug, hidden_dim=H_, log_interval=100, **kw)


def make_buffer(aug, **kw):
    import curla_amd
    rb = curla_amd.ReplayBuffer((9, 34, 40), (A_,), 32, B_, "cpu", aug, **kw)
    for _ in range(12):
        rb.add(np.zeros((9, 34, 40), np.uint8), [0, 0], 0.0, np.zeros((9, 34, 40), np.uint8), False)
    return rb


class Log:
    def __init__(self):
        self.keys = []

    def log(self, key, *a, **k):
        self.keys.append(key)


def traced(fn):
    """The (name, args) launch list of ``fn()`` under the trace hook (nothing is computed)."""
    from curla_amd import _lib
    calls = []
    _lib.set_trace_hook(lambda name, args: calls.append((name, args)))
    try:
        fn()
    finally:
        _lib.set_trace_hook(None)
    return calls


def traced_update(step, only_cpc=False, rb_kw=None, **kw):
    import curla_amd
    aug = curla_amd.RandomCrop((34, 40), (28, 34))
    curla_amd.set_seed_everywhere(1)
    agent = make_agent(aug=aug, **kw)
    rb = make_buffer(aug, **(dict(pos_offset=1) if rb_kw is None else rb_kw))
    log = Log()
    calls = traced(lambda: agent.update(rb, log, step, only_cpc=only_cpc))
    return agent, calls, log


def names(calls):
    return [n for n, _ in calls]


def is_orthogonal(w):
    """weight_init's Linear weights: orthonormal rows or columns, whichever are fewer."""
    w = w.detach().double()
    gram = w @ w.T if w.shape[0] <= w.shape[1] else w.T @ w
    return float((gram - torch.eye(gram.shape[0], dtype=torch.float64)).abs().max()) <= 1e-5


# ------------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("B,Fd", [(1, 1), (3, 2), (5, 50), (9, 65)])
def test_reference_against_the_closed_form(B, Fd):
    """autograd's float64 gradient is the issue's formula: (2 / B)(I - ph ph^T)(ph - th) / |p| for |p| >= eps and
    (2 / B)(ph - th) / eps below it; the row loss is 2 - 2 cos(p, t) where neither vector is zero."""
    p, t, where = R.inputs(B, Fd)
    rows, total, dp = R.loss(p, t)
    p64, t64 = p.double(), t.double()
    n_p, n_t = p64.norm(dim=-1, keepdim=True), t64.norm(dim=-1, keepdim=True)
    ph, th = p64 / n_p.clamp_min(R.EPS), t64 / n_t.clamp_min(R.EPS)
    d = ph - th
    want = torch.where(n_p >= R.EPS, (2.0 / B) * (d - ph * (ph * d).sum(-1, keepdim=True)) / n_p.clamp_min(R.EPS),
                       (2.0 / B) * d / R.EPS)
    scale = torch.maximum(want.abs().amax(-1), R.dp_scale(p, B))
    assert float(((dp - want).abs().amax(-1) / scale).max()) <= 1e-12
    live = ((n_p > 0) & (n_t > 0)).reshape(-1)
    cos = (ph * th).sum(-1)
    assert float((rows - (2 - 2 * cos))[live].abs().max()) <= 1e-12
    assert abs(float(total) - float(rows.mean())) <= 1e-15 and bool(torch.isfinite(dp).all())
    for name, value in (("p_is_t", 0.0), ("p_is_minus_t", 4.0), ("p_zero", 1.0), ("t_zero", 1.0)):
        if name in where:
            assert abs(float(rows[where[name]]) - value) <= 1e-12
    if "orthogonal" in where and Fd >= 2:
        assert abs(float(rows[where["orthogonal"]]) - 2.0) <= 1e-12


@pytest.mark.parametrize("n", [1, 2, 67, 255, 256, 257, 515])
def test_the_restated_mean_is_a_float32_mean(n):
    x = np.random.default_rng(n).uniform(0, 4, n).astype(np.float32)
    got = R.fixed_order_mean(x)
    assert got.dtype == np.float32 and abs(float(got) - float(x.astype(np.float64).mean())) <= 4 * 12 * 2.0 ** -24


# ------------------------------------------------------------------------------------------------ keywords, validation
def test_keywords_and_defaults():
    import curla_amd
    from curla_amd import agent_cpc, ops
    init = list(inspect.signature(curla_amd.CurlSacAgent.__init__).parameters)
    assert init[-1] == "pixel_sac" and "cpc_objective" not in init and "predictor_hidden" not in init
    call = inspect.signature(curla_amd.CurlSacAgent).parameters
    for k, default in (("cpc_objective", "infonce"), ("predictor_hidden", None)):
        assert call[k].default == default and call[k].kind is inspect.Parameter.KEYWORD_ONLY
    # update_cpc takes ``action=`` behind the reference's five arguments (default None); what introspection lists stays
    # the reference's (the drop-in contract pins it name for name)
    up = curla_amd.CurlSacAgent.update_cpc
    assert up.__code__.co_varnames[:7] == ("self", "obs_anchor", "obs_pos", "cpc_kwargs", "L", "step", "action")
    assert up.__defaults__ == (None,)
    assert list(inspect.signature(up).parameters)[1:] == ["obs_anchor", "obs_pos", "cpc_kwargs", "L", "step"]
    assert agent_cpc.OBJECTIVES == ("infonce", "predictive") and ops.PRED_MAX == 1024
    assert issubclass(curla_amd.CurlSacAgent, agent_cpc._CpcMixin)
    off = make_agent()
    assert off.cpc_objective == "infonce" and off.predictor_hidden is None and not hasattr(off.CURL, "predictor")
    on = make_agent(cpc_objective="predictive")
    assert on.cpc_objective == "predictive" and on.predictor_hidden == H_ and type(on.predictor_hidden) is int
    assert make_agent(cpc_objective="predictive", predictor_hidden=np.int64(24)).predictor_hidden == 24
    for text in (curla_amd.CurlSacAgent.__doc__, open(os.path.join(ROOT, "README.md")).read()):
        assert "cpc_objective" in text and "predictor_hidden" in text
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## 7n." in design and "agent_cpc.py" in design and "curla_pred_loss" in design


@pytest.mark.parametrize("bad", ["", "spr", "Predictive", None, 1, True, b"predictive"])
def test_an_unknown_objective_is_refused(bad):
    with pytest.raises(ValueError, match="cpc_objective"):
        make_agent(cpc_objective=bad)


@pytest.mark.parametrize("bad", [0, -1, 2.0, True, "64", (64,)])
def test_predictor_hidden_must_be_a_positive_int(bad):
    with pytest.raises(ValueError, match="predictor_hidden"):
        make_agent(cpc_objective="predictive", predictor_hidden=bad)
    with pytest.raises(ValueError, match="predictor_hidden"):
        make_agent(predictor_hidden=bad)


def test_predictor_hidden_needs_the_objective_and_pixel_sac_is_refused():
    with pytest.raises(ValueError, match="predictor_hidden needs"):
        make_agent(predictor_hidden=32)
    torch.manual_seed(1)
    before = torch.random.get_rng_state()
    with pytest.raises(ValueError, match="pixel_sac"):
        import curla_amd
        curla_amd.CurlSacAgent((9, 28, 34), (A_,), "cpu", None, hidden_dim=H_, cpc_objective="predictive", pixel_sac=True)
    assert torch.equal(before, torch.random.get_rng_state())  # (refused before a network was drawn)
    assert make_agent(pixel_sac=True).pixel_sac  # (the default objective beside pixel SAC: as ever)


# ------------------------------------------------------------------------------------- the default agent is the parent's
def test_a_default_agent_is_the_agent_without_the_keywords():
    plain, off = make_agent(), make_agent(cpc_objective="infonce", predictor_hidden=None)
    assert sorted(plain.__dict__) == sorted(off.__dict__)
    assert sorted(plain.CURL.__dict__["_modules"]) == sorted(off.CURL.__dict__["_modules"]) == ["encoder", "encoder_target"]
    assert plain._lay == off._lay and plain._lay["w"] == (0, F_ * F_) and plain._graph_key() == off._graph_key()
    assert not any(isinstance(k, tuple) and k and k[0] == "cpc" for k in plain._graph_key())
    for a, b in ((plain.critic, off.critic), (plain.actor, off.actor), (plain.CURL, off.CURL)):
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert [tuple(p.shape) for p in plain.cpc_optimizer.param_groups[0]["params"]][0] == (F_, F_)
    assert plain.cpc_optimizer.param_groups[0]["params"][0] is plain.CURL.W
    # the construction's draws from torch's generator: the same number, so the stream stands where it stood
    torch.manual_seed(1)
    make_agent(seed=1)
    after_plain = torch.rand(3)
    make_agent(seed=1, cpc_objective="infonce")
    assert torch.equal(after_plain, torch.rand(3))


@pytest.mark.parametrize("step,only_cpc", [(1, False), (2, False), (100, False), (3, True)])
def test_a_default_agents_launch_lists_are_those_without_the_keywords(step, only_cpc):
    """Every kind of update -- odd, even, a logging step, only_cpc -- with and without the (default) keywords, on a
    buffer with and without temporal positives: the same launches with the same integer arguments."""
    for rb_kw in ({}, dict(pos_offset=1)):
        _, plain, log_a = traced_update(step, only_cpc, rb_kw=rb_kw)
        _, off, log_b = traced_update(step, only_cpc, rb_kw=rb_kw, cpc_objective="infonce", predictor_hidden=None)
        assert names(plain) == names(off) and log_a.keys == log_b.keys
        ints = lambda calls: [[a for a in args if isinstance(a, int) and abs(a) < 2 ** 20] for _, args in calls]  # noqa: E731
        assert ints(plain) == ints(off)
        assert "curla_pred_loss" not in names(plain)
        assert ("train/curl_loss" in log_a.keys) == (step % 100 == 0) and "train/pred_loss" not in log_a.keys


# ------------------------------------------------------------------------------------------------- the predictive agent
def test_a_seeded_predictive_agent_has_the_default_agents_networks_and_a_predictor_behind_them():
    from curla_amd.optim import FlatAdam
    plain, on = make_agent(), make_agent(cpc_objective="predictive", predictor_hidden=24)
    for a, b in ((plain.critic, on.critic), (plain.critic_target, on.critic_target), (plain.actor, on.actor)):
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert torch.equal(plain.CURL.W, on.CURL.W) and torch.equal(plain.log_alpha, on.log_alpha)
    pred = on.CURL.predictor
    assert [type(m).__name__ for m in pred] == ["Linear", "ReLU", "Linear"]
    assert pred[0].weight.shape == (24, F_ + A_) and pred[2].weight.shape == (F_, 24)
    for lin in (pred[0], pred[2]):  # weight_init: orthogonal weights, zero biases
        assert is_orthogonal(lin.weight) and not bool(lin.bias.any())
    extra = ["predictor.0.weight", "predictor.0.bias", "predictor.2.weight", "predictor.2.bias"]
    assert list(on.CURL.state_dict()) == list(plain.CURL.state_dict()) + extra
    # the flat layout: the predictor behind W in the W group, every later offset moved by its (aligned) size
    size = sum((p.numel() + 3) & ~3 for p in pred.parameters())
    assert on._lay["w"] == (0, F_ * F_ + size) and on._lay["qblock"] == plain._lay["qblock"]
    for k in ("enc", "q"):
        assert on._lay[k] == tuple(v + size for v in plain._lay[k])
    assert on._lay["total"] == plain._lay["total"] + size == on._critic_flat.numel() == on._target_flat.numel()
    base = on._critic_flat.data_ptr()
    assert on.CURL.W.data_ptr() == base  # (the same slot)
    off = F_ * F_
    for p in pred.parameters():
        assert p.data_ptr() == base + 4 * off and p.grad.data_ptr() == on._critic_gflat.data_ptr() + 4 * off
        off += (p.numel() + 3) & ~3
    assert on.critic.encoder.convs[0].weight.data_ptr() == base + 4 * on._lay["enc"][0]
    assert not bool(on._target_flat[:on._lay["w"][1]].any())  # (the target's unused slot)
    # cpc_optimizer: [predictor | encoder] -- W belongs to no optimizer (never stepped, never decayed)
    params = on.cpc_optimizer.param_groups[0]["params"]
    assert [id(p) for p in params[:4]] == [id(p) for p in pred.parameters()]
    assert all(p is not on.CURL.W for o in on._optimizers().values() for g in o.param_groups for p in g["params"])
    assert len(params) == 4 + len(list(on.critic.encoder.parameters()))
    span = FlatAdam(params, on._critic_flat, on._critic_gflat)  # (a CPU agent's optimizers are torch's: the flat one's view)
    # ONE run of the flat buffer from the predictor's first float to the encoder's last (the slot's alignment padding
    # behind it, at most 3 floats, is no parameter's), the encoder its tail: what FlatAdam.step_pair fuses
    assert span._lo == F_ * F_ and span._hi <= on._lay["enc"][1] <= span._hi + 3
    assert span._single_run()[:2] == (span._lo, span._hi)
    # graph key, checkpoint entries
    assert on._graph_key()[-1] == ("cpc", "predictive", 24) and on._graph_key()[:-1] == plain._graph_key()
    assert on._cpc_checkpoint() == {"cpc_objective": "predictive", "predictor_hidden": 24} and plain._cpc_checkpoint() == {}
    assert set(on.__dict__) - set(plain.__dict__) == {"cpc_objective", "predictor_hidden"}


@pytest.mark.parametrize("step,only_cpc", [(1, False), (2, False), (100, False), (3, True)])
def test_the_predictive_phases_launch_list(step, only_cpc):
    agent, calls, log = traced_update(step, only_cpc, cpc_objective="predictive", predictor_hidden=24)
    _, plain, _ = traced_update(step, only_cpc)
    got = names(calls)
    assert got.count("curla_pred_loss") == 1
    assert not any(n in got for n in ("curla_curl_head", "curla_curl_ce", "curla_curl_ce_views"))
    assert ("train/pred_loss" in log.keys) == (step % 100 == 0) and "train/curl_loss" not in log.keys
    ws, Hp = agent._ws(B_), 24
    i = got.index("curla_pred_loss")
    a = calls[i][1]
    assert a[0] == ws.p_out.data_ptr() and a[1] == ws.z_pos.data_ptr() and a[2:4] == (B_, F_)
    assert a[4] == ws.row_loss.data_ptr() and a[6] == ws.p_dout.data_ptr()
    assert a[5] == (ws.scalars.data_ptr() + 20 if step % 100 == 0 else None)  # (scalars[5]: only when it is logged)
    # the head's own launches, in order: concat, two forward products | the loss | the predictor's backward
    assert got[i - 3:i] == ["curla_concat", "curla_gemm", "curla_gemm"]
    assert got[i + 1:i + 7] == ["curla_gemm", "curla_colsum", "curla_gemm", "curla_gemm", "curla_colsum", "curla_gemm"]
    cat = calls[i - 3][1]
    assert cat[0] == ws.z_c.data_ptr() and cat[2:5] == (B_, F_, A_) and cat[5] == ws.p_xa.data_ptr()
    l1, l2 = agent.CURL.predictor[0], agent.CURL.predictor[2]
    fwd1, fwd2 = calls[i - 2][1], calls[i - 1][1]
    assert fwd1[4] == l1.weight.data_ptr() and fwd1[11:14] == (B_, Hp, F_ + A_) and fwd1[20] == 1  # (the ReLU epilogue)
    assert fwd2[4] == l2.weight.data_ptr() and fwd2[11:14] == (B_, F_, Hp) and fwd2[20] == 0
    dz = calls[i + 6][1]  # d(loss)/d(z_c): the first F columns of the first layer's input gradient
    assert dz[0] == ws.p_dh.data_ptr() and dz[4] == l1.weight.data_ptr() and dz[5:7] == (1, F_ + A_)  # (k-major, ld F + A)
    assert dz[8] == ws.dz.data_ptr() and dz[9] == F_ and dz[11:14] == (B_, F_, Hp)
    dw = {calls[i + k][1][8] for k in (1, 4)}
    assert dw == {l2.weight.grad.data_ptr(), l1.weight.grad.data_ptr()}
    assert {calls[i + k][1][5] for k in (2, 5)} == {l2.bias.grad.data_ptr(), l1.bias.grad.data_ptr()}
    # everything in front of the head and behind it is the default agent's (the encoders' passes, the encoder's backward
    # as the unfused CURL route calls it, the optimizer steps)
    j = names(plain).index("curla_curl_ce")
    assert got[:i - 3] == names(plain)[:j - 2]  # (in front of CURL's head: W z_pos^T, the logits)
    assert got[i + 7:] == names(plain)[j + 4:]  # (behind it: its three backward products)


def test_reset_networks_stages_a_fresh_predictor_from_the_reset_stream():
    plain, on = make_agent(reset_seed=5), make_agent(cpc_objective="predictive", reset_seed=5)
    calls_on = traced(lambda: on.reset_networks(encoder_keep=0.5))
    calls_off = traced(lambda: plain.reset_networks(encoder_keep=0.5))
    assert names(calls_on) == names(calls_off) == ["curla_shrink_perturb2"] * 3
    assert calls_on[0][1][3] == calls_on[0][1][4] == on._lay["w"][1]  # (the W group's launch covers the predictor)
    host_on, host_off = on._reset_stage["critic"]["host"], plain._reset_stage["critic"]["host"]
    assert torch.equal(host_on[:F_ * F_], host_off[:F_ * F_])  # (the same fresh W: the predictor is drawn behind it)
    w0, w1 = on._lay["w"]
    l1 = on.CURL.predictor[0]
    fresh = host_on[F_ * F_:F_ * F_ + l1.weight.numel()].view(l1.weight.shape)
    assert is_orthogonal(fresh) and not torch.equal(fresh, l1.weight)  # (weight_init's; fresh values, not the live ones)
    assert torch.equal(host_on[w1:], host_off[F_ * F_:])  # (the fresh encoder and Q functions: the default's)
    assert not torch.equal(on._reset_rng, plain._reset_rng)  # (the stream has moved on by the predictor's draws)


# ----------------------------------------------------------------------------------------------------------- refusals
class NoOffset:
    """A replay buffer without the attribute (its sampler must never be reached)."""

    def sample_cpc(self):
        raise AssertionError("update() drew a minibatch before it refused the buffer")


@pytest.mark.parametrize("rb_kw", [dict(), dict(pos_offset=0), dict(pos_offset=2), None])
def test_update_refuses_a_buffer_whose_positive_is_not_the_next_observation(rb_kw):
    import curla_amd
    aug = curla_amd.RandomCrop((34, 40), (28, 34))
    agent = make_agent(aug=aug, cpc_objective="predictive")
    rb = NoOffset() if rb_kw is None else make_buffer(aug, **rb_kw)
    state, flat = np.random.get_state()[1].copy(), agent._critic_flat.clone()
    calls = []
    with pytest.raises(ValueError, match="pos_offset"):
        calls = traced(lambda: agent.update(rb, Log(), 1))
    assert calls == [] and np.array_equal(np.random.get_state()[1], state) and torch.equal(agent._critic_flat, flat)
    # n_step > 1 is fine: pos_offset = 1 still gives the stored row's own next_obs
    ok = make_buffer(aug, pos_offset=1, n_step=3, discount=agent.discount)
    assert "curla_pred_loss" in names(traced(lambda: agent.update(ok, Log(), 1)))


def test_a_hand_call_without_the_action_is_refused_before_any_launch():
    agent = make_agent(cpc_objective="predictive")
    x = torch.zeros(4, 9, 28, 34)
    for kw, what in ((dict(), "needs action"), (dict(action=torch.zeros(4, A_ + 1)), "shape"),
                     (dict(action=torch.zeros(3, A_)), "shape")):
        calls = []
        with pytest.raises(ValueError, match=what):
            calls = traced(lambda: agent.update_cpc(x, x, {}, Log(), 1, **kw))
        assert calls == []
    assert "curla_pred_loss" in names(traced(lambda: agent.update_cpc(x, x, {}, Log(), 1, action=torch.zeros(4, A_))))
    # the reference's five-argument call keeps working for the default objective
    plain = make_agent()
    assert "curla_curl_ce" in names(traced(lambda: plain.update_cpc(x, x, {}, Log(), 1)))


def test_a_checkpoint_of_the_other_objective_is_refused_before_anything_is_written(tmp_path):
    plain, on = make_agent(), make_agent(cpc_objective="predictive")
    files = {}
    for name, agent in (("infonce", plain), ("predictive", on)):
        files[name] = str(tmp_path / (name + ".pt"))
        agent.save_checkpoint(files[name], 7)
        agent.save(str(tmp_path), name, 7)
    saved = torch.load(files["predictive"], map_location="cpu", weights_only=False)
    assert saved["cpc_objective"] == "predictive" and saved["predictor_hidden"] == H_
    assert "predictor.2.bias" in saved["curl"] and len(saved["optimizers"]["cpc"]["param_groups"][0]["params"]) == \
        4 + len(list(on.critic.encoder.parameters()))
    assert "cpc_objective" not in torch.load(files["infonce"], map_location="cpu", weights_only=False)
    for agent, other in ((make_agent(seed=2), "predictive"), (make_agent(seed=2, cpc_objective="predictive"), "infonce")):
        before = {k: v.clone() for k, v in agent.CURL.state_dict().items()}
        rng = torch.random.get_rng_state()
        with pytest.raises(ValueError, match="cpc_objective"):
            agent.load_checkpoint(files[other])
        with pytest.raises(ValueError, match="predictor"):
            agent.load(str(tmp_path), other, 7)
        after = agent.CURL.state_dict()
        assert all(torch.equal(before[k], after[k]) for k in before) and torch.equal(rng, torch.random.get_rng_state())
    with pytest.raises(ValueError, match="predictor_hidden"):
        make_agent(cpc_objective="predictive", predictor_hidden=24).load_checkpoint(files["predictive"])
    # the own objective's files load, predictor included
    twin = make_agent(seed=2, cpc_objective="predictive")
    assert twin.load_checkpoint(files["predictive"]) == 7
    assert all(torch.equal(v, twin.CURL.state_dict()[k]) for k, v in on.CURL.state_dict().items())
    twin = make_agent(seed=3, cpc_objective="predictive")
    twin.load(str(tmp_path), "predictive", 7)
    assert torch.equal(twin.CURL.predictor[2].weight, on.CURL.predictor[2].weight)


# -------------------------------------------------------------------------------------------------------- entry point
def test_the_entry_point_is_declared_bound_and_exported():
    import __graft_entry__ as ge
    ge.build()
    from curla_amd import _lib, ops
    name = "curla_pred_loss"
    text = open(os.path.join(ROOT, "include", "curla_hip.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int %s\(([^;]*)\);" % name, text, flags=re.S)
    assert m, "include/curla_hip.h does not declare curla_pred_loss behind a comment"
    assert "Additive: CURLA_ABI_VERSION stays 8" in " ".join(m.group(1).replace("*", " ").split())
    params = [p.strip() for p in m.group(2).split(",")]
    assert len(params) == len(_lib.SIGNATURES[name])
    for p, t in zip(params, _lib.SIGNATURES[name]):
        assert t is (_lib.vp if "*" in p else _lib.c_int), (name, p)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name) and _lib.ABI_VERSION == 8 and callable(ops.pred_loss)
    kernel = open(os.path.join(ROOT, "curla_amd", "csrc", "pred_loss.h")).read()
    assert "pred_loss_kernel" in kernel and "atomic" not in kernel.replace("no atomics", "") and "__shared__" not in kernel
    heads = open(os.path.join(ROOT, "curla_amd", "csrc", "heads.hip")).read()
    assert heads.index('#include "reduce.h"') < heads.index('#include "pred_loss.h"')
    lib = _lib.load()
    a = 4096  # a non-NULL address that is never dereferenced: the checks run on the host, before any launch
    ok = dict(p=a, t=a, B=4, F=50, rows=a, dp=a)
    for bad in (dict(p=None), dict(t=None), dict(rows=None), dict(dp=None), dict(B=0), dict(B=-1), dict(F=0), dict(F=1025)):
        k = {**ok, **bad}
        assert lib.curla_pred_loss(k["p"], k["t"], k["B"], k["F"], k["rows"], None, k["dp"], None) == -1, bad
