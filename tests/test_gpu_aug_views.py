"""``aug_views = 2`` on the MI355X: the two kernels against the float64 reference of
tests/_aug_views_ref.py (checked on the CPU by tests/test_aug_views_host.py) inside its derived bounds and in their exact
properties, then through the agent -- the critic phase's and the CURL phase's gradients against autograd through the
differentiable modules, graph replays against eager updates bit for bit, and one view against no keyword at all.

Every output buffer is NaN before a launch and every padding region must still be NaN after it."""
import collections

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _aug_views_ref as V
from tests import _loss_head_ref as R
from tests._util import RTOL, load, rel_err, sub
from tests.test_gpu_agent import HP, NullLogger, grads_of, load_state
from tests.test_gpu_graph_aug import _episode, _state

pytestmark = pytest.mark.gpu

GAMMA = 0.99
TAIL = 5  # NaN floats behind every dense output


@pytest.fixture(scope="module")
def ops():
    from curla_amd import ops as o
    return o


def dev(x):
    return torch.as_tensor(x).cuda().contiguous()


def nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def all_nan(t):
    return bool(torch.isnan(t).all())


def bits_equal(a, b):
    """Equal with the NaN of the untouched padding in the same places (a zero's sign is not compared, as elsewhere)."""
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and \
        torch.equal(a.nan_to_num(0.0), b.nan_to_num(0.0))


def within(name, got, ref, bound):
    """|got - ref| <= bound element by element; prints the element with the worst error / bound first."""
    ref = R.f64(ref)
    got, bound = R.f64(got).reshape(ref.shape), R.f64(bound).expand(ref.shape)
    assert bool(torch.isfinite(got).all()), f"{name}: not finite"
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    i = int(ratio.reshape(-1).argmax()) if ratio.numel() else 0
    print(f"{name}: {float(err.reshape(-1)[i]):.3e} (bound {float(bound.reshape(-1)[i]):.3e})")
    assert bool((err <= bound).all()), name


def twin_rows(t, B, stride):
    return torch.stack([t[:B], t[stride:stride + B]])


def twin_gaps_nan(t, B, stride):
    return all_nan(t[B:stride]) and all_nan(t[stride + B:])


# ------------------------------------------------------------------------------- 5. critic_td_loss_views vs float64
def _views_launch(ops, d):
    B, stride = d["B"], d["stride"]
    dd = {k: dev(v) for k, v in d.items() if isinstance(v, torch.Tensor)}
    tgt, loss, dq = nan(B + TAIL), nan(1 + TAIL), nan(2 * stride)
    ops.critic_td_loss_views(dd["q"], dd["tq"], stride, dd["log_pi"], dd["reward"], dd["not_done"], dd["log_alpha"], GAMMA,
                             B, tgt, loss, dq)
    return dd, tgt, loss, dq


def _views_case(ops, B, stride, not_done="mixed"):
    d = R.loss_inputs(B, stride, seed=2000 + B, not_done=not_done)
    _, tgt, loss, dq = _views_launch(ops, d)
    tag = f"B{B} s{stride} nd {not_done}"
    tbar, Sbar = V.views_target(d["tq1"], d["tq2"], d["log_pi"], d["reward"], d["not_done"], d["log_alpha"], GAMMA)
    within(f"views target {tag}", tgt[:B], tbar, V.views_bounds_target(Sbar))
    ref = V.views_critic_loss(d["q1"], d["q2"], tgt[:B].cpu())  # (on the float32 target the kernel wrote)
    within(f"views loss {tag}", loss[:1], ref["loss"].reshape(1), R.scalar_bound(ref["terms"]))
    within(f"views dq {tag}", twin_rows(dq, B, stride), ref["dq"], V.views_bounds_dq(ref))
    assert all_nan(tgt[B:]) and all_nan(loss[1:]) and twin_gaps_nan(dq, B, stride)


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("B", [2, 4, 126, 128, 130, 510, 512, 514, 1030])
def test_critic_td_loss_views_vs_float64(ops, B, pad):
    _views_case(ops, B, B + pad)


@pytest.mark.parametrize("not_done", [0, 1, "mixed"])
def test_critic_td_loss_views_not_done(ops, not_done):
    _views_case(ops, 130, 133, not_done)


# ------------------------------------------------------------------------------------------------ 6. exact properties
@pytest.mark.parametrize("B", [130, 514])
def test_critic_td_loss_views_exact_properties(ops, B):
    stride, H = B + 3, B // 2
    d = R.loss_inputs(B, stride, seed=3000 + B)
    _, tgt, loss, dq = _views_launch(ops, d)
    # (a) the two views of a transition are given the same bits
    assert torch.equal(tgt[:H], tgt[H:B]) and not all_nan(tgt[:B])
    # (c) a rerun writes the same bits
    _, tgt2, loss2, dq2 = _views_launch(ops, d)
    assert bits_equal(tgt, tgt2) and bits_equal(loss, loss2) and bits_equal(dq, dq2)
    # (b) mirrored views: the plain kernel's target; over half as many transitions, twice its dq
    m = V.mirrored(d)
    dd, tgt_v, loss_v, dq_v = _views_launch(ops, m)
    tgt_p, loss_p, dq_p = nan(B + TAIL), nan(1 + TAIL), nan(2 * stride)
    ops.critic_td_loss(dd["q"], dd["tq"], stride, dd["log_pi"], dd["reward"], dd["not_done"], dd["log_alpha"], GAMMA, B,
                       tgt_p, loss_p, dq_p)
    assert bits_equal(tgt_v, tgt_p)
    assert bits_equal(dq_v, 2 * dq_p)  # 1 / (B / 2) == 2 * (1 / B) in float32
    print(f"mirrored B{B}: views loss {float(loss_v[0])!r}, twice the plain loss {2 * float(loss_p[0])!r}")


def test_the_views_entry_points_refuse_an_odd_batch(ops):
    from curla_amd._lib import CurlaHipError
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    la = torch.zeros((), dtype=torch.float64, device="cuda")
    for B in (1, 7):
        with pytest.raises(CurlaHipError):
            ops.critic_td_loss_views(z(2 * B), z(2 * B), B, z(B), z(B), z(B), la, GAMMA, B, z(B), z(1), z(2 * B))
        with pytest.raises(CurlaHipError):
            ops.curl_ce_views(z(B, B), B, B, z(B), z(1), z(B, B))
    with pytest.raises(CurlaHipError):
        ops.critic_td_loss_views(z(16), z(16), 7, z(8), z(8), z(8), la, GAMMA, 8, z(8), z(1), z(16))


# ------------------------------------------------------------------------------------- 7. curl_ce_views vs float64
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("B", [2, 4, 64, 66, 130, 514])
def test_curl_ce_views(ops, B, pad):
    ld = B + pad
    logits = torch.randn(B, B, generator=torch.Generator().manual_seed(B)) * 40.0
    # expf overflows without the max in every row -- and in row B / 2 the largest entry is the partner's
    logits[:, 0] = 250.0 + (torch.arange(B) % 7).float()
    assert float(logits.max(1).values.min()) > 89 and int(logits[B // 2].argmax()) == 0
    ref, bounds = V.curl_ce_views(logits), V.curl_ce_views_bounds(logits)
    lg = torch.full((B, ld), float("nan"))
    lg[:, :B] = logits
    rl, loss, dl = nan(B + TAIL), nan(1 + TAIL), nan(B, ld)
    ops.curl_ce_views(dev(lg), B, ld, rl, loss, dl)
    tag = f"B{B} ld{ld}"
    within(f"curl_ce_views row_loss {tag}", rl[:B], ref["row_loss"], bounds["row_loss"])
    within(f"curl_ce_views dlogits {tag}", dl[:, :B], ref["dlogits"], bounds["dlogits"])
    within(f"curl_ce_views loss {tag}", loss[:1], ref["loss"].reshape(1),
           float(bounds["row_loss"].mean()) + R.scalar_bound(ref["row_loss"]))
    assert all_nan(rl[B:]) and all_nan(loss[1:]) and all_nan(dl[:, B:])
    # the partner entries: exactly zero
    p = V.partner(B)
    assert bool((dl.cpu()[torch.arange(B), p] == 0).all())
    # ... and everything is what the plain kernel gives on logits whose partner entries are -inf
    lm = torch.full((B, ld), float("nan"))
    lm[:, :B] = V.masked(logits)
    rl2, loss2, dl2 = nan(B + TAIL), nan(1 + TAIL), nan(B, ld)
    ops.curl_ce(dev(lm), B, ld, rl2, loss2, dl2)
    assert bits_equal(rl, rl2) and bits_equal(loss, loss2) and bits_equal(dl, dl2)
    if B == 2:  # nothing but the positive is left in a row
        assert float(rl[0]) == 0.0 and float(rl[1]) == 0.0 and not bool(dl[:, :B].any())


# ------------------------------------------------------------------------------------------------- the agent's phases
AGENT_B, IN_HW, OUT_HW = 8, (34, 40), (28, 34)


def _tiny(views=None, B=AGENT_B, seed=5, dedup_frames=False, **agent_kw):
    """The suite's tiny agent (tests/golden/tiny.npz's state) and a RandomCrop buffer of 400 transitions at batch B;
    ``views`` None: both built without the keyword."""
    import curla_amd
    kw = {} if views is None else dict(aug_views=views)
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    np.random.seed(seed)
    device = torch.device("cuda")
    aug = curla_amd.RandomCrop(IN_HW, OUT_HW)
    agent = curla_amd.CurlSacAgent((9,) + OUT_HW, (2,), device, aug, hidden_dim=64, **{**HP, **agent_kw}, **kw)
    g = load("tiny.npz")
    load_state(agent, sub(g, "state0/actor/"), sub(g, "state0/critic/"), sub(g, "state0/critic_target/"), g["state0/W"],
               g["state0/log_alpha"])
    rb = curla_amd.ReplayBuffer((9,) + IN_HW, (2,), 512, B, device, aug, dedup_frames=dedup_frames, **kw)
    rb.add_batch(*_episode(400, 3, IN_HW, 6))
    return agent, rb


def test_the_critic_gradient_is_that_of_the_averaged_target():
    """update_critic of a views agent against loss.backward() through the differentiable Critic on both views' MSEs
    against tbar, taken from the update's workspace; each position's own target gives another gradient."""
    agent, rb = _tiny(views=2)
    B, H = AGENT_B, AGENT_B // 2
    obs, act, rew, nxt, nd, _ = rb.sample_cpc()
    assert torch.equal(act[:H], act[H:]) and torch.equal(rew[:H], rew[H:]) and not torch.equal(obs[:H], obs[H:])
    agent.critic_optimizer.step = lambda: None  # gradients before Adam moves the weights
    L = NullLogger()
    agent.update_critic(obs, act, rew, nxt, nd, L, 1)
    ws = agent._ws(B)
    got = grads_of(agent.critic)
    tbar = ws.target_q.clone()
    assert torch.equal(tbar[:H], tbar[H:])
    # tbar from what the phase's forward left, inside the kernel test's bound
    ref_t, Sbar = V.views_target(ws.tq[0], ws.tq[1], ws.log_pi, rew, nd, float(agent.log_alpha.detach()), agent.discount)
    within("update_critic tbar", tbar.view(-1), ref_t, V.views_bounds_target(Sbar))
    alpha = agent.log_alpha.exp().float()
    own = (rew + nd * np.float32(agent.discount) * (torch.min(ws.tq[0], ws.tq[1]) - alpha * ws.log_pi)).detach().clone()
    assert not torch.equal(own[:H], own[H:])

    def grads(t):
        agent.critic_optimizer.zero_grad()
        q1, q2 = agent.critic(obs, act)
        loss = ((q1 - t) ** 2).mean() * 2 + ((q2 - t) ** 2).mean() * 2
        loss.backward()
        return loss.item(), grads_of(agent.critic)
    loss_v, ref = grads(tbar)
    print(f"views critic loss: logged {L.scalars['train_critic/loss']!r} against {loss_v!r}")
    assert abs(L.scalars["train_critic/loss"] - loss_v) <= RTOL * abs(loss_v)
    _, plain = grads(own)
    assert set(got) == set(ref)
    for k in ref:
        e = rel_err(got[k], ref[k])
        print(f"views critic gradient {k}: rel err {e:.3e}; "
              f"the un-averaged target's is {rel_err(plain[k], ref[k]):.3e} away")
        assert np.isfinite(e) and e <= RTOL, (k, e)
    assert max(rel_err(plain[k], ref[k]) for k in ref) > 1e-2


def test_the_curl_phase_leaves_the_partner_out_of_the_negatives():
    """update_cpc of a views agent against autograd through CURL.compute_logits with the partner column removed."""
    agent, rb = _tiny(views=2)
    B = AGENT_B
    obs, act, rew, nxt, nd, kw = rb.sample_cpc()
    anchor, pos = kw["obs_anchor"], kw["obs_pos"]
    agent._cpc_steps = lambda: None  # gradients before the two Adams move the weights
    L = NullLogger()
    agent.update_cpc(anchor, pos, kw, L, 1)
    got = grads_of(agent.critic.encoder, "encoder.")
    got["W"] = agent.CURL.W.grad.detach().cpu().clone()
    logged = L.scalars["train/curl_loss"]

    def grads(remove):
        agent.encoder_optimizer.zero_grad()
        agent.cpc_optimizer.zero_grad()
        z_a = agent.CURL.encode(anchor)
        z_pos = agent.CURL.encode(pos, ema=True)
        logits = agent.CURL.compute_logits(z_a, z_pos)
        if remove:
            rows, labels = V.without_partner(logits)
            assert rows.shape == (B, B - 1)
        else:
            rows, labels = logits, torch.arange(B, device=logits.device)
        loss = F.cross_entropy(rows, labels)
        loss.backward()
        out = grads_of(agent.critic.encoder, "encoder.")
        out["W"] = agent.CURL.W.grad.detach().cpu().clone()
        return loss.item(), out
    loss_v, ref = grads(True)
    print(f"views curl loss: logged {logged!r} against {loss_v!r}")
    assert abs(logged - loss_v) <= RTOL * abs(loss_v)
    _, plain = grads(False)
    assert set(got) == set(ref)
    for k in ref:
        e = rel_err(got[k], ref[k])
        print(f"views cpc gradient {k}: rel err {e:.3e}; "
              f"with the partner among the negatives {rel_err(plain[k], ref[k]):.3e} away")
        assert np.isfinite(e) and e <= RTOL, (k, e)


# ------------------------------------------------------------------------------------------------------------ 10. graphs
def _run(graphs, steps, **setup):
    """Updates 1 .. steps (log_interval beyond them: none logs) of a views agent; per update the host's kernel calls."""
    import curla_amd.ops as ops_mod
    import curla_amd.optim as optim_mod
    from curla_amd import _lib
    agent, rb = _tiny(views=2, B=16, log_interval=1000, **setup)
    if graphs:
        agent.enable_update_graphs(rb, warm=1, depth=1)
    real_call, counter, per_step = _lib.call, collections.Counter(), []

    def traced(name, *a):
        counter[name] += 1
        return real_call(name, *a)
    for m in (ops_mod, optim_mod):
        m.call = traced
    L = NullLogger()
    try:
        for step in range(1, steps + 1):
            counter.clear()
            agent.update(rb, L, step)
            per_step.append(sum(counter.values()))
        torch.cuda.synchronize()
    finally:
        for m in (ops_mod, optim_mod):
            m.call = real_call
    return _state(agent, rb), per_step, agent


@pytest.mark.parametrize("utd", [1, 2])
@pytest.mark.parametrize("dedup", [False, True], ids=["ring", "dedup_frames"])
def test_graph_replay_of_a_views_agent_is_the_eager_update_bit_for_bit(dedup, utd):
    """Steps 1, 2 warm the odd and the even kind up (utd_ratio = 2: and their critic-only leading kinds), 3, 4 capture,
    5 .. 8 -- four updates, two even and two odd -- replay with no kernel call from the host."""
    eager, calls_e, _ = _run(False, 8, dedup_frames=dedup, utd_ratio=utd)
    graph, calls_g, agent = _run(True, 8, dedup_frames=dedup, utd_ratio=utd)
    assert min(calls_e) > 15 and calls_g[4:] == [0, 0, 0, 0] and min(calls_g[:4]) > 15, (calls_e, calls_g)
    assert len(agent._graphs) == 2 * utd and ("aug_views", 2) in agent._graph_key_at_capture
    assert sorted(eager) == sorted(graph)
    for k in eager:
        assert torch.equal(eager[k], graph[k]), k


# -------------------------------------------------------------------------------------------------------- 11. off is off
def test_one_view_is_the_agent_without_the_keyword_bit_for_bit():
    states = []
    for views in (1, None):
        agent, rb = _tiny(views=views)
        L = NullLogger()
        for step in range(3):
            agent.update(rb, L, step)
        torch.cuda.synchronize()
        states.append((_state(agent, rb), dict(L.scalars)))
    (one, logs_one), (none, logs_none) = states
    assert logs_one == logs_none and sorted(one) == sorted(none)
    for k in one:
        assert torch.equal(one[k], none[k]), k
