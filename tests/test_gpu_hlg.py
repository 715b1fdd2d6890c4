"""CurlSacAgent(critic_bins=M, critic_value_range=..., critic_bin_sigma=s) on the MI355X: the two loss
kernels alone against the float64 definition (tests/_hlg_ref.py) -- every bin-count corner, partly filled workgroups,
twin strides in NaN-filled buffers, rows at the definition's seams, two views, bit-identical reruns --, Critic.forward
under user autograd, the critic and actor phases of an even and an odd update against float64 on the agent's own
parameters (both last-layer forms, both schedules, detach_encoder, LayerNorm + dropout), one aug_views = 2 critic phase,
and whole-agent cases: update graphs, utd_ratio, one-rank data parallel, clipping, resets, checkpoints, refusals, the
clip-fraction diagnostic."""
import socket

import numpy as np
import pytest
import torch

from tests import _hlg_ref as R
from tests.test_gpu_critic_dropout import _drop_mlp3
from tests.test_gpu_critic_ln import (GUARD, HP, IN_HW, NAN, OUT_HW, NullLogger, _branches, _data, _gather, _grads_of, _ring,
                                      _same_bits, _snap, _state_of, _strided, perturb_layer_norms, rnd)
from tests.test_gpu_critic_ln import check as _check
from tests.test_gpu_tqc import _Adam64, _assert_same_state, _float64_trunk
from tests.test_gpu_utd import _build, _lead_step, _state
from tests._util import RTOL, rel_err

pytestmark = pytest.mark.gpu

GAMMA = 0.97
RANGE = (-4.0, 6.0)
WORST = {}  # the largest error each group of checks has seen: printed by the module's last test


def check(name, got, ref, tol=RTOL):
    """test_gpu_critic_ln.check, remembering the worst figure of the kernels-alone checks and of the agent-level ones."""
    group = "kernels alone" if name.startswith(("hlg critic", "hlg actor", "views B", "hlg t ")) else "agent level"
    e = rel_err(got, ref)
    if np.isfinite(e) and e > WORST.get(group, (0.0, ""))[0]:
        WORST[group] = (e, name)
    _check(name, got, ref, tol)


def make_agent(M, hidden=96, seed=0, value_range=RANGE, **kw):
    import curla_amd
    aug = curla_amd.RandomCrop(IN_HW, OUT_HW)
    torch.manual_seed(seed)
    agent = curla_amd.CurlSacAgent((9,) + OUT_HW, (2,), torch.device("cuda"), aug, hidden_dim=hidden,
                                   critic_bins=M, critic_value_range=value_range, **{**HP, **kw})
    return agent, aug


# ------------------------------------------------------------------------------------------------- 1. the kernels alone
def _loss_inputs(B, M, seed, bin_sigma=0.75, v=RANGE):
    """Logits a few units apart and rewards that put some targets outside the range, most inside."""
    return dict(q=2.0 * rnd(2, B, M, seed=seed), tq=2.0 * rnd(2, B, M, seed=seed + 1), log_pi=rnd(B, seed=seed + 2),
                reward=3.0 * rnd(B, seed=seed + 3), not_done=(torch.arange(B) % 3 != 1).float(),
                log_alpha=torch.tensor(np.log(0.3)), discount=GAMMA, v_min=v[0], v_max=v[1],
                sigma=bin_sigma * (v[1] - v[0]) / M)


def _run_critic_loss(x, pad=(0, 0, 0), views=False):
    """ops.hlg_critic_loss on NaN-filled buffers whose twins lie ``pad`` floats further apart than dense; returns
    (dq [2, B, M], row_loss [B], loss [1], target_q [B]) after checking that nothing outside the tensors was written."""
    from curla_amd import ops
    _, B, M = x["q"].shape
    sq, st, sd = (B * M + p for p in pad)
    q, _ = _strided(x["q"], (sq,))
    tq, _ = _strided(x["tq"], (st,))
    dq, dmask = _strided(torch.full((2, B, M), 7.0), (sd,))
    row_loss, target_q = (torch.full((B + GUARD,), NAN, device="cuda") for _ in range(2))
    loss = torch.full((1 + GUARD,), NAN, device="cuda")
    dev = lambda t: t.float().cuda().contiguous()  # noqa: E731
    ops.hlg_critic_loss(q, sq, tq, st, dev(x["log_pi"]), dev(x["reward"]), dev(x["not_done"]),
                        x["log_alpha"].double().cuda(), x["discount"], B, M, x["v_min"], x["v_max"], x["sigma"], dq, sd,
                        target_q, row_loss, loss, views=views)
    torch.cuda.synchronize()
    assert torch.isnan(dq[~dmask.cuda()]).all(), "dq was written between or behind the twins"
    assert torch.isnan(row_loss[B:]).all() and torch.isnan(loss[1:]).all() and torch.isnan(target_q[B:]).all()
    return _gather(dq, (2, B, M), (sd,)), row_loss[:B].cpu(), loss[:1].cpu(), target_q[:B].cpu()


def _check_critic_loss(tag, x, pad=(0, 0, 0), views=False):
    ref = R.critic_loss(views=views, **x)
    got = _run_critic_loss(x, pad, views)
    dq, row_loss, loss, target_q = got
    check(f"hlg critic loss {tag}", loss, ref["loss"].reshape(1))
    check(f"hlg critic row_loss {tag}", row_loss, ref["row_loss"])
    check(f"hlg critic dq {tag}", dq, ref["dq"])
    check(f"hlg critic target_q {tag}", target_q, ref["target_q"])
    assert bool(torch.isfinite(dq).all())
    again = _run_critic_loss(x, pad, views)
    assert all(_same_bits(a, b) for a, b in zip(again, got)), "a rerun changed bits"
    return got


@pytest.mark.parametrize("bin_sigma", [0.3, 0.75, 2.0])
@pytest.mark.parametrize("M", [2, 3, 51, 63, 64, 65, 128, 255, 256])
def test_critic_loss_kernel(M, bin_sigma):
    """B = 1, 3: less than a workgroup's four rows; 5: a second, partly filled one.  M = 2, 3: most lanes dead; 63, 64,
    65: around one bin per lane; 128, 255, 256: up to the four bins a lane holds.  Dense once and with three different
    twin strides."""
    for B in (1, 3, 5):
        x = _loss_inputs(B, M, seed=100 * B + M, bin_sigma=bin_sigma)
        dense = _check_critic_loss(f"B{B} M{M} s{bin_sigma}", x)
        strided = _check_critic_loss(f"B{B} M{M} s{bin_sigma} strided", x, pad=(8, 20, 12))
        assert all(_same_bits(a, b) for a, b in zip(dense, strided))


def _one_hot_logits(M, j, height=80.0):
    l = torch.zeros(M)
    l[j] = height
    return l


def test_critic_loss_kernel_at_the_seams():
    """Rows built on exact small numbers: v = (-4, 4), M = 8 (w = 1, edges the integers, centres the halves),
    log_pi = 0, discount = 1 and target logits saturated on one bin (80 among zeros: Q' is that bin's centre to within
    8 e^-80), so y = reward + centre to the last bit."""
    M, v = 8, (-4.0, 4.0)
    hot = lambda j: _one_hot_logits(M, j)  # noqa: E731
    #        Q' = centre of bin     reward  not_done    y
    rows = [(4, 4, -0.5, 1.0),   # 0.5 - 0.5 = 0: exactly on an edge
            (4, 5, 0.0, 1.0),    # min(0.5, 1.5) = 0.5: exactly on a centre
            (0, 1, -3.0, 1.0),   # -3.5 - 3 = -6.5: below v_min
            (7, 7, 2.0, 1.0),    # 3.5 + 2 = 5.5: above v_max
            (7, 6, 1.25, 0.0),   # a finished episode: y = reward
            (2, 3, 0.25, 1.0),
            (5, 5, -4.0, 1.0)]   # 1.5 - 4 = -2.5
    B = len(rows)
    tq = torch.stack([torch.stack([hot(r[0]) for r in rows]), torch.stack([hot(r[1]) for r in rows])])
    q = 2.0 * rnd(2, B, M, seed=7)
    q[0, 5], q[1, 5] = hot(1), hot(6)           # a saturated softmax in both networks
    q[0, 6], q[1, 6] = torch.full((M,), 3.0), torch.zeros(M)  # all logits equal
    x = dict(q=q, tq=tq, log_pi=torch.zeros(B), reward=torch.tensor([r[2] for r in rows]),
             not_done=torch.tensor([r[3] for r in rows]), log_alpha=torch.tensor(0.0), discount=1.0, v_min=v[0],
             v_max=v[1], sigma=0.75)
    ref = R.critic_loss(**x)
    want_y = torch.tensor([0.0, 0.5, -4.0, 4.0, 1.25, -1.25, -2.5])
    assert float((ref["target_q"] - want_y.double()).abs().max()) < 1e-30 + 1e-15
    for pad in ((0, 0, 0), (4, 0, 8)):
        dq, row_loss, loss, target_q = _check_critic_loss("seams", x, pad=pad)
        assert torch.equal(target_q, want_y)      # the bounds, the edge, the centre and the reward, exactly
        assert bool(torch.isfinite(row_loss).all()) and float(row_loss[5]) > 80.0  # finite on a saturated softmax
    # all logits equal: p = 1 / M in both networks, so the two gradients of the row are one
    assert _same_bits(dq[0, 6], dq[1, 6])
    # y on a centre: the histogram is symmetric about bin 4
    t = 1.0 / M - dq[0, 6] * B
    check("hlg t of the all-equal row", t, ref["t"][6])
    sym = (ref["t"][1][4 - 3:4] - ref["t"][1][5:8].flip(0)).abs().max()
    assert float(sym) < 1e-15


@pytest.mark.parametrize("B", [2, 6, 10])
def test_critic_loss_kernel_views(B):
    """Positions p and p + B/2 share the mean of their two targets, bit for bit; loss and dq are over B/2 transitions.
    Two identical views: the non-view kernel's target_q bits, and dq equal to its dq times B / H = 2 (exactly: a power
    of two)."""
    H = B // 2
    for M, bin_sigma in ((5, 0.75), (65, 0.3), (256, 2.0)):
        x = _loss_inputs(B, M, seed=10 * B + M, bin_sigma=bin_sigma)
        dq, row_loss, loss, target_q = _check_critic_loss(f"views B{B} M{M}", x, pad=(4, 12, 8), views=True)
        assert _same_bits(target_q[:H], target_q[H:])
        twice = {k: (torch.cat([v[..., :H, :], v[..., :H, :]], dim=-2) if k in ("q", "tq") else
                     torch.cat([v[:H], v[:H]]) if k in ("log_pi", "reward", "not_done") else v) for k, v in x.items()}
        v_dq, v_rows, v_loss, v_t = _run_critic_loss(twice, views=True)
        p_dq, p_rows, p_loss, p_t = _run_critic_loss(twice)
        assert _same_bits(v_t, p_t) and _same_bits(v_rows, p_rows)
        assert _same_bits(v_dq, p_dq * 2.0)
        check(f"views B{B} M{M} loss of identical views", v_loss, 2.0 * p_loss.double())


def _run_actor_loss(q, log_pi, log_std, la, pad, v=RANGE, with_dla=True):
    from curla_amd import ops
    _, B, M = q.shape
    A = log_std.shape[1]
    sq, sd = B * M + pad[0], B * M + pad[1]
    qd, _ = _strided(q, (sq,))
    dq, dmask = _strided(torch.full((2, B, M), 7.0), (sd,))
    sc = torch.full((4 + GUARD,), NAN, device="cuda")
    row_q = torch.full((B + GUARD,), NAN, device="cuda")
    dla = torch.full((1 + GUARD,), NAN, device="cuda", dtype=torch.float64)
    ops.hlg_actor_loss(qd, sq, log_pi.cuda(), log_std.cuda(), A, la.double().cuda(), -float(A), B, M, v[0], v[1], row_q, sc,
                       dq, sd, dla if with_dla else None)
    torch.cuda.synchronize()
    assert torch.isnan(dq[~dmask.cuda()]).all() and torch.isnan(sc[4:]).all() and torch.isnan(dla[1:]).all()
    assert torch.isnan(row_q[B:]).all() and (with_dla or torch.isnan(dla).all())
    return sc[:4].cpu(), _gather(dq, (2, B, M), (sd,)), dla[:1].cpu(), row_q[:B].cpu()


@pytest.mark.parametrize("B,M,A", [(1, 2, 1), (3, 5, 2), (5, 65, 6), (300, 51, 2), (257, 256, 3)])
def test_actor_loss_kernel(B, M, A):
    """Scalars, dq, min(Q1, Q2) per row and dlog_alpha against float64, twin strides in NaN-filled buffers, reruns
    bit-identical, dlog_alpha optional.  Every third row holds the same logits in both networks: the exact tie, whose
    gradient is split."""
    q, log_pi, log_std = 2.0 * rnd(2, B, M, seed=B), rnd(B, seed=B + 1), 0.5 * rnd(B, A, seed=B + 2)
    ties = torch.arange(B) % 3 == 0
    q[1, ties] = q[0, ties]
    la = torch.tensor(np.log(0.3))
    ref = R.actor_loss(q, log_pi, log_std, la, -float(A), *RANGE)
    sc, dq, dla, row_q = _run_actor_loss(q, log_pi, log_std, la, (0, 0))
    tag = f"B{B} M{M} A{A}"
    for i, name in enumerate(("actor loss", "alpha loss", "entropy", "alpha")):
        check(f"hlg actor {name} {tag}", sc[i:i + 1], ref["scalars"][i:i + 1])
    check(f"hlg actor dq {tag}", dq, ref["dq"])
    check(f"hlg actor row_q {tag}", row_q, torch.minimum(ref["q_values"][0], ref["q_values"][1]))
    check(f"hlg actor dlog_alpha {tag}", dla, ref["dlog_alpha"].reshape(1))
    assert _same_bits(dq[0, ties], dq[1, ties]) and bool(dq[0, ties].any())  # the tie: split, not dropped
    zero = (dq == 0).all(dim=-1)
    assert bool((zero[0] ^ zero[1])[~ties].all())                          # elsewhere exactly one network is left out
    for other in (_run_actor_loss(q, log_pi, log_std, la, (0, 0)), _run_actor_loss(q, log_pi, log_std, la, (12, 4))):
        assert all(_same_bits(a, b) for a, b in zip(other, (sc, dq, dla, row_q)))
    no_dla = _run_actor_loss(q, log_pi, log_std, la, (0, 0), with_dla=False)
    assert _same_bits(no_dla[0], sc) and _same_bits(no_dla[1], dq)


def test_entry_points_refuse_what_the_kernels_do_not_take():
    from curla_amd import ops
    from curla_amd._lib import CurlaHipError
    B, M = 4, 5
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    la = torch.zeros((), device="cuda", dtype=torch.float64)

    def ok(M=M, B=B, s=None, lo=-1.0, hi=1.0, sigma=0.3, views=False):
        s = B * M if s is None else s
        ops.hlg_critic_loss(z(2, B, 257), s, z(2, B, 257), s, z(B), z(B), z(B), la, 0.99, B, M, lo, hi, sigma,
                            z(2, B, 257), s, z(B), z(B), z(1), views=views)
    ok()
    ok(B=4, views=True)
    for bad in (dict(M=1), dict(M=257, s=B * 257), dict(lo=1.0), dict(lo=2.0), dict(hi=float("inf")), dict(sigma=0.0), dict(sigma=-1.0),
                dict(sigma=float("inf")), dict(sigma=float("nan")), dict(s=B * M - 1), dict(B=5, views=True)):
        with pytest.raises(CurlaHipError, match="CURLA_ERR_ARG"):
            ok(**bad)

    def actor(M=M, s=B * M, lo=-1.0):
        ops.hlg_actor_loss(z(2, B, 257), s, z(B), z(B, 2), 2, la, -2.0, B, M, lo, 1.0, z(B), z(4), z(2, B, 257), s, None)
    actor()
    for bad in (dict(M=1), dict(M=257, s=B * 257), dict(lo=1.0), dict(s=B * M - 1)):
        with pytest.raises(CurlaHipError, match="CURLA_ERR_ARG"):
            actor(**bad)


# ------------------------------------------------------------------------------- 2. Critic.forward under user autograd
@pytest.mark.parametrize("M,ln", [(5, False), (51, True), (51, False), (5, True)])
def test_critic_forward_under_user_autograd(M, ln):
    B, A = 5, 2
    agent, _ = make_agent(M, hidden=96, critic_layer_norm=ln)
    if ln:
        perturb_layer_norms(agent)
    critic = agent.critic
    obs = torch.rand((B, 9) + OUT_HW, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)) * 255
    with torch.no_grad():
        z0 = critic.encoder(obs).clone()
        action0 = torch.tanh(rnd(B, A, seed=2)).cuda()
        q1_ng, q2_ng = (q.clone() for q in critic(obs, action0))
    assert q1_ng.shape == q2_ng.shape == (B, M) and critic.outputs["q1"].shape == (B, M)
    z = z0.clone().requires_grad_(True)
    action = action0.clone().requires_grad_(True)
    hook = critic.encoder.register_forward_hook(lambda mod, args, out: z)  # the features as a leaf: d z is observable
    try:
        agent.critic_optimizer.zero_grad()
        q1, q2 = critic(obs, action)
        c1, c2 = rnd(B, M, seed=3).cuda(), rnd(B, M, seed=4).cuda()
        ((q1 * c1).sum() + (q2 * c2).sum()).backward()
    finally:
        hook.remove()
    assert q1.shape == (B, M) and torch.equal(q1.detach(), q1_ng) and torch.equal(q2.detach(), q2_ng)
    z64 = z0.detach().cpu().double().requires_grad_(True)
    a64 = action0.detach().cpu().double().requires_grad_(True)
    refs = [_float64_trunk(critic.Q1.trunk), _float64_trunk(critic.Q2.trunk)]
    xa = torch.cat([z64, a64], 1)
    r1, r2 = refs[0](xa), refs[1](xa)
    ((r1 * c1.cpu().double()).sum() + (r2 * c2.cpu().double()).sum()).backward()
    tag = f"M{M} ln={ln}"
    check(f"autograd q1 {tag}", q1, r1.detach())
    check(f"autograd q2 {tag}", q2, r2.detach())
    check(f"autograd d z {tag}", z.grad, z64.grad)
    check(f"autograd d action {tag}", action.grad, a64.grad)
    n = 0
    for name, q, ref in (("Q1", critic.Q1, refs[0]), ("Q2", critic.Q2, refs[1])):
        got = dict(q.trunk.named_parameters())
        for k, p in ref.named_parameters():
            assert got[k].grad is not None and got[k].grad.shape == p.grad.shape, (name, k)
            check(f"autograd {name}.trunk.{k} grad {tag}", got[k].grad, p.grad)
            n += 1
    assert n == (20 if ln else 12)
    # expected(): torch's expression on the logits against the kernel's Q (the actor kernel's min over the two)
    e1, e2 = critic.expected(q1_ng), critic.expected(q2_ng)
    assert e1.shape == (B, 1)
    check(f"expected() vs float64 {tag}", e1.view(-1), R.expected(r1.detach(), M, *RANGE))
    logits = torch.stack([q1_ng, q2_ng]).cpu()
    row_q = _run_actor_loss(logits, rnd(B, seed=5), rnd(B, A, seed=6), torch.tensor(0.0), (0, 0))[3]
    check(f"expected() vs the kernel's Q {tag}", torch.minimum(e1, e2).view(-1), row_q.double())


# ------------------------------------------------------------------ 3. the phases against float64, own parameters
def _critic_phase64(O, pre, batch, noise, hlg, detach, layers, relu_branches=None, views=False):
    actor, critic, target, log_alpha = pre
    obs, act, rew, nxt, nd = batch
    with torch.no_grad():
        _, pa, log_pi, _ = O.actor_forward(actor, critic, nxt, noise, layers, -10, 2)
        z1, z2 = O.critic_forward(target, nxt, pa, layers)
    c = O._leafify(critic)
    enc = {}
    q1, q2 = O.critic_forward(c, obs, act, layers, detach_encoder=detach, outputs=enc, plan=O._branch_plan(relu_branches))
    out = R.critic_loss(torch.stack([q1, q2]), torch.stack([z1, z2]), log_pi, rew, nd, log_alpha, HP["discount"], *hlg,
                        views=views)
    out["loss"].backward()
    return dict(loss=out["loss"].detach(), grads=O._grads(c), enc={k: v.detach() for k, v in enc.items()},
                target_q=out["target_q"])


def _actor_phase64(O, actor, critic, log_alpha, obs, noise, target_entropy, layers, v):
    a = O._leafify(actor)
    la = log_alpha.detach().clone().requires_grad_(True)
    _, pi, log_pi, log_std = O.actor_forward(a, critic, obs, noise, layers, -10, 2, detach_encoder=True)
    q1, q2 = O.critic_forward(critic, obs, pi, layers, detach_encoder=True)
    out = R.actor_loss(torch.stack([q1, q2]), log_pi, log_std, la, target_entropy, *v)
    out["actor_loss"].backward()
    out["alpha_loss"].backward()
    return dict(actor_loss=out["actor_loss"].detach(), alpha_loss=out["alpha_loss"].detach(),
                grads={k: g for k, g in O._grads(a).items() if g is not None}, log_alpha_grad=la.grad.detach().clone())


PHASES = [("four_q", 5), ("four_q", 51), ("two_launches", 5), ("two_launches", 51), ("detach_encoder", 5),
          ("ln_dropout", 51), ("ln_dropout", 5)]
PHASE_RANGE, PHASE_SIGMA = (-2.0, 3.0), 0.75


@pytest.mark.parametrize("variant,M", PHASES)
def test_phases_vs_float64_on_the_agents_own_parameters(variant, M, monkeypatch):
    """Two updates (one even, one odd): the critic loss and every critic gradient, the actor and alpha losses, the
    actor's ten gradients and log_alpha's, all within RTOL of the float64 evaluation -- the oracle's encoder_forward /
    actor_forward / mlp3 on the agent's own parameters produce the logits, tests/_hlg_ref.py the losses --, and the
    parameters each step leaves within RTOL of a float64 Adam step on the gradients it was handed.  M = 5 takes the last
    layer's small forms, 51 the GEMM forms; ``ln_dropout``: LayerNorm and dropout 0.1, the masks of the reference stream
    at the ``dropout_rng`` both sides are handed."""
    import curla_amd
    from oracle import curla_oracle as O
    dropq = variant == "ln_dropout"
    state = dict(p=0.1, rng=None, actor=False)
    if dropq:
        monkeypatch.setattr(O, "mlp3", _drop_mlp3(O, state))
    monkeypatch.setenv("CURLA_FOUR_Q", "0" if variant == "two_launches" else "1")
    torch.manual_seed(9)
    np.random.seed(9)
    B, layers = 16, 4
    detach = variant == "detach_encoder"
    agent, aug = make_agent(M, hidden=96, detach_encoder=detach, value_range=PHASE_RANGE, critic_bin_sigma=PHASE_SIGMA,
                            **(dict(critic_layer_norm=True, critic_dropout=0.1) if dropq else {}))
    hlg = PHASE_RANGE + (PHASE_SIGMA * (PHASE_RANGE[1] - PHASE_RANGE[0]) / M,)
    assert (agent._twin_outer is None) == (variant == "two_launches")
    if dropq:
        perturb_layer_norms(agent)
    data = _data()
    rb = curla_amd.ReplayBuffer((9,) + IN_HW, (2,), 64, B, torch.device("cuda"), aug)
    rb.add_batch(data["obs"], data["act"], data["rew"], data["nxt"], data["done"])
    L = NullLogger()
    taken = {}

    def keep(name, module, opt, extra=None):
        real = opt.step

        def step():
            taken[name] = _grads_of(module)
            taken[name + ".raw"] = ({n: p.detach().double().cpu() for n, p in module.named_parameters() if p.grad is not None},
                                    {n: p.grad.detach().double().cpu() for n, p in module.named_parameters() if p.grad is not None})
            if extra is not None:
                taken[name + ".extra"] = extra()
            real()
        opt.step = step
    keep("critic", agent.critic, agent.critic_optimizer)
    keep("actor", agent.actor, agent.actor_optimizer,
         lambda: (agent.log_alpha.detach().cpu().clone(), agent.log_alpha.grad.detach().cpu().clone()))
    adam_c, adam_a = _Adam64(HP["critic_lr"], HP["critic_beta"]), _Adam64(HP["actor_lr"], HP["actor_beta"])
    adam_la = _Adam64(HP["alpha_lr"], HP["alpha_beta"])
    f64 = lambda x: O.as_dtype(x, torch.float64)  # noqa: E731
    n_last = 0

    for step in range(2):
        idxs, offs = rb.draw_indices()
        nc, na = torch.randn(B, 2), torch.randn(B, 2)
        obs, act, rew, nxt, nd, _ = rb.sample_cpc_refs(indices=(idxs, offs))
        if variant == "four_q":
            assert obs.pair is not None and obs.pair[1] is nxt and obs.pair[0].B == 2 * B
        crop = lambda src, j: torch.from_numpy(O.random_crop(src[idxs], offs[2 * j], offs[2 * j + 1], OUT_HW)).double()  # noqa: E731
        o_obs, o_nxt = crop(data["obs"], 0), crop(data["nxt"], 1)
        batch = (o_obs, torch.from_numpy(data["act"][idxs]).double(), torch.from_numpy(data["rew"][idxs])[:, None].double(),
                 o_nxt, torch.from_numpy(1.0 - data["done"][idxs].astype(np.float32))[:, None].double())
        ws = agent._ws(B)
        tag = f"hlg {variant} M{M} step{step}"
        rng_c, rng_a = ((0x1234ABCD + step, 7 + 10 * step), (0x1234ABCD + step, (1 << 40) + step)) if dropq else (None, None)
        # ---- critic
        pre = f64((_snap(agent.actor, True), _snap(agent.critic), _snap(agent.critic_target), agent.log_alpha.detach().cpu().clone()))
        agent.update_critic(obs, act, rew, nxt, nd, L, step, noise=nc.cuda(), dropout_rng=rng_c)
        state.update(rng=rng_c, actor=False)
        ref = _critic_phase64(O, pre, batch, nc.double(), hlg, detach, layers)
        br = _branches(O, ws, ref["enc"], tag + " critic")
        ref = _critic_phase64(O, pre, batch, nc.double(), hlg, detach, layers, relu_branches=br)
        check(f"{tag} critic loss", L.scalars["train_critic/loss"], ref["loss"])
        check(f"{tag} target_q", ws.target_q.view(-1), ref["target_q"])
        want = {k: v for k, v in ref["grads"].items() if v is not None}
        n_q = 20 if dropq else 12
        assert len(taken["critic"]) == len(want) == n_q + (4 if detach else 12)
        for k, v in want.items():
            check(f"{tag} critic grad {k}", taken["critic"][k], v)
            if k.endswith(("trunk.4.weight", "trunk.6.weight")) and v.shape[0] == M:
                assert bool((v.abs().sum(dim=1) > 0).all())  # (every bin's row has a gradient)
                n_last += 1
        params, grads = taken["critic.raw"]
        after = adam_c.step(params, grads)
        now = dict(agent.critic.named_parameters())
        for k, v in after.items():
            check(f"{tag} critic post-step {k}", now[k], v)
        if step % 2 == 0 and not detach:
            # ---- actor / alpha (on the critic as its step left it)
            state.update(rng=rng_a, actor=True)
            ref = _actor_phase64(O, f64(_snap(agent.actor, True)), f64(_snap(agent.critic)),
                                 agent.log_alpha.detach().cpu().clone(), o_obs, na.double(), float(agent.target_entropy), layers,
                                 PHASE_RANGE)
            agent.update_actor_and_alpha(obs, L, step, noise=na.cuda(), dropout_rng=rng_a)
            check(f"{tag} actor loss", L.scalars["train_actor/loss"], ref["actor_loss"])
            check(f"{tag} alpha loss", L.scalars["train_alpha/loss"], ref["alpha_loss"])
            got = {k: v for k, v in taken["actor"].items() if ".convs." not in k}
            assert len(got) == len(ref["grads"]) == 10
            for k, v in ref["grads"].items():
                check(f"{tag} actor grad {k}", got[k], v)
            la_before, la_grad = taken["actor.extra"]
            check(f"{tag} log_alpha grad", la_grad, ref["log_alpha_grad"])
            params, grads = ({k: v for k, v in t.items() if ".convs." not in k} for t in taken["actor.raw"])  # (tied: the critic's)
            now = dict(agent.actor.named_parameters())
            for k, v in adam_a.step(params, grads).items():
                check(f"{tag} actor post-step {k}", now[k], v)
            la_after = adam_la.step({"la": la_before.double()}, {"la": la_grad.double()})["la"]
            check(f"{tag} log_alpha post-step", agent.log_alpha.detach(), la_after, 1e-9)
            agent.soft_update_targets()
    assert n_last == 4  # both Q functions' last layers, both steps


@pytest.mark.parametrize("M", [5, 51])
def test_a_views_critic_phase_regresses_on_the_averaged_target(M):
    """aug_views = 2 on both the buffer and the agent: one update_critic against tests/_hlg_ref.critic_loss(views=True)
    on the logits the phase's forward left in the workspace -- the logged loss, target_q (one value per pair) and dq --,
    and every critic gradient against loss.backward() through the differentiable Critic on the same definition."""
    np.random.seed(4)
    B, H = 16, 8
    agent, aug = make_agent(M, hidden=96, value_range=PHASE_RANGE, aug_views=2)
    rb = _ring(aug, aug_views=2)
    obs, act, rew, nxt, nd, _ = rb.sample_cpc()
    assert torch.equal(act[:H], act[H:]) and torch.equal(rew[:H], rew[H:]) and not torch.equal(obs[:H], obs[H:])
    agent.critic_optimizer.step = lambda: None  # gradients before Adam moves the weights
    L = NullLogger()
    agent.update_critic(obs, act, rew, nxt, nd, L, 1)
    ws = agent._ws(B)
    got = _grads_of(agent.critic)
    sigma = 0.75 * (PHASE_RANGE[1] - PHASE_RANGE[0]) / M
    args = (ws.log_pi.cpu(), rew.cpu(), nd.cpu(), agent.log_alpha.detach().cpu(), agent.discount, *PHASE_RANGE, sigma)
    ref = R.critic_loss(ws.q.cpu(), ws.tq.cpu(), *args, views=True)
    tag = f"hlg views M{M}"
    check(f"{tag} loss", L.scalars["train_critic/loss"], ref["loss"])
    check(f"{tag} target_q", ws.target_q.view(-1), ref["target_q"])
    check(f"{tag} dq", ws.dq, ref["dq"])
    assert _same_bits(ws.target_q[:H], ws.target_q[H:])
    own = R.critic_loss(ws.q.cpu(), ws.tq.cpu(), *args)
    assert float((own["target_q"][:H] - own["target_q"][H:]).abs().max()) > 1e-3  # (the two views' own targets differ)
    agent.critic_optimizer.zero_grad()
    q1, q2 = agent.critic(obs, act)
    loss = _views_loss_on_device(torch.stack([q1, q2]), ref["t"].cuda(), H)
    loss.backward()
    want = _grads_of(agent.critic)
    assert set(got) == set(want)
    for k in want:
        check(f"{tag} critic grad {k}", got[k], want[k])


def _views_loss_on_device(logits, t, H):
    """-sum_n sum_b sum_j t log_softmax(logits) / H in float64 on the device, differentiable in the float32 logits."""
    return -(t[None] * torch.log_softmax(logits.double(), dim=-1)).sum() / H


# ------------------------------------------------------------------------------------------------- 4. whole-agent cases
HLG = dict(critic_bins=51, critic_value_range=(-5.0, 5.0))


def _run_updates(steps, G=1, graphs=False, edit=None, dp=None, rb_kw=None, clip=None, hp=None):
    """test_gpu_utd's agent (B = 256, hidden 64, LayerNorm + dropout critics) with bins on, through ``steps``."""
    agent, rb, _ = _build(G, rb_kw=rb_kw, clip=clip, hp={**HLG, **(hp or {})})
    if dp is not None:
        agent.enable_data_parallel(single_rank_collectives=True, **dp)
    if graphs:
        agent.enable_update_graphs(rb, warm=1, depth=2)
    L = NullLogger()
    for step in steps:
        if edit is not None and step == edit[0]:
            agent.critic_bin_sigma = edit[1]
        agent.update(rb, L, step)
    return _state(agent, rb), dict(L.scalars), agent


@pytest.mark.parametrize("small", [False, True], ids=["M51", "M5"])
def test_update_graphs_replay_bit_identically_and_recapture_on_an_edited_sigma(small):
    hp = dict(log_interval=10 ** 9, actor_update_freq=2, cpc_update_freq=1, **(dict(critic_bins=5) if small else {}))
    steps = list(range(1, 13))
    eager, _, _ = _run_updates(steps, edit=(8, 1.5), hp=hp)
    graph, _, agent = _run_updates(steps, graphs=True, edit=(8, 1.5), hp=hp)
    _assert_same_state(eager, graph)
    assert agent._graph_key_at_capture[-1] == ("bins", 5 if small else 51, -5.0, 5.0, 1.5)  # captured again after the edit
    assert agent._graphs and all(any(g["graph"] is not None for g in r) for r in agent._graphs.values())
    unedited, _, _ = _run_updates(steps, graphs=True, hp=hp)
    assert not torch.equal(unedited["critic"], graph["critic"])  # (the smoothing matters)
    assert bool(torch.isfinite(graph["critic"]).all())


@pytest.mark.parametrize("name,kw", [
    ("plain", {}),
    ("n_step, pos_offset", dict(rb_kw=dict(n_step=3, discount=HP["discount"], dedup_frames=True, pos_offset=2))),
    ("max_grad_norm, weight_decay", dict(clip=1e-3, hp=dict(weight_decay=1e-2))),
], ids=lambda v: v if isinstance(v, str) else "")
def test_utd_ratio_3_is_two_critic_only_updates_and_an_ordinary_one(name, kw):
    steps, freq = [4, 5], 2
    kw = dict(kw)
    hp = {**kw.pop("hp", {}), "critic_target_update_freq": freq}
    got, logged, agent = _run_updates(steps, G=3, hp=hp, **kw)
    twin, rb, _ = _build(1, hp={**HLG, **hp}, **kw)
    L = NullLogger()
    for step in steps:
        for _ in range(2):
            twin.update(rb, NullLogger(), _lead_step(step, freq))
        twin.update(rb, L, step)
    _assert_same_state(got, _state(twin, rb))
    assert logged == L.scalars and "train_critic/loss" in logged
    assert float(got["critic_steps"][0]) == 6 and bool(torch.isfinite(got["critic"]).all())
    if name.startswith("max_grad_norm"):
        print("critic gradient norm, clip coefficient:", agent.grad_clip_stats[0].tolist())
        assert float(agent.grad_clip_stats[0, 1]) < 1.0  # (the critic's gradient really was clipped)


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


def test_one_rank_data_parallel_is_the_plain_agent(nccl_world1):
    steps = (3, 4, 5)
    base = _run_updates(steps)
    for mode in (dict(overlap=False, check_every=1), dict(overlap=True, check_every=0)):
        other = _run_updates(steps, dp=mode)
        _assert_same_state(base[0], other[0])
        assert base[1] == other[1], mode


def test_clipped_critic_norm_counts_the_wider_last_layer():
    np.random.seed(6)
    M = 51
    agent, aug = make_agent(M, hidden=96, seed=6)
    agent.set_max_grad_norm(1e-3)
    rb = _ring(aug)
    taken = {}
    real = agent.critic_optimizer.step

    def step():
        taken.update({n: p.grad.detach().double().cpu().clone() for n, p in agent.critic.named_parameters()})
        real()
    agent.critic_optimizer.step = step
    obs, act, rew, nxt, nd, _ = rb.sample_cpc_refs()
    agent.update_critic(obs, act, rew, nxt, nd, NullLogger(), 1)
    del agent.critic_optimizer.step
    assert taken["Q1.trunk.4.weight"].shape == (M, 96) and taken["Q2.trunk.4.bias"].shape == (M,)
    norm = lambda rows: float(torch.sqrt(sum(((g if ".trunk.4." not in n else g[:rows]) ** 2).sum() for n, g in taken.items())))  # noqa: E731
    whole, first_row = norm(M), norm(1)
    logged = float(agent.grad_clip_stats[0, 0])
    print(f"critic gradient norm: logged {logged!r}, float64 {whole!r}, with one row per last layer {first_row!r}")
    assert whole > 1e-3  # (the step was clipped)
    # the logged figure is a float32 (2^-24 relative) of a sum taken in double: 1e-5 relative is generous for "equal",
    # and "not the norm over one row of each last layer" has to clear that same margin, by a factor of ten
    tol = 1e-5 * whole
    assert abs(logged - whole) <= tol and abs(logged - first_row) > 10 * tol


def test_reset_networks_keeps_the_bins_and_later_updates_stay_finite():
    np.random.seed(7)
    M = 51
    agent, aug = make_agent(M, hidden=96, seed=7)
    rb, L = _ring(aug), NullLogger()
    for step in range(2):
        agent.update(rb, L, step)
    before = agent._critic_flat.clone()
    agent.reset_networks()
    for critic in (agent.critic, agent.critic_target):
        assert critic.out_dim == M and critic.Q1.trunk[-1].weight.shape == (M, 96) and critic.Q2.trunk[-1].bias.shape == (M,)
    assert not torch.equal(agent._critic_flat, before)
    for step in range(2, 5):
        agent.update(rb, L, step)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v.float()).all()) for v in _state_of(agent).values())
    assert np.isfinite(L.scalars["train_critic/loss"]) and 0.0 <= agent.target_clip_fraction() <= 1.0


def test_checkpoint_round_trip_and_another_width(tmp_path):
    np.random.seed(5)
    agent, aug = make_agent(51, hidden=96, seed=5, critic_bin_sigma=1.25)
    rb, L = _ring(aug), NullLogger()
    for step in range(3):
        agent.update(rb, L, step)
    ck = tmp_path / "hlg.pt"
    agent.save_checkpoint(str(ck), 3)
    saved = torch.load(str(ck), map_location="cpu", weights_only=False)
    assert saved["critic_bins"] == 51 and saved["critic_value_range"] == RANGE and saved["critic_bin_sigma"] == 1.25
    for step in range(3, 5):
        agent.update(rb, L, step)
    want = _state_of(agent)

    np.random.seed(99)  # a different process state, another range and smoothing: everything must come from the file
    other, aug2 = make_agent(51, hidden=96, seed=99, value_range=(0.0, 1.0), critic_bin_sigma=0.5)
    rb2 = _ring(aug2)
    assert other.load_checkpoint(str(ck)) == 3 and other.critic_value_range == RANGE and other.critic_bin_sigma == 1.25
    for step in range(3, 5):
        other.update(rb2, L, step)
    torch.cuda.synchronize()
    got = _state_of(other)
    assert set(got) == set(want)
    for k, v in want.items():
        assert torch.equal(v, got[k]), k
    wrong, _ = make_agent(5, hidden=96, seed=5)  # another width: torch's shape error
    with pytest.raises(RuntimeError, match="size mismatch"):
        wrong.load_checkpoint(str(ck))


def test_a_prioritized_minibatch_and_quantiles_are_refused():
    import curla_amd
    agent, aug = make_agent(5, hidden=96)
    rb = _ring(aug, prioritized=True)
    before = (agent._critic_flat.clone(), agent._actor_flat.clone(), agent._target_flat.clone())
    with pytest.raises(ValueError, match="prioritized"):
        agent.update(rb, NullLogger(), 1)
    now = (agent._critic_flat, agent._actor_flat, agent._target_flat)
    assert all(torch.equal(a, b) for a, b in zip(now, before))
    plain = _ring(aug)
    agent.update(plain, NullLogger(), 1)  # the same agent goes on with a uniform buffer
    assert not torch.equal(agent._critic_flat, before[0]) and isinstance(rb, curla_amd.ReplayBuffer)
    with pytest.raises(ValueError, match="critic_quantiles"):
        make_agent(5, hidden=96, critic_quantiles=5)


def test_target_clip_fraction_tells_a_range_that_does_not_fit():
    """Rewards are standard normal (the helpers' data) and Q' lies inside the range by construction.  A narrow range far
    above the rewards, (1000, 1001): y <= reward + 0.99 * 1001 + alpha |log_pi| stays below 1000, so every target is
    clamped onto v_min; (-100, 100) holds every target (Q' near 0 for fresh networks) and clamps none."""
    np.random.seed(8)
    far, aug = make_agent(5, hidden=96, seed=8, value_range=(1000.0, 1001.0))
    wide, aug2 = make_agent(5, hidden=96, seed=8, value_range=(-100.0, 100.0))
    L = NullLogger()
    far.update(_ring(aug), L, 1)
    wide.update(_ring(aug2), L, 1)
    assert far.target_clip_fraction() == 1.0 and wide.target_clip_fraction() == 0.0
    assert float(far._ws(16).target_q.min()) == float(far._ws(16).target_q.max()) == 1000.0


def test_report_the_worst_errors_seen():
    """Prints, per group, the largest error against float64 that the checks of this module saw in this run (what
    DESIGN.md 7l quotes); each of them has already been held to its bound."""
    print()
    for group, (e, name) in sorted(WORST.items()):
        print(f"worst {group}: {e:.3e} ({name})")
    assert all(e <= RTOL for e, _ in WORST.values())
