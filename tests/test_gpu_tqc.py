"""CurlSacAgent(critic_quantiles=M, critic_drop_quantiles=d) on the MI355X: the two loss kernels alone
against the float64 definition (tests/_tqc_ref.py) -- every (M, d) corner, partly filled workgroups, twin strides in
NaN-filled buffers, rows at the definition's seams, bit-identical reruns --, Critic.forward under user autograd, the
critic and actor phases of an even and an odd update against float64 on the agent's own parameters (both last-layer
forms, both schedules, detach_encoder, LayerNorm + dropout), and whole-agent cases: update graphs, utd_ratio, one-rank
data parallel, clipping, checkpoints, a prioritized buffer."""
import socket

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import _tqc_ref as R
from tests.test_gpu_critic_dropout import _drop_mlp3
from tests.test_gpu_critic_ln import (GUARD, HP, IN_HW, NAN, OUT_HW, NullLogger, _branches, _data, _gather, _grads_of, _ring,
                                      _same_bits, _snap, _state_of, _strided, check, perturb_layer_norms, rnd)
from tests.test_gpu_utd import _build, _lead_step, _state

pytestmark = pytest.mark.gpu

GAMMA = 0.97


def make_agent(M, d=0, hidden=96, seed=0, **kw):
    import curla_amd
    aug = curla_amd.RandomCrop(IN_HW, OUT_HW)
    torch.manual_seed(seed)
    agent = curla_amd.CurlSacAgent((9,) + OUT_HW, (2,), torch.device("cuda"), aug, hidden_dim=hidden,
                                   critic_quantiles=M, critic_drop_quantiles=d, **{**HP, **kw})
    return agent, aug


# ------------------------------------------------------------------------------------------------- 1. the kernels alone
def _loss_inputs(B, M, seed):
    """Atoms a few Huber widths apart, so that |u| falls on both sides of 1 in every row."""
    return dict(theta=1.5 * rnd(2, B, M, seed=seed), z=1.5 * rnd(2, B, M, seed=seed + 1), log_pi=rnd(B, seed=seed + 2),
                reward=rnd(B, seed=seed + 3), not_done=(torch.arange(B) % 3 != 1).float(),
                log_alpha=torch.tensor(np.log(0.3)), discount=GAMMA)


def _run_critic_loss(x, d, pad=(0, 0, 0)):
    """ops.tqc_critic_loss on NaN-filled buffers whose twins lie ``pad`` floats further apart than dense; returns
    (dq [2, B, M], row_loss [B], loss [1]) after checking that nothing outside the tensors was written."""
    from curla_amd import ops
    _, B, M = x["theta"].shape
    sq, st, sd = (B * M + p for p in pad)
    q, _ = _strided(x["theta"], (sq,))
    tq, _ = _strided(x["z"], (st,))
    dq, dmask = _strided(torch.full((2, B, M), 7.0), (sd,))
    row_loss = torch.full((B + GUARD,), NAN, device="cuda")
    loss = torch.full((1 + GUARD,), NAN, device="cuda")
    dev = lambda t: t.float().cuda().contiguous()  # noqa: E731
    ops.tqc_critic_loss(q, sq, tq, st, dev(x["log_pi"]), dev(x["reward"]), dev(x["not_done"]),
                        x["log_alpha"].double().cuda(), x["discount"], B, M, d, dq, sd, row_loss, loss)
    torch.cuda.synchronize()
    assert torch.isnan(dq[~dmask.cuda()]).all(), "dq was written between or behind the twins"
    assert torch.isnan(row_loss[B:]).all() and torch.isnan(loss[1:]).all()
    return _gather(dq, (2, B, M), (sd,)), row_loss[:B].cpu(), loss[:1].cpu()


def _check_critic_loss(tag, x, d, pad=(0, 0, 0)):
    ref = R.critic_loss(d=d, **x)
    dq, row_loss, loss = _run_critic_loss(x, d, pad)
    check(f"tqc critic loss {tag}", loss, ref["loss"].reshape(1))
    check(f"tqc critic row_loss {tag}", row_loss, ref["row_loss"])
    check(f"tqc critic dq {tag}", dq, ref["dq"])
    again = _run_critic_loss(x, d, pad)
    assert all(_same_bits(a, b) for a, b in zip(again, (dq, row_loss, loss))), "a rerun changed bits"
    return dq, row_loss, loss


MD = [(1, 0), (2, 1), (5, 0), (5, 2), (16, 15), (17, 3), (25, 2), (32, 0), (32, 31)]


@pytest.mark.parametrize("M,d", MD)
@pytest.mark.parametrize("B", [1, 3, 5])
def test_critic_loss_kernel(B, M, d):
    """B = 1, 3: less than a workgroup's four rows; 5: a second, partly filled one.  M = 32: every lane live; (16, 15),
    (32, 31): two atoms kept; (1, 0): one atom per network.  Dense once and with three different twin strides."""
    x = _loss_inputs(B, M, seed=100 * B + M)
    dense = _check_critic_loss(f"B{B} M{M} d{d}", x, d)
    strided = _check_critic_loss(f"B{B} M{M} d{d} strided", x, d, pad=(8, 20, 12))
    assert all(_same_bits(a, b) for a, b in zip(dense, strided))


def test_critic_loss_kernel_at_the_seams():
    """Rows built on small integers (reward 0, discount 1, log_pi 0: y = the kept atoms, exactly) so that u is exactly
    0 and +-1 and sits on both sides of 1: all atoms equal; atoms duplicated across the networks; a finished episode
    (not_done = 0: every y = reward); 1e30 among the dropped atoms.  Ties: the kept multiset and hence loss and gradient
    do not depend on their order -- swapping the target networks leaves the same values."""
    M, d = 4, 1
    z = torch.tensor([
        [[2., 2., 2., 2.], [2., 2., 2., 2.]],            # all atoms equal
        [[0., 1., 2., 3.], [0., 1., 2., 3.]],            # duplicated across the two networks
        [[0., 1., 2., 3.], [4., 5., 6., 7.]],            # not_done = 0 (below)
        [[0., 1e30, 2., 3.], [1., 1e30, 2., 0.]],        # huge values among the dropped atoms
        [[0., 1., 1., 2.], [1., 3., 0., 2.]],
    ]).permute(1, 0, 2).contiguous()
    theta = torch.tensor([
        [[2., 1., 3., 0.], [2.5, 1.5, 2.999, 4.]],       # u = 0, +1, -1, +2 | +-0.5, ~-1, -2
        [[0., 1., 2., 3.], [1.001, 0.999, -1., 5.]],
        [[0.5, 1.5, -0.5, 0.], [1., -1., 2., 0.5]],
        [[0., 1., 2., 3.], [3., 2., 1., 0.]],
        [[0., 0., 0., 0.], [1., 1., 1., 1.]],
    ]).permute(1, 0, 2).contiguous()
    B = z.shape[1]
    x = dict(theta=theta, z=z, log_pi=torch.zeros(B), reward=torch.tensor([0., 0., 0.5, 0., 0.]),
             not_done=torch.tensor([1., 1., 0., 1., 1.]), log_alpha=torch.tensor(0.0), discount=1.0)
    ref = R.critic_loss(d=d, **x)
    assert torch.equal(ref["y"][2], torch.full((6,), 0.5, dtype=torch.float64)) and float(ref["y"].max()) == 3.0
    u = ref["y"][:, None, None, :] - theta.double().permute(1, 0, 2)[:, :, :, None]
    assert (u == 0).any() and (u == 1).any() and (u == -1).any() and ((u.abs() > 1) & (u.abs() < 1.01)).any()
    dq, row_loss, loss = _check_critic_loss("seams", x, d, pad=(4, 0, 8))
    swapped, _, _ = _run_critic_loss({**x, "z": z.flip(0).contiguous()}, d)
    assert _same_bits(swapped, dq)
    # d = 0: the huge atoms count (row 3 alone moves, by ~1e30 / 4)
    full = R.critic_loss(d=0, **x)
    _, row0, _ = _run_critic_loss(x, 0)
    check("tqc critic row_loss seams d=0", row0, full["row_loss"])
    assert float(row0[3]) > 1e28 and _same_bits(row0[:3], _run_critic_loss({**x, "z": z.clamp(max=8.0)}, 0)[1][:3])


@pytest.mark.parametrize("B,M,A", [(1, 1, 1), (3, 5, 2), (5, 17, 6), (300, 32, 2), (257, 25, 3)])
def test_actor_loss_kernel(B, M, A):
    """One workgroup of 256 threads: B below, at and above one row per thread; scalars, dq and dlog_alpha against
    float64, twin strides in NaN-filled buffers, reruns bit-identical, dlog_alpha optional."""
    from curla_amd import ops
    theta, log_pi, log_std = 1.5 * rnd(2, B, M, seed=B), rnd(B, seed=B + 1), 0.5 * rnd(B, A, seed=B + 2)
    la = torch.tensor(np.log(0.3))
    ref = R.actor_loss(theta, log_pi, log_std, la, -float(A))

    def run(pad, with_dla=True):
        sq, sd = B * M + pad[0], B * M + pad[1]
        q, _ = _strided(theta, (sq,))
        dq, dmask = _strided(torch.full((2, B, M), 7.0), (sd,))
        sc = torch.full((4 + GUARD,), NAN, device="cuda")
        dla = torch.full((1 + GUARD,), NAN, device="cuda", dtype=torch.float64)
        ops.tqc_actor_loss(q, sq, log_pi.cuda(), log_std.cuda(), A, la.double().cuda(), -float(A), B, M, sc, dq, sd,
                           dla if with_dla else None)
        torch.cuda.synchronize()
        assert torch.isnan(dq[~dmask.cuda()]).all() and torch.isnan(sc[4:]).all() and torch.isnan(dla[1:]).all()
        assert with_dla or torch.isnan(dla).all()
        return sc[:4].cpu(), _gather(dq, (2, B, M), (sd,)), dla[:1].cpu()
    sc, dq, dla = run((0, 0))
    tag = f"B{B} M{M} A{A}"
    for i, name in enumerate(("actor loss", "alpha loss", "entropy", "alpha")):
        check(f"tqc actor {name} {tag}", sc[i:i + 1], ref["scalars"][i:i + 1])
    check(f"tqc actor dq {tag}", dq, ref["dq"])
    check(f"tqc actor dlog_alpha {tag}", dla, ref["dlog_alpha"].reshape(1))
    assert float(dq.min()) == float(dq.max())  # one constant
    for other in (run((0, 0)), run((12, 4))):
        assert all(_same_bits(a, b) for a, b in zip(other, (sc, dq, dla)))
    assert all(_same_bits(a, b) for a, b in zip(run((0, 0), with_dla=False)[:2], (sc, dq)))


def test_entry_points_refuse_what_the_kernels_do_not_take():
    from curla_amd import ops
    from curla_amd._lib import CurlaHipError
    B, M = 4, 5
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    la = torch.zeros((), device="cuda", dtype=torch.float64)
    ok = lambda M=M, d=1, B=B, s=B * M: ops.tqc_critic_loss(z(2, B, 33), s, z(2, B, 33), s, z(B), z(B), z(B), la, 0.99, B,  # noqa: E731
                                                            M, d, z(2, B, 33), s, z(B), z(1))
    ok()
    for bad in (dict(M=0, d=0), dict(M=33, s=B * 33), dict(d=-1), dict(d=5), dict(s=B * M - 1)):
        with pytest.raises(CurlaHipError, match="CURLA_ERR_ARG"):
            ok(**bad)
    with pytest.raises(CurlaHipError, match="CURLA_ERR_ARG"):
        ops.tqc_actor_loss(z(2, B, 33), B * 33, z(B), z(B, 2), 2, la, -2.0, B, 33, z(4), z(2, B, 33), B * 33, None)


# ------------------------------------------------------------------------------- 2. Critic.forward under user autograd
def _float64_trunk(trunk):
    ref = nn.Sequential(*[nn.Linear(m.in_features, m.out_features) if isinstance(m, nn.Linear) else
                          nn.LayerNorm(m.normalized_shape) if isinstance(m, nn.LayerNorm) else nn.ReLU() for m in trunk]).double()
    ref.load_state_dict({k: v.detach().cpu().double() for k, v in trunk.state_dict().items()})
    return ref


@pytest.mark.parametrize("M,ln", [(5, False), (25, True), (25, False), (5, True)])
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


# ------------------------------------------------------------------ 3. the phases against float64, own parameters
class _Adam64:
    """torch.optim.Adam's step in float64 on given gradients, state kept per name across steps."""

    def __init__(self, lr, beta1, beta2=0.999, eps=1e-8):
        self.lr, self.b1, self.b2, self.eps, self.state = lr, beta1, beta2, eps, {}

    def step(self, params, grads):
        out = {}
        for k, g in grads.items():
            m, v, t = self.state.get(k, (torch.zeros_like(g), torch.zeros_like(g), 0))
            m, v, t = self.b1 * m + (1 - self.b1) * g, self.b2 * v + (1 - self.b2) * g * g, t + 1
            self.state[k] = (m, v, t)
            out[k] = params[k] - self.lr / (1 - self.b1 ** t) * m / (v.sqrt() / np.sqrt(1 - self.b2 ** t) + self.eps)
        return out


def _critic_phase64(O, pre, batch, noise, d, detach, layers, relu_branches=None):
    actor, critic, target, log_alpha = pre
    obs, act, rew, nxt, nd = batch
    with torch.no_grad():
        _, pa, log_pi, _ = O.actor_forward(actor, critic, nxt, noise, layers, -10, 2)
        z1, z2 = O.critic_forward(target, nxt, pa, layers)
    c = O._leafify(critic)
    enc = {}
    q1, q2 = O.critic_forward(c, obs, act, layers, detach_encoder=detach, outputs=enc, plan=O._branch_plan(relu_branches))
    out = R.critic_loss(torch.stack([q1, q2]), torch.stack([z1, z2]), log_pi, rew, nd, log_alpha, HP["discount"], d)
    out["loss"].backward()
    return dict(loss=out["loss"].detach(), grads=O._grads(c), enc={k: v.detach() for k, v in enc.items()})


def _actor_phase64(O, actor, critic, log_alpha, obs, noise, target_entropy, layers):
    a = O._leafify(actor)
    la = log_alpha.detach().clone().requires_grad_(True)
    _, pi, log_pi, log_std = O.actor_forward(a, critic, obs, noise, layers, -10, 2, detach_encoder=True)
    q1, q2 = O.critic_forward(critic, obs, pi, layers, detach_encoder=True)
    out = R.actor_loss(torch.stack([q1, q2]), log_pi, log_std, la, target_entropy)
    out["actor_loss"].backward()
    out["alpha_loss"].backward()
    return dict(actor_loss=out["actor_loss"].detach(), alpha_loss=out["alpha_loss"].detach(),
                grads={k: g for k, g in O._grads(a).items() if g is not None}, log_alpha_grad=la.grad.detach().clone())


PHASES = [("four_q", 5, 2), ("four_q", 25, 3), ("two_launches", 5, 0), ("two_launches", 25, 24), ("detach_encoder", 5, 2),
          ("ln_dropout", 25, 3), ("ln_dropout", 5, 1)]


@pytest.mark.parametrize("variant,M,d", PHASES)
def test_phases_vs_float64_on_the_agents_own_parameters(variant, M, d, monkeypatch):
    """Two updates (one even, one odd): the critic loss and every critic gradient, the actor and alpha losses, the
    actor's ten gradients and log_alpha's, all within RTOL of the float64 evaluation -- the oracle's encoder_forward /
    actor_forward / mlp3 on the agent's own parameters produce the atoms, tests/_tqc_ref.py the losses --, and the
    parameters each step leaves within RTOL of a float64 Adam step on the gradients it was handed.  M = 5 takes the last
    layer's small forms, 25 the GEMM forms; ``ln_dropout``: LayerNorm and dropout 0.1, the masks of the reference stream
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
    agent, aug = make_agent(M, d, hidden=96, detach_encoder=detach,
                            **(dict(critic_layer_norm=True, critic_dropout=0.1) if dropq else {}))
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
        tag = f"tqc {variant} M{M} d{d} step{step}"
        rng_c, rng_a = ((0x1234ABCD + step, 7 + 10 * step), (0x1234ABCD + step, (1 << 40) + step)) if dropq else (None, None)
        # ---- critic
        pre = f64((_snap(agent.actor, True), _snap(agent.critic), _snap(agent.critic_target), agent.log_alpha.detach().cpu().clone()))
        agent.update_critic(obs, act, rew, nxt, nd, L, step, noise=nc.cuda(), dropout_rng=rng_c)
        state.update(rng=rng_c, actor=False)
        ref = _critic_phase64(O, pre, batch, nc.double(), d, detach, layers)
        br = _branches(O, ws, ref["enc"], tag + " critic")
        ref = _critic_phase64(O, pre, batch, nc.double(), d, detach, layers, relu_branches=br)
        check(f"{tag} critic loss", L.scalars["train_critic/loss"], ref["loss"])
        want = {k: v for k, v in ref["grads"].items() if v is not None}
        n_q = 20 if dropq else 12
        assert len(taken["critic"]) == len(want) == n_q + (4 if detach else 12)
        for k, v in want.items():
            check(f"{tag} critic grad {k}", taken["critic"][k], v)
            if k.endswith(("trunk.4.weight", "trunk.6.weight")) and v.shape[0] == M:
                assert bool((v.abs().sum(dim=1) > 0).all())  # (every atom's row has a gradient)
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
                                 agent.log_alpha.detach().cpu().clone(), o_obs, na.double(), float(agent.target_entropy), layers)
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


# ------------------------------------------------------------------------------------------------- 4. whole-agent cases
TQC = dict(critic_quantiles=25, critic_drop_quantiles=2)


def _run_updates(steps, G=1, graphs=False, edit=None, dp=None, rb_kw=None, clip=None, hp=None):
    """test_gpu_utd's agent (B = 256, hidden 64, LayerNorm + dropout critics) with quantiles on, through ``steps``."""
    agent, rb, _ = _build(G, rb_kw=rb_kw, clip=clip, hp={**TQC, **(hp or {})})
    if dp is not None:
        agent.enable_data_parallel(single_rank_collectives=True, **dp)
    if graphs:
        agent.enable_update_graphs(rb, warm=1, depth=2)
    L = NullLogger()
    for step in steps:
        if edit is not None and step == edit[0]:
            agent.critic_drop_quantiles = edit[1]
        agent.update(rb, L, step)
    return _state(agent, rb), dict(L.scalars), agent


def _assert_same_state(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("small", [False, True], ids=["M25", "M5"])
def test_update_graphs_replay_bit_identically_and_recapture_on_an_edited_drop_count(small):
    hp = dict(log_interval=10 ** 9, actor_update_freq=2, cpc_update_freq=1, **(dict(critic_quantiles=5) if small else {}))
    steps = list(range(1, 13))
    eager, _, _ = _run_updates(steps, edit=(8, 4), hp=hp)
    graph, _, agent = _run_updates(steps, graphs=True, edit=(8, 4), hp=hp)
    _assert_same_state(eager, graph)
    assert agent._graph_key_at_capture[-1] == ("quantiles", 5 if small else 25, 4)  # captured again after the edit
    assert agent._graphs and all(any(g["graph"] is not None for g in r) for r in agent._graphs.values())
    unedited, _, _ = _run_updates(steps, graphs=True, hp=hp)
    assert not torch.equal(unedited["critic"], graph["critic"])  # (the drop count matters)


@pytest.mark.parametrize("name,kw", [
    ("plain", {}),
    ("n_step, pos_offset", dict(rb_kw=dict(n_step=3, discount=HP["discount"], dedup_frames=True, pos_offset=2))),
    ("max_grad_norm, weight_decay", dict(clip=1e-3, hp=dict(weight_decay=1e-2))),
    ("pixel_sac", dict(hp=dict(pixel_sac=True))),
], ids=lambda v: v if isinstance(v, str) else "")
def test_utd_ratio_3_is_two_critic_only_updates_and_an_ordinary_one(name, kw):
    steps, freq = [4, 5], 2
    kw = dict(kw)
    hp = {**kw.pop("hp", {}), "critic_target_update_freq": freq}
    got, logged, agent = _run_updates(steps, G=3, hp=hp, **kw)
    twin, rb, _ = _build(1, hp={**TQC, **hp}, **kw)
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
    M = 25
    agent, aug = make_agent(M, 2, hidden=96, seed=6)
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


def test_checkpoint_round_trip_and_another_width(tmp_path):
    np.random.seed(5)
    agent, aug = make_agent(25, 2, hidden=96, seed=5)
    rb, L = _ring(aug), NullLogger()
    for step in range(3):
        agent.update(rb, L, step)
    ck = tmp_path / "tqc.pt"
    agent.save_checkpoint(str(ck), 3)
    saved = torch.load(str(ck), map_location="cpu", weights_only=False)
    assert saved["critic_quantiles"] == 25 and saved["critic_drop_quantiles"] == 2
    for step in range(3, 5):
        agent.update(rb, L, step)
    want = _state_of(agent)

    np.random.seed(99)  # a different process state, and another drop count: everything must come from the file
    other, aug2 = make_agent(25, 7, hidden=96, seed=99)
    rb2 = _ring(aug2)
    assert other.load_checkpoint(str(ck)) == 3 and other.critic_drop_quantiles == 2
    for step in range(3, 5):
        other.update(rb2, L, step)
    torch.cuda.synchronize()
    got = _state_of(other)
    assert set(got) == set(want)
    for k, v in want.items():
        assert torch.equal(v, got[k]), k
    for M in (5, 0):  # another width, and no quantiles at all: torch's shape error
        wrong, _ = make_agent(M, hidden=96, seed=5)
        with pytest.raises(RuntimeError, match="size mismatch"):
            wrong.load_checkpoint(str(ck))


def test_a_prioritized_minibatch_is_refused():
    import curla_amd
    agent, aug = make_agent(5, 1, hidden=96)
    rb = _ring(aug, prioritized=True)
    before = agent._critic_flat.clone()
    with pytest.raises(ValueError, match="prioritized"):
        agent.update(rb, NullLogger(), 1)
    assert torch.equal(agent._critic_flat, before)
    plain = _ring(aug)
    agent.update(plain, NullLogger(), 1)  # the same agent goes on with a uniform buffer
    assert not torch.equal(agent._critic_flat, before) and isinstance(rb, curla_amd.ReplayBuffer)
