"""CurlSacAgent(critic_layer_norm=True, critic_dropout=p) on the MI355X: the two dropout-LayerNorm kernels alone (the
mask read back from the device and compared, element for element, with the NumPy restatement of its stream; values
against float64 with that mask inserted), Critic.forward under user autograd, every phase of an update against the
oracle with the reference masks per pass (both schedules, detach_encoder), update graphs and checkpoints."""
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _dropout_ref as R
from tests._util import RTOL
from tests.test_gpu_critic_ln import (GUARD, HP, IN_HW, NAN, OUT_HW, NullLogger, _branches, _data, _gather, _grads_of, _ring,
                                      _same_bits, _snap, _state_of, _strided, check, perturb_layer_norms, rnd)

pytestmark = pytest.mark.gpu

SEED, COUNTER = 0x1234ABCD5678, 7


def scale_of(p):
    """s = 1.0f / (1.0f - p), as the kernels form it."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def mask_t(seed, counter, tag, nb, B, H, p):
    return torch.from_numpy(R.keep_mask(seed, counter, tag, nb, B, H, p))


def make_agent(hidden=96, seed=0, dropout=0.1, **kw):
    import curla_amd
    aug = curla_amd.RandomCrop(IN_HW, OUT_HW)
    torch.manual_seed(seed)
    agent = curla_amd.CurlSacAgent((9,) + OUT_HW, (2,), torch.device("cuda"), aug, hidden_dim=hidden,
                                   critic_layer_norm=True, critic_dropout=dropout, **{**HP, **kw})
    return agent, aug


# ------------------------------------------------------------------------------------------------- 1. the kernels alone
def _kernels_case(H, B, n2, first, p, seed=SEED, counter=COUNTER, tag0=3):
    """One forward (and, for one group, backward) of the kernels on NaN-filled strided buffers against float64 with the
    reference masks; returns (reference masks [n2, nb, B, H], device output y, device dh or None)."""
    from curla_amd import ops
    nb = 2
    rng = (seed, counter)
    s = scale_of(p)
    sH, sP = B * H + 8, H + 12           # twin strides of the activations / of the parameters
    sH2, sP2 = nb * sH + 24, nb * sP + 4  # group strides
    keep = torch.stack([mask_t(seed, counter, tag0 + 2 * o, nb, B, H, p) for o in range(n2)])
    x = rnd(n2, nb, B, H, seed=H + B) * 1.5 + 0.3
    gamma = 1 + 0.3 * rnd(n2, nb, 1, H, seed=1)
    beta = 0.3 * rnd(n2, nb, 1, H, seed=2)
    x64 = x.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    xd = x64 * keep * s
    mean, var = xd.mean(-1, keepdim=True), xd.var(-1, unbiased=False, keepdim=True)
    rstd_ref = (var + 1e-5).rsqrt()
    xhat_ref = (xd - mean) * rstd_ref
    y_ref = torch.stack([torch.stack([F.relu(F.layer_norm(xd[o, z], (H,), g64[o, z, 0], b64[o, z, 0], 1e-5))
                                      for z in range(nb)]) for o in range(n2)])
    tag = f"H{H} B{B} n2={n2} first={first} p={p}"
    outer = None if n2 == 1 else (n2, sH2, sP2)
    gm, _ = _strided(gamma, (sP2, sP))
    bt, _ = _strided(beta, (sP2, sP))
    # ---- the forward's mask, read back: a constant input leaves s or 0 in front of the LayerNorm, so with gamma = 1,
    # beta = 0 a row that has both kinds comes out positive exactly where it was kept (a uniform row: constant)
    ones, _ = _strided(torch.ones(n2, nb, B, H), (sH2, sH))
    g1, _ = _strided(torch.ones(n2, nb, 1, H), (sP2, sP))
    b0, _ = _strided(torch.zeros(n2, nb, 1, H), (sP2, sP))
    ops.mlp_drop_ln_relu_fwd(ones, sH, g1, b0, sP, B, H, p, rng, tag0, nb, outer=outer)
    y1 = _gather(ones, (n2, nb, B, H), (sH2, sH))
    mixed = keep.any(-1, keepdim=True) & ~keep.all(-1, keepdim=True)
    assert torch.equal((y1 > 0) & mixed, keep & mixed), "the forward's mask is not the reference's"
    uniform = y1[~mixed.expand_as(y1)].view(-1, H)
    assert (uniform == uniform[:, :1]).all()
    # ---- forward
    h, hmask = _strided(x, (sH2, sH))
    before = h.clone()
    ns = n2 - first
    xhat = torch.full((ns * nb * B * H + GUARD,), NAN, device="cuda")
    rstd = torch.full((ns * nb * B + GUARD,), NAN, device="cuda")
    ops.mlp_drop_ln_relu_fwd(h, sH, gm, bt, sP, B, H, p, rng, tag0, nb, xhat=xhat, rstd=rstd, outer=outer, save_first=first)
    torch.cuda.synchronize()
    assert _same_bits(h[~hmask.cuda()], before[~hmask.cuda()]), "the forward wrote between or behind the rows"
    assert torch.isnan(xhat[-GUARD:]).all() and torch.isnan(rstd[-GUARD:]).all()
    y = _gather(h, (n2, nb, B, H), (sH2, sH))
    check(f"critic dropout fwd h {tag}", y, y_ref.detach())
    check(f"critic dropout fwd xhat {tag}", xhat[:-GUARD].view(ns, nb, B, H), xhat_ref.detach()[first:])
    check(f"critic dropout fwd rstd {tag}", rstd[:-GUARD].view(ns, nb, B), rstd_ref.detach()[first:, :, :, 0])
    # a no-grad pass (NULL xhat / rstd) and a rerun compute the same bits
    h2, _ = _strided(x, (sH2, sH))
    ops.mlp_drop_ln_relu_fwd(h2, sH, gm, bt, sP, B, H, p, rng, tag0, nb, outer=outer)
    assert _same_bits(h2, h)
    if n2 > 1:
        return keep, y, None
    # ---- backward (one group: the backward has no outer level)
    up = rnd(nb, B, H, seed=7)
    y_ref[0].backward(up.double())
    dh_in = up * (y[0] > 0)              # what the layer behind hands over: masked by the post-LayerNorm activation
    assert ((y[0] > 0) == (y_ref[0].detach() > 0)).all()
    sD, sG = B * H + 20, H + 4
    refs = (("dpre", x64.grad[0]), ("dgamma", g64.grad[0]), ("dbeta", b64.grad[0]),
            ("linear bias", x64.grad[0].sum(1, keepdim=True)))

    def run(params):
        dh, dmask = _strided(dh_in, (sD,))
        was = dh.clone()
        outs = [torch.full(((nb - 1) * sG + H + GUARD,), NAN, device="cuda") for _ in range(3)]
        part = torch.full((ops.mlp_ln_partial_floats(B, H, nb) + GUARD,), NAN, device="cuda")
        kw = dict(partial=part, dgamma=outs[0], dbeta=outs[1], dbias=outs[2], sg=sG) if params else {}
        ops.mlp_drop_ln_bwd(dh, sD, xhat, rstd, gm, sP, B, H, p, rng, tag0, nb, **kw)
        torch.cuda.synchronize()
        assert _same_bits(dh[~dmask.cuda()], was[~dmask.cuda()]), "the backward wrote between or behind the rows"
        assert torch.isnan(part[-GUARD:]).all() and (params or torch.isnan(part).all())
        for o in outs:
            touched = ~torch.isnan(o.cpu())
            want = torch.zeros_like(touched)
            if params:
                for z in range(nb):
                    want[z * sG:z * sG + H] = True
            assert torch.equal(touched, want), "a parameter gradient was written outside its [H] slots"
        return dh, outs

    dh, outs = run(True)
    got = [_gather(dh, (nb, B, H), (sD,))] + [_gather(o, (nb, 1, H), (sG,)) for o in outs]
    # the backward's mask, read back: the Linear-output gradient is an exact zero where, and only where, it was dropped.
    # (Only where: except in a row with ONE kept element, whose LayerNorm output does not depend on that element's
    # size, so that its true gradient is ~0 and the computed one rounding noise that may come out as a zero.)
    lone = keep[0].sum(-1, keepdim=True) == 1
    assert not (got[0] != 0)[~keep[0]].any(), "the backward left a gradient where the reference drops"
    assert torch.equal((got[0] != 0) | lone, keep[0] | lone), "the backward's mask is not the reference's"
    assert not lone.any() or p > 0.9
    for (n, r), g in zip(refs, got):
        check(f"critic dropout bwd {n} {tag}", g, r)
    dh_again, outs_again = run(True)
    assert _same_bits(dh_again, dh) and all(_same_bits(a, b) for a, b in zip(outs_again, outs))
    dh_only, _ = run(False)              # the actor phase's form: the data gradient alone, the same bits
    assert _same_bits(dh_only, dh)
    return keep, y, got[0]


KERNEL_CASES = [(H, B, 1, 0, p) for H in (64, 100, 513, 1024) for B in (3, 5) for p in (0.1, 0.5)] + \
    [(100, 5, 2, 0, 0.1), (100, 5, 2, 1, 0.5)]


@pytest.mark.parametrize("H,B,n2,first,p", KERNEL_CASES)
def test_kernels_alone(H, B, n2, first, p):
    """The lane widths, row counts, strides and group cases of test_gpu_critic_ln.py's kernel test, each with the
    mask: NF = 1 (one Philox evaluation per lane, one word used), 2 (two words), 16 with one feature in the ninth slot
    (H = 513: three chunks of 256, the last nearly empty) and 16 full (four evaluations, all words)."""
    keep, _, _ = _kernels_case(H, B, n2, first, p)
    assert not keep.all() and keep.any()


def test_kernels_alone_with_a_row_dropped_entirely():
    """p = 0.97, H = 64: a stream position, found with the NumPy reference, at which a whole row is dropped.  Its
    LayerNorm sees zeros -- mean 0, variance 0, rstd = 1 / sqrt(eps) -- so it must leave relu(beta), finite, and a
    Linear-output gradient of exact zeros."""
    H, B, p, tag0 = 64, 5, 0.97, 3
    counter = next(c for c in range(64) if not R.keep_mask(SEED, c, tag0, 2, B, H, p).any(-1).all())
    keep, y, dh = _kernels_case(H, B, 1, 0, p, counter=counter, tag0=tag0)
    gone = ~keep[0].any(-1)              # [nb, B]
    assert gone.any() and keep.any() and not keep.all(), "the case is not the one this test is about"
    beta = 0.3 * rnd(1, 2, 1, H, seed=2)
    want = torch.relu(beta[0]).expand(2, B, H)
    assert torch.isfinite(y).all() and torch.isfinite(dh).all()
    assert torch.equal(y[0][gone], want[gone])
    assert (dh[gone] == 0).all()


# ------------------------------------------------------------------------------- 2. Critic.forward under user autograd
def _masked_trunk64(trunk, xa, masks, s):
    """A Q function's trunk in float64 on ``xa`` with the keep masks of its two hidden layers inserted; returns (q, the
    float64 leaves by state-dict key)."""
    p = {k: v.detach().cpu().double().requires_grad_(True) for k, v in trunk.state_dict().items()}
    h = xa
    for lin, ln, m in ((0, 1, masks[0]), (3, 4, masks[1])):
        h = F.linear(h, p[f"{lin}.weight"], p[f"{lin}.bias"]) * m * s
        h = F.relu(F.layer_norm(h, (h.size(-1),), p[f"{ln}.weight"], p[f"{ln}.bias"], 1e-5))
    return F.linear(h, p["6.weight"], p["6.bias"]), p


def test_critic_forward_under_user_autograd():
    B, A, H, p = 5, 2, 96, 0.1
    agent, _ = make_agent(hidden=H, dropout=p)
    perturb_layer_norms(agent)
    critic = agent.critic
    assert critic.training and critic.dropout == p
    obs = torch.rand((B, 9) + OUT_HW, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)) * 255
    rng = (SEED, COUNTER)
    with torch.no_grad():
        z0 = critic.encoder(obs).clone()
        action0 = torch.tanh(rnd(B, A, seed=2)).cuda()
        q1_ng, q2_ng = (q.clone() for q in critic(obs, action0, dropout_rng=rng))
    z = z0.clone().requires_grad_(True)
    action = action0.clone().requires_grad_(True)
    hook = critic.encoder.register_forward_hook(lambda mod, args, out: z)  # the features as a leaf: d z is observable
    try:
        agent.critic_optimizer.zero_grad()
        q1, q2 = critic(obs, action, dropout_rng=rng)
        c1, c2 = rnd(B, 1, seed=3).cuda(), rnd(B, 1, seed=4).cuda()
        ((q1 * c1).sum() + (q2 * c2).sum()).backward()
    finally:
        hook.remove()
    assert torch.equal(q1.detach(), q1_ng) and torch.equal(q2.detach(), q2_ng)  # same launches, same masks, same bits
    z64 = z0.detach().cpu().double().requires_grad_(True)
    a64 = action0.detach().cpu().double().requires_grad_(True)
    xa = torch.cat([z64, a64], 1)
    masks = [mask_t(*rng, tag, 2, B, H, p) for tag in (7, 8)]  # a forward() call: pass 3
    (r1, p1), (r2, p2) = (_masked_trunk64(q.trunk, xa, [m[i] for m in masks], scale_of(p))
                          for i, q in enumerate((critic.Q1, critic.Q2)))
    ((r1 * c1.cpu().double()).sum() + (r2 * c2.cpu().double()).sum()).backward()
    check("dropout autograd q1", q1, r1.detach())
    check("dropout autograd q2", q2, r2.detach())
    check("dropout autograd d z", z.grad, z64.grad)
    check("dropout autograd d action", action.grad, a64.grad)
    n = 0
    for tag, q, ref in (("Q1", critic.Q1, p1), ("Q2", critic.Q2, p2)):
        got = dict(q.trunk.named_parameters())
        for k, leaf in ref.items():
            assert got[k].grad is not None, (tag, k)
            check(f"dropout autograd {tag}.trunk.{k} grad", got[k].grad, leaf.grad)
            n += 1
    assert n == 20
    # another stream position: other masks, other values; no position given: one counter of the device generator per call
    with torch.no_grad():
        assert not torch.equal(critic(obs, action0, dropout_rng=(SEED, COUNTER + 1))[0], q1_ng)
        gen = torch.cuda.default_generators[torch.cuda.current_device()]
        off = gen.get_offset()
        got = critic(obs, action0)[0].clone()
        assert gen.get_offset() == off + 4
        assert torch.equal(got, critic(obs, action0, dropout_rng=(gen.initial_seed(), off // 4))[0])
    # eval mode: the deterministic Q, bit for bit a LayerNorm critic's on the same parameters
    plain, _ = make_agent(hidden=H, dropout=0.0)
    plain.critic.load_state_dict(critic.state_dict())
    critic.eval()
    try:
        with torch.no_grad():
            off = gen.get_offset()
            e1, e2 = (q.clone() for q in critic(obs, action0))
            assert gen.get_offset() == off
            w1, w2 = plain.critic(obs, action0)
        assert torch.equal(e1, w1) and torch.equal(e2, w2)
        assert not torch.equal(e1, q1_ng)
    finally:
        critic.train()


# --------------------------------------------------------------- 3. the phases against the oracle, own parameters
def _drop_mlp3(O, state):
    """oracle.mlp3 with Linear - Dropout - LayerNorm - ReLU hidden layers in the Q functions' trunks, the keep masks
    those of the reference stream: ``state`` = dict(p, rng, actor) names the stream position and whether the oracle is
    in its actor phase (pass 2); within the critic phase the target's pass runs under no_grad (pass 0), the critic's
    does not (pass 1).  The actor's trunk is the oracle's own."""
    real = O.mlp3

    def mlp3(p, prefix, x, plan=None, hidden=None):
        if prefix not in ("Q1.trunk.", "Q2.trunk."):
            return real(p, prefix, x, plan, hidden)
        ps = 2 if state["actor"] else 1 if torch.is_grad_enabled() else 0
        z, (B, H), pd = int(prefix[1]) - 1, (x.size(0), p[f"{prefix}0.bias"].numel()), state["p"]
        m = [mask_t(*state["rng"], 1 + 2 * ps + layer, 2, B, H, pd)[z].to(x.dtype) * scale_of(pd) for layer in (0, 1)]
        ln = lambda h, i: F.layer_norm(h, (h.size(-1),), p[f"{prefix}{i}.weight"], p[f"{prefix}{i}.bias"], 1e-5)  # noqa: E731
        h1 = F.linear(x, p[f"{prefix}0.weight"], p[f"{prefix}0.bias"]) * m[0]
        h2 = F.linear(O._relu(ln(h1, 1), plan, (prefix, 0)), p[f"{prefix}3.weight"], p[f"{prefix}3.bias"]) * m[1]
        if hidden is not None:
            hidden += [h1.detach(), h2.detach()]
        return F.linear(O._relu(ln(h2, 4), plan, (prefix, 1)), p[f"{prefix}6.weight"], p[f"{prefix}6.bias"])
    return mlp3


def _run_phases(variant, monkeypatch, oracle=True):
    """Two updates (one even, one odd), every phase given its stream position; with ``oracle`` each is held to RTOL
    against the oracle's phase functions on the agent's own parameters.  Returns what the phases left, for bit
    comparisons between the schedules."""
    import curla_amd
    from oracle import curla_oracle as O
    pd = 0.1
    state = dict(p=pd, rng=None, actor=False)
    monkeypatch.setattr(O, "mlp3", _drop_mlp3(O, state))
    monkeypatch.setenv("CURLA_FOUR_Q", "0" if variant == "two_launches" else "1")
    torch.manual_seed(9)
    np.random.seed(9)
    B, layers = 16, 4
    detach = variant == "detach_encoder"
    agent, aug = make_agent(hidden=96, dropout=pd, detach_encoder=detach)
    assert (agent._twin_outer is None) == (variant == "two_launches")
    perturb_layer_norms(agent)
    d = _data()
    rb = curla_amd.ReplayBuffer((9,) + IN_HW, (2,), 64, B, torch.device("cuda"), aug)
    rb.add_batch(d["obs"], d["act"], d["rew"], d["nxt"], d["done"])
    L = NullLogger()
    kw = dict(num_layers=layers, log_std_min=-10, log_std_max=2)
    grads, left = {}, {}

    def keep(name, module, opt, extra=None):
        real = opt.step

        def step():
            grads[name] = _grads_of(module)
            if extra is not None:
                grads[name + ".extra"] = extra()
            real()
        opt.step = step
    keep("critic", agent.critic, agent.critic_optimizer)
    keep("actor", agent.actor, agent.actor_optimizer, lambda: agent.log_alpha.grad.detach().cpu().clone())

    for step in range(2):
        idxs, offs = rb.draw_indices()
        nc, na = torch.randn(B, 2), torch.randn(B, 2)
        obs, act, rew, nxt, nd, _ = rb.sample_cpc_refs(indices=(idxs, offs))
        if variant == "four_q":  # (obs and next_obs as one handle: the schedule with the four Q functions in one launch)
            assert obs.pair is not None and obs.pair[1] is nxt and obs.pair[0].B == 2 * B
        crop = lambda src, j: torch.from_numpy(O.random_crop(src[idxs], offs[2 * j], offs[2 * j + 1], OUT_HW)).float()  # noqa: E731
        o_obs, o_nxt = crop(d["obs"], 0), crop(d["nxt"], 1)
        o_act, o_rew = torch.from_numpy(d["act"][idxs]), torch.from_numpy(d["rew"][idxs])[:, None]
        o_nd = torch.from_numpy(1.0 - d["done"][idxs].astype(np.float32))[:, None]
        ws = agent._ws(B)
        tag = f"critic-dropout {variant} step{step}"
        rng_c, rng_a = (SEED + step, COUNTER + 10 * step), (SEED + step, (1 << 40) + step)  # (a counter above 2^32 too)
        # ---- critic
        pre = (_snap(agent.actor, True), _snap(agent.critic), _snap(agent.critic_target), agent.log_alpha.detach().cpu().clone())
        agent.update_critic(obs, act, rew, nxt, nd, L, step, noise=nc.cuda(), dropout_rng=rng_c)
        left[f"critic loss {step}"] = torch.tensor(L.scalars["train_critic/loss"])
        left.update({f"critic grad {step} {k}": v for k, v in grads["critic"].items()})
        if oracle:
            state.update(rng=rng_c, actor=False)
            args = (*pre, o_obs, o_act, o_rew, o_nxt, o_nd, nc)
            ref = O.critic_phase(*args, discount=0.99, detach_encoder=detach, **kw)
            br = _branches(O, ws, ref["enc"], tag + " critic")
            ref = O.critic_phase(*args, discount=0.99, detach_encoder=detach, relu_branches=br, **kw)
            check(f"{tag} critic loss", L.scalars["train_critic/loss"], ref["loss"])
            want = {k: v for k, v in ref["grads"].items() if v is not None}
            assert len(grads["critic"]) == len(want) == (24 if detach else 32)
            for k, v in want.items():
                check(f"{tag} critic grad {k}", grads["critic"][k], v)
        if step % 2 == 0 and not detach:
            # ---- actor / alpha (on the critic as its step left it)
            if oracle:
                state.update(rng=rng_a, actor=True)
                ref = O.actor_phase(_snap(agent.actor, True), _snap(agent.critic), agent.log_alpha.detach().cpu().clone(),
                                    o_obs, na, target_entropy=float(agent.target_entropy), **kw)
            agent.update_actor_and_alpha(obs, L, step, noise=na.cuda(), dropout_rng=rng_a)
            got = {k: v for k, v in grads["actor"].items() if ".convs." not in k}
            left[f"actor loss {step}"] = torch.tensor(L.scalars["train_actor/loss"])
            left.update({f"actor grad {step} {k}": v for k, v in got.items()})
            if oracle:
                check(f"{tag} actor loss", L.scalars["train_actor/loss"], ref["actor_loss"])
                check(f"{tag} alpha loss", L.scalars["train_alpha/loss"], ref["alpha_loss"])
                assert len(got) == len(ref["grads"]) == 10
                for k, v in ref["grads"].items():
                    check(f"{tag} actor grad {k}", got[k], v)
                check(f"{tag} log_alpha grad", grads["actor.extra"], ref["log_alpha_grad"])
            agent.soft_update_targets()
    return left


@pytest.mark.parametrize("variant", ["four_q", "two_launches", "detach_encoder"])
def test_phases_vs_oracle_on_the_agents_own_parameters(variant, monkeypatch):
    """test_gpu_critic_ln.py's phase test with the masks: the oracle's Q trunks drop under the reference stream -- the
    target twins under tags 1 / 2, the critic twins under 3 / 4, the actor phase's under 5 / 6 -- and the critic loss,
    all 32 critic gradients, the actor and alpha losses, the actor's 10 gradients and log_alpha's stay within RTOL."""
    assert RTOL == 1e-4
    _run_phases(variant, monkeypatch)


def test_the_two_schedules_draw_the_same_masks_and_leave_the_same_bits(monkeypatch):
    """The four-Q launch numbers its rows within each group and moves the tag by 2 per group, so it draws what the
    two-launch schedule draws."""
    a = _run_phases("four_q", monkeypatch, oracle=False)
    b = _run_phases("two_launches", monkeypatch, oracle=False)
    assert set(a) == set(b) and len(a) > 40
    for k, v in a.items():
        assert _same_bits(v, b[k]), k


# ---------------------------------------------------------------------------------------------------- 4. update graphs
def _assert_xhat_shows_mask(xhat, keep, what):
    """A dropped element enters the LayerNorm as 0, so within a row all dropped elements share ONE xhat value
    (-mean * rstd) and, the kept ones being spread, no kept element has it."""
    xhat = xhat.cpu()
    n = 0
    for z in range(xhat.shape[0]):
        for r in range(xhat.shape[1]):
            gone = xhat[z, r][~keep[z, r]]
            if gone.numel():
                assert (gone == gone[0]).all() and not (xhat[z, r][keep[z, r]] == gone[0]).any(), (what, z, r)
                n += gone.numel()
    assert n > 0, what


def test_update_graphs_replay_a_dropout_agent_bit_identically():
    """Eager and replayed runs from the same seeds agree bit for bit over warm-up, capture and replays of both kinds;
    the replayed updates' masks (read from the xhat the critic's first LayerNorm saved last) are the reference's at
    the stream positions the device generator stood at, so two consecutive updates draw different ones; editing
    ``agent.critic_dropout`` drops the graphs, and the re-captured ones drop with the new p."""
    B, A, H = 16, 2, 96

    def run(graphs):
        np.random.seed(11)
        torch.manual_seed(11)
        torch.cuda.manual_seed_all(11)
        agent, aug = make_agent(hidden=H, seed=11, dropout=0.1, log_interval=100)
        perturb_layer_norms(agent)
        rb = _ring(aug)
        if graphs:
            agent.enable_update_graphs(rb, warm=1)
        L = NullLogger()
        gen = torch.cuda.default_generators[torch.cuda.current_device()]
        masks = []
        for step in range(1, 11):
            if step == 7:
                agent.critic_dropout = 0.2
                if graphs:
                    assert agent._graph_key_at_capture is not None and 0.1 in agent._graph_key_at_capture
            off = gen.get_offset()
            agent.update(rb, L, step)
            torch.cuda.synchronize()
            # the pass that saved last: the actor phase's (tag 5, the second draw's counter) on an even step, the
            # critic's (tag 3, the first draw's) on an odd one
            even = step % 2 == 0
            counter = off // 4 + ((B * A + 3) // 4 if even else 0)
            keep = mask_t(gen.initial_seed(), counter, 5 if even else 3, 2, B, H, agent.critic_dropout)
            _assert_xhat_shows_mask(agent._ws(B).q_xhat1, keep, f"step {step}")
            masks.append(keep)
            if graphs and step in (6, 10):  # (captured at 3 / 4 and again at 9 / 10)
                assert len(agent._graphs) == 2 and all(st["graph"] is not None for ring in agent._graphs.values() for st in ring)
        assert all(not torch.equal(a, b) for a, b in zip(masks[:-2], masks[2:]))  # consecutive updates of one kind
        if graphs:
            assert 0.2 in agent._graph_key_at_capture and 0.1 not in agent._graph_key_at_capture
        return _state_of(agent)
    eager, graphed = run(False), run(True)
    assert set(eager) == set(graphed) and len(eager) > 20
    for k, v in eager.items():
        assert torch.equal(v, graphed[k]), k


# ------------------------------------------------------------------------------------------------------ 5. persistence
def test_checkpoint_round_trip_resumes_the_masks(tmp_path):
    np.random.seed(5)
    agent, aug = make_agent(hidden=96, seed=5)
    rb, L = _ring(aug), NullLogger()
    for step in range(3):
        agent.update(rb, L, step)
    ck = tmp_path / "drop.pt"
    agent.save_checkpoint(str(ck), 3)
    for step in range(3, 5):
        agent.update(rb, L, step)
    want = _state_of(agent)

    np.random.seed(99)  # a different process state: everything, the masks' stream position included, comes from the file
    torch.cuda.manual_seed_all(99)
    other, aug2 = make_agent(hidden=96, seed=99)
    rb2 = _ring(aug2)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)   # (same p: nothing to warn about)
        assert other.load_checkpoint(str(ck)) == 3
    for step in range(3, 5):
        other.update(rb2, L, step)
    torch.cuda.synchronize()
    got = _state_of(other)
    assert set(got) == set(want)
    for k, v in want.items():
        assert torch.equal(v, got[k]), k
    # a LayerNorm-only file loads into a dropout agent, which keeps its p
    plain, _ = make_agent(hidden=96, seed=5, dropout=0.0)
    plain_ck = tmp_path / "ln.pt"
    plain.save_checkpoint(str(plain_ck), 0)
    with pytest.warns(RuntimeWarning, match="critic_dropout"):
        assert other.load_checkpoint(str(plain_ck)) == 0
    assert other.critic_dropout == 0.1
    for k, v in plain.critic.state_dict().items():
        assert torch.equal(v, other.critic.state_dict()[k]), k
    other.update(rb2, L, 0)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v).all()) for v in _state_of(other).values())
