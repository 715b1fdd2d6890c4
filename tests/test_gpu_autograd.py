"""Autograd through the HIP encoder, actor, critic and CURL head (curla_amd/autograd.py).

1. the reference's update written as plain user autograd code on the modules, against the golden gradients;
2. unit gradients of every differentiable forward against a float64 torch restatement (NCHW conv2d / linear /
   layer_norm / squash), differentiating along the device's ReLU branches (an activation within rounding of zero may
   fall on either side in fp32 and fp64; values are untouched);
3. the observation-gradient kernel against torch.nn.grad.conv2d_input, and a saliency call;
4. no behaviour change: grad-mode forwards equal no-grad forwards bit for bit, forwards keep their own buffers, double
   backward raises;
5. gradients land in the flat buffers: FlatAdam after a user backward equals torch.optim.Adam, unused parameters stay
   None and untouched, and a checkpointed agent's next update() is bit-identical to the original's."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from tests._util import RTOL, load, rel_err, sub
from tests.test_gpu_agent import HP, _t, _tiny_agent, grads_of

pytestmark = pytest.mark.gpu


def check(name, got, ref, tol=RTOL):
    e = rel_err(got, ref)
    assert np.isfinite(e) and e <= tol, f"{name}: rel err {e:.3e} > {tol:.1e}"


@pytest.fixture(scope="module")
def tiny():
    return load("tiny.npz")


def _agent(obs_shape, B=8, A=2, hidden=64, filters=32, seed=0, **kw):
    import curla_amd
    c, h, w = obs_shape
    aug = curla_amd.RandomCrop((h + 4, w + 4), (h, w))
    torch.manual_seed(seed)
    hp = dict(HP, num_filters=filters, **kw)
    return curla_amd.CurlSacAgent(obs_shape, (A,), torch.device("cuda"), aug, hidden_dim=hidden, **hp)


# ---------------------------------------------------------------------------------------------- 1. the reference update
def test_reference_update_as_user_autograd(tiny):
    g = tiny
    agent, _ = _tiny_agent(g)
    obs, nxt, pos = (_t(g[k]).float() for k in ("batch/obs", "batch/next_obs", "batch/pos"))
    act, rew, nd = _t(g["batch/action"]), _t(g["batch/reward"]), _t(g["batch/not_done"])
    B = obs.shape[0]

    # critic: TD target under no_grad, twin MSE, backward
    with torch.no_grad():
        _, pi_n, logpi_n, _ = agent.actor(nxt, noise=_t(g["noise/critic"]))
        tq1, tq2 = agent.critic_target(nxt, pi_n)
        target = rew + nd * 0.99 * (torch.min(tq1, tq2) - agent.alpha.detach() * logpi_n)
    q1, q2 = agent.critic(obs, act)
    critic_loss = Fn.mse_loss(q1, target) + Fn.mse_loss(q2, target)
    check("critic loss", critic_loss.item(), g["scalar/train_critic/loss"])
    agent.critic_optimizer.zero_grad()
    critic_loss.backward()
    got, ref = grads_of(agent.critic), sub(g, "critic/grad/")
    assert set(got) == set(ref)
    for k in ref:
        check(f"critic grad {k}", got[k], ref[k])

    # actor + alpha, encoder detached, from the critic after its Adam step
    agent.critic.load_state_dict(sub(g, "critic_after/"))
    agent.actor_optimizer.zero_grad()
    _, pi, log_pi, log_std = agent.actor(obs, detach_encoder=True, noise=_t(g["noise/actor"]))
    aq1, aq2 = agent.critic(obs, pi, detach_encoder=True)
    actor_loss = (agent.alpha.detach() * log_pi - torch.min(aq1, aq2)).mean()
    check("actor loss", actor_loss.item(), g["scalar/train_actor/loss"])
    actor_loss.backward()
    got, ref = grads_of(agent.actor), sub(g, "actor/grad/")
    for k in ref:
        check(f"actor grad {k}", got[k], ref[k])
    for m in agent.actor.encoder.convs:  # tied to the critic's, which the critic's backward above filled
        assert m.weight.grad is not None
    agent.log_alpha_optimizer.zero_grad()
    alpha_loss = (agent.alpha * (-log_pi - agent.target_entropy).detach()).mean()
    check("alpha loss", alpha_loss.item(), g["scalar/train_alpha/loss"])
    alpha_loss.backward()
    check("log_alpha grad", agent.log_alpha.grad.cpu(), g["alpha/grad/log_alpha"])

    # CURL: anchors through the online encoder, positives through the target encoder (ema)
    agent.critic_target.load_state_dict(sub(g, "target_after/"))
    agent.encoder_optimizer.zero_grad()
    agent.cpc_optimizer.zero_grad()
    z_a = agent.CURL.encode(obs)
    z_pos = agent.CURL.encode(pos, ema=True)
    assert not z_pos.requires_grad
    logits = agent.CURL.compute_logits(z_a, z_pos)
    curl_loss = Fn.cross_entropy(logits, torch.arange(B, device=logits.device))
    check("curl loss", curl_loss.item(), g["scalar/train/curl_loss"])
    curl_loss.backward()
    got = grads_of(agent.critic.encoder, "encoder.")
    got["W"] = agent.CURL.W.grad.cpu()
    ref = sub(g, "cpc/grad/")
    for k in ref:
        check(f"cpc grad {k}", got[k], ref[k])


# ---------------------------------------------------------------------------------------------- 2. float64 restatement
def _leaves(params):
    return [p.detach().double().requires_grad_(True) for p in params]


def _ref_encoder(enc, x, detach, masks, P):
    """float64 encoder.py:77-110 with the device's ReLU branches; P = leaves of autograd.encoder_params(enc) with
    fc.weight in the reference's (c, y, x) column order."""
    h = x / 255.0
    L = enc.num_layers
    for i in range(L):
        h = Fn.conv2d(h, P[2 * i], P[2 * i + 1], stride=2 if i == 0 else 1) * masks[i]
    h = h.flatten(1)
    if detach:
        h = h.detach()
    y = Fn.layer_norm(Fn.linear(h, P[2 * L], P[2 * L + 1]), (enc.feature_dim,), P[2 * L + 2], P[2 * L + 3], enc.ln.eps)
    return y if enc.output_logits else torch.tanh(y)


def _enc_leaves(enc):
    from curla_amd import autograd
    ps = list(autograd.encoder_params(enc))
    L = enc.num_layers
    ps[2 * L] = enc.fc.to_reference_layout(enc.fc.weight)
    return _leaves(ps)


def _enc_grads(enc):
    from curla_amd import autograd
    ps = autograd.encoder_params(enc)
    out = [p.grad for p in ps]
    L = enc.num_layers
    if out[2 * L] is not None:
        out[2 * L] = enc.fc.to_reference_layout(out[2 * L])
    return out


def _masks(enc):
    return [(enc.outputs[f"conv{i + 1}"] > 0).double() for i in range(enc.num_layers)]


def _zero_grads(params):
    for p in params:
        p.grad = None


GEOMS = [(9, 76, 76), (9, 76, 135), (12, 76, 76), (3, 84, 84)]
CASES = [(s, B, 32) for s in GEOMS for B in (8, 512)] + [((9, 76, 76), 8, 16), ((9, 76, 76), 512, 16)]


@pytest.mark.parametrize("shape,B,filters", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
@pytest.mark.parametrize("detach", [False, True])
def test_encoder_grads_vs_float64(shape, B, filters, detach):
    from curla_amd import autograd
    agent = _agent(shape, filters=filters)
    enc = agent.critic.encoder
    enc.record_outputs = True
    gen = torch.Generator(device="cuda").manual_seed(B)
    x = (torch.rand((B,) + shape, device="cuda", generator=gen) * 255).requires_grad_(True)
    params = autograd.encoder_params(enc)
    _zero_grads(params)
    z = enc(x, detach=detach)
    dz = torch.randn(z.shape, device="cuda", generator=gen)
    z.backward(dz)
    P = _enc_leaves(enc)
    x64 = x.detach().double().requires_grad_(True)
    zr = _ref_encoder(enc, x64, detach, _masks(enc), P)
    check("z", z, zr)
    zr.backward(dz.double())
    got = _enc_grads(enc)
    for i, (a, r) in enumerate(zip(got, P)):
        if detach and i < 2 * enc.num_layers:
            assert a is None, f"conv parameter {i} received a gradient through a detached encoder"
        else:
            check(f"param {i}", a, r.grad)
    if detach:
        assert x.grad is None
    else:
        check("d obs", x.grad, x64.grad)


@pytest.mark.parametrize("B", [8, 512])
def test_encoder_tanh_output_and_forward_conv(B):
    """output_logits=False (tanh after the LayerNorm) and forward_conv's (c, y, x) features."""
    from curla_amd import autograd
    from curla_amd.encoder import CNNEncoder
    shape = (9, 76, 76)
    agent = _agent(shape)
    enc = CNNEncoder(shape, 50, 4, 32, output_logits=False).cuda().to_kernel_layout()
    enc.load_state_dict(agent.critic.encoder.state_dict())
    enc.record_outputs = True
    gen = torch.Generator(device="cuda").manual_seed(7)
    x = (torch.rand((B,) + shape, device="cuda", generator=gen) * 255).requires_grad_(True)
    z = enc(x)
    dz = torch.randn(z.shape, device="cuda", generator=gen)
    z.backward(dz)
    P = _enc_leaves(enc)
    x64 = x.detach().double().requires_grad_(True)
    zr = _ref_encoder(enc, x64, False, _masks(enc), P)
    check("tanh z", z, zr)
    zr.backward(dz.double())
    for i, (a, r) in enumerate(zip(_enc_grads(enc), P)):
        check(f"tanh param {i}", a, r.grad)
    check("tanh d obs", x.grad, x64.grad)

    # forward_conv
    _zero_grads(autograd.encoder_params(enc))
    x.grad = None
    h = enc.forward_conv(x)
    dh = torch.randn(h.shape, device="cuda", generator=gen)
    h.backward(dh)
    P = _enc_leaves(enc)
    x64 = x.detach().double().requires_grad_(True)
    hr = x64 / 255.0
    masks = _masks(enc)
    for i in range(4):
        hr = Fn.conv2d(hr, P[2 * i], P[2 * i + 1], stride=2 if i == 0 else 1) * masks[i]
    hr = hr.flatten(1)
    check("forward_conv", h, hr)
    hr.backward(dh.double())
    for i in range(8):
        check(f"forward_conv param {i}", _enc_grads(enc)[i], P[i].grad)
    check("forward_conv d obs", x.grad, x64.grad)


def _ref_head(out, noise, lo, hi, A):
    """curl_sac.py:20-35,85-108 in float64 (noise a constant)."""
    mu, log_std = out.chunk(2, dim=-1)
    log_std = torch.tanh(log_std)
    log_std = lo + 0.5 * (hi - lo) * (log_std + 1)
    pi = mu + noise * log_std.exp()
    log_pi = (-0.5 * noise.pow(2) - log_std).sum(-1, keepdim=True) - 0.5 * math.log(2 * math.pi) * A
    mu, pi = torch.tanh(mu), torch.tanh(pi)
    log_pi = log_pi - torch.log(Fn.relu(1 - pi.pow(2)) + 1e-6).sum(-1, keepdim=True)
    return mu, pi, log_pi, log_std


def _mlp_ref(x, P, m1, m2):
    h1 = Fn.linear(x, P[0], P[1]) * m1
    h2 = Fn.linear(h1, P[2], P[3]) * m2
    return Fn.linear(h2, P[4], P[5])


@pytest.mark.parametrize("B", [8, 512])
@pytest.mark.parametrize("compute_pi,compute_log_pi", [(True, True), (True, False), (False, True), (False, False)])
def test_actor_grads_vs_float64(B, compute_pi, compute_log_pi):
    agent = _agent((9, 28, 34), A=3, hidden=64)
    actor = agent.actor
    gen = torch.Generator(device="cuda").manual_seed(B + 1)
    # (features of half the LayerNorm's spread: a squashed pi within fp32 rounding of +-1 makes log(1 - pi^2 + 1e-6)
    # -- the reference's formula -- ill-conditioned in ANY fp32 evaluation)
    z = (0.5 * torch.randn((B, 50), device="cuda", generator=gen)).requires_grad_(True)
    noise = torch.randn((B, 3), device="cuda", generator=gen)
    trunk = [t for i in (0, 2, 4) for t in (actor.trunk[i].weight, actor.trunk[i].bias)]
    _zero_grads(trunk)
    # the trunk alone, through a features leaf (actor.encoder is exercised by the encoder tests)
    from curla_amd import autograd
    outs = autograd.actor_forward(actor, z, compute_pi, compute_log_pi, noise)
    node = outs[0].grad_fn
    m1, m2 = (node.h1 > 0).double(), (node.h2 > 0).double()
    ups = [None if o is None else torch.randn(o.shape, device="cuda", generator=gen) for o in outs]
    torch.autograd.backward([o for o in outs if o is not None], [u for u in ups if u is not None])
    P = _leaves(trunk)
    z64 = z.detach().double().requires_grad_(True)
    ref = _ref_head(_mlp_ref(z64, P, m1, m2), noise.double(), actor.log_std_min, actor.log_std_max, 3)
    total = 0
    for name, o, r, u in zip(("mu", "pi", "log_pi", "log_std"), outs, ref, ups):
        if name in ("pi", "log_pi") and not compute_pi or name == "log_pi" and not compute_log_pi:
            assert o is None
            continue
        check(name, o, r)
        total = total + (r * u.double()).sum()
    total.backward()
    check("d z", z.grad, z64.grad)
    for i, (p, r) in enumerate(zip(trunk, P)):
        check(f"trunk param {i}", p.grad, r.grad)


@pytest.mark.parametrize("B", [8, 512])
def test_critic_grads_vs_float64(B):
    from curla_amd import autograd
    agent = _agent((9, 28, 34), A=3, hidden=64)
    critic = agent.critic
    gen = torch.Generator(device="cuda").manual_seed(B + 2)
    z = torch.randn((B, 50), device="cuda", generator=gen).requires_grad_(True)
    a = torch.rand((B, 3), device="cuda", generator=gen).mul(2).sub(1).requires_grad_(True)
    qp = autograd._q_params(critic)
    _zero_grads(qp)
    q1, q2 = autograd.critic_forward(critic, z, a)
    node = q1.grad_fn
    masks = (node.h1 > 0).double(), (node.h2 > 0).double()
    u1, u2 = torch.randn(q1.shape, device="cuda", generator=gen), torch.randn(q2.shape, device="cuda", generator=gen)
    torch.autograd.backward([q1, q2], [u1, u2])
    P = _leaves(qp)
    z64, a64 = z.detach().double().requires_grad_(True), a.detach().double().requires_grad_(True)
    xa = torch.cat([z64, a64], 1)
    r1 = _mlp_ref(xa, P[:6], masks[0][0], masks[1][0])
    r2 = _mlp_ref(xa, P[6:], masks[0][1], masks[1][1])
    check("q1", q1, r1)
    check("q2", q2, r2)
    ((r1 * u1.double()).sum() + (r2 * u2.double()).sum()).backward()
    check("d z", z.grad, z64.grad)
    check("d action", a.grad, a64.grad)
    for i, (p, r) in enumerate(zip(qp, P)):
        check(f"Q param {i}", p.grad, r.grad)


@pytest.mark.parametrize("B", [8, 512])
def test_curl_logits_grads_vs_float64(B):
    agent = _agent((9, 28, 34))
    gen = torch.Generator(device="cuda").manual_seed(B + 3)
    za = torch.randn((B, 50), device="cuda", generator=gen).requires_grad_(True)
    zp = torch.randn((B, 50), device="cuda", generator=gen).requires_grad_(True)
    W = agent.CURL.W
    W.grad = None
    lg = agent.CURL.compute_logits(za, zp)
    u = torch.randn(lg.shape, device="cuda", generator=gen)
    lg.backward(u)
    za64, zp64 = za.detach().double().requires_grad_(True), zp.detach().double().requires_grad_(True)
    W64 = W.detach().double().requires_grad_(True)
    r = za64 @ (W64 @ zp64.T)
    r = r - torch.max(r, 1)[0][:, None]
    check("logits", lg, r)
    (r * u.double()).sum().backward()
    check("d z_a", za.grad, za64.grad)
    check("d z_pos", zp.grad, zp64.grad)
    check("d W", W.grad, W64.grad)


def test_tied_convs_accumulate_actor_and_critic():
    agent = _agent((9, 76, 76))
    gen = torch.Generator(device="cuda").manual_seed(11)
    x = torch.rand((8, 9, 76, 76), device="cuda", generator=gen) * 255
    a = torch.rand((8, 2), device="cuda", generator=gen)
    noise = torch.randn((8, 2), device="cuda", generator=gen)
    conv = agent.critic.encoder.convs[1].weight
    assert conv is agent.actor.encoder.convs[1].weight

    def run(actor, critic):
        conv.grad = None
        loss = 0
        if actor:
            loss = loss + agent.actor(x, noise=noise)[1].sum()
        if critic:
            loss = loss + agent.critic(x, a)[0].sum()
        loss.backward()
        return conv.grad.clone()
    ga, gc, both = run(True, False), run(False, True), run(True, True)
    check("tied conv grad = actor's + critic's", both, ga + gc, 1e-5)


# ---------------------------------------------------------------------------------------------- 3. obs gradient
@pytest.mark.parametrize("shape,B,filters", CASES + [((9, 77, 135), 8, 32), ((3, 85, 83), 8, 32), ((6, 31, 40), 16, 64),
                                                     ((12, 33, 33), 8, 16)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_conv1_dgrad_vs_conv2d_input(shape, B, filters):
    from curla_amd import ops
    C, H, W = shape
    Ho, Wo = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    gen = torch.Generator(device="cuda").manual_seed(H * W + B)
    g = torch.randn((B, Ho, Wo, filters), device="cuda", generator=gen)
    w = torch.randn((filters, C, 3, 3), device="cuda", generator=gen)
    dobs = torch.full((B, C, H, W), float("nan"), device="cuda")
    ops.conv1_dgrad(g, w, dobs)
    ref = torch.nn.grad.conv2d_input((B, C, H, W), w.double(), g.double().permute(0, 3, 1, 2), stride=2) / 255.0
    check("dobs", dobs, ref)
    assert torch.isfinite(dobs).all()
    # rows / columns no output reaches are exactly zero
    if H % 2 == 0:
        assert (dobs[:, :, H - 1] == 0).all()
    if W % 2 == 0:
        assert (dobs[:, :, :, W - 1] == 0).all()


def test_saliency():
    agent = _agent((9, 76, 76))
    agent.critic.encoder.record_outputs = True
    gen = torch.Generator(device="cuda").manual_seed(5)
    obs = torch.rand((8, 9, 76, 76), device="cuda", generator=gen) * 255
    act = torch.rand((8, 2), device="cuda", generator=gen)
    x = obs.clone().requires_grad_()
    q1, _ = agent.critic(x, act)
    (sal,) = torch.autograd.grad(q1.sum(), x)
    assert sal.shape == obs.shape and sal.abs().max() > 0
    # the float64 restatement, along the device's branches
    enc = agent.critic.encoder
    P = _enc_leaves(enc)
    x64 = obs.double().requires_grad_()
    z = _ref_encoder(enc, x64, False, _masks(enc), P)
    qp = [p.detach().double() for p in (agent.critic.Q1.trunk[i].weight if j == 0 else agent.critic.Q1.trunk[i].bias
                                         for i in (0, 2, 4) for j in (0, 1))]
    xa = torch.cat([z, act.double()], 1)
    h1 = Fn.relu(Fn.linear(xa, qp[0], qp[1]))
    h2 = Fn.relu(Fn.linear(h1, qp[2], qp[3]))
    (ref,) = torch.autograd.grad(Fn.linear(h2, qp[4], qp[5]).sum(), x64)
    check("saliency", sal, ref, 1e-3)


# ---------------------------------------------------------------------------------------------- 4. no behaviour change
def test_grad_mode_forwards_bit_identical_and_independent():
    agent = _agent((9, 76, 76))
    gen = torch.Generator(device="cuda").manual_seed(3)
    x1, x2 = (torch.rand((16, 9, 76, 76), device="cuda", generator=gen) * 255 for _ in range(2))
    a = torch.rand((16, 2), device="cuda", generator=gen)
    noise = torch.randn((16, 2), device="cuda", generator=gen)

    def fwd():
        outs = list(agent.actor(x1, noise=noise))
        outs += list(agent.critic(x1, a))
        outs += [agent.critic.encoder(x1), agent.critic.encoder.forward_conv(x1)]
        za = agent.CURL.encode(x1)
        outs.append(agent.CURL.compute_logits(za, agent.CURL.encode(x2, ema=True)))
        return outs
    with torch.no_grad():
        ref = [o.clone() for o in fwd()]
    got = fwd()
    assert all(o.requires_grad for o in got)
    for i, (o, r) in enumerate(zip(got, ref)):
        assert torch.equal(o.detach(), r), f"output {i} differs between grad and no_grad mode"

    # two graph-building forwards, one backward of their sum == the sum of the two separate backwards
    enc = agent.critic.encoder
    params = list(enc.parameters())

    def grads(*xs):
        _zero_grads(params)
        sum(enc(x).pow(2).sum() for x in xs).backward()
        return [p.grad.clone() for p in params]
    g1, g2, g12 = grads(x1), grads(x2), grads(x1, x2)
    for i, (a_, b_, c_) in enumerate(zip(g1, g2, g12)):
        check(f"two forwards, one backward: param {i}", c_, a_ + b_, 1e-5)

    # double backward raises
    x = x1.clone().requires_grad_()
    q1, _ = agent.critic(x, a)
    with pytest.raises(RuntimeError, match="double backward"):
        torch.autograd.grad(q1.sum(), x, create_graph=True)
    z = agent.critic.encoder(x)
    with pytest.raises(RuntimeError, match="double backward"):
        torch.autograd.grad(z.pow(2).sum(), x, create_graph=True)


# ---------------------------------------------------------------------------------------------- 5. flat buffers
def test_flat_buffers_adam_and_checkpoint(tmp_path):
    import curla_amd
    shape = (9, 28, 34)
    agent = _agent(shape, seed=1)
    gen = torch.Generator(device="cuda").manual_seed(9)
    obs = torch.rand((8,) + shape, device="cuda", generator=gen) * 255
    act = torch.rand((8, 2), device="cuda", generator=gen)
    target = torch.randn((8, 1), device="cuda", generator=gen)

    # actor optimizer over fc / ln / trunk; with detach_encoder=True fc and ln of the ACTOR get gradients, the critic
    # step below leaves the critic's convs without one
    opt = agent.critic_optimizer
    params = list(agent.critic.parameters())
    before = [p.detach().clone() for p in params]
    host = [p.detach().clone().requires_grad_(True) for p in params]
    host_opt = torch.optim.Adam(host, lr=1e-3, betas=(0.9, 0.999))
    conv_ids = {id(t) for m in agent.critic.encoder.convs for t in (m.weight, m.bias)}
    for step in range(2):
        opt.zero_grad()
        assert all(p.grad is None for p in params)
        q1, q2 = agent.critic(obs, act, detach_encoder=True)
        (Fn.mse_loss(q1, target) + Fn.mse_loss(q2, target)).backward()
        base = agent._critic_gflat.data_ptr()
        for p in params:
            if id(p) in conv_ids:
                assert p.grad is None
            else:
                assert p.grad is not None and base <= p.grad.data_ptr() < base + 4 * agent._critic_gflat.numel()
                assert p.grad.data_ptr() == dict(agent._grad_views)[p].data_ptr()
        for h, p in zip(host, params):
            h.grad = None if p.grad is None else p.grad.detach().clone()
        opt.step()
        host_opt.step()
    for i, (p, h, b) in enumerate(zip(params, host, before)):
        if id(p) in conv_ids:
            assert torch.equal(p.detach(), b), f"param {i} moved without a gradient"
            assert len(opt.state[p]) == 0 and len(host_opt.state[h]) == 0
        else:
            check(f"FlatAdam vs torch Adam, param {i}", p.detach(), h.detach(), 1e-5)

    # the agent still trains: checkpoint it, restore into a second agent, one update() each on the same ring / noise
    path = str(tmp_path / "ck.pt")
    agent.save_checkpoint(path, 7)
    other = _agent(shape, seed=2)
    other.load_checkpoint(path)
    rb = curla_amd.ReplayBuffer((9, 32, 38), (2,), 64, 8, torch.device("cuda"), agent.augmentor)
    rs = np.random.RandomState(0)
    n = 40
    rb.add_batch(rs.randint(0, 256, (n, 9, 32, 38), dtype=np.uint8), rs.uniform(-1, 1, (n, 2)).astype(np.float32),
                 rs.randn(n).astype(np.float32), rs.randint(0, 256, (n, 9, 32, 38), dtype=np.uint8), np.zeros(n, bool))

    class Log:
        def log(self, *a, **k):
            pass
    def state(ag):
        return torch.cat([ag._critic_flat, ag._target_flat, ag._actor_flat, ag.log_alpha.detach().float().view(1)]).clone()

    noise = (torch.randn((8, 2), device="cuda"), torch.randn((8, 2), device="cuda"))
    finals = []
    for ag in (agent, other):
        np.random.seed(123)
        ag.update(rb, Log(), 8, noise=noise)
        finals.append(state(ag))
    assert torch.equal(finals[0], finals[1]), "eager update() after user autograd differs from the restored agent"
    # graph-replayed updates (non-logging steps; each kind is captured after one eager update of it -- or runs eagerly
    # when the user steps above left the critic optimizer's step counts unequal: either way both agents must agree)
    finals = []
    for ag in (agent, other):
        ag.log_interval = 1000
        ag.enable_update_graphs(rb)
        np.random.seed(321)
        torch.cuda.manual_seed(321)
        for step in range(9, 15):
            ag.update(rb, Log(), step)
        assert ag._graphs, "no update graph was captured"
        finals.append(state(ag))
        ag.disable_update_graphs()
    assert torch.equal(finals[0], finals[1]), "graph-replayed update() after user autograd differs"
