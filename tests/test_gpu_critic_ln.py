"""CurlSacAgent(critic_layer_norm=True) on the MI355X: the two LayerNorm kernels of the critics alone against float64
(every lane width, a partly filled second workgroup, twin and group strides, untouched neighbours, bit-identical
reruns), Critic.forward under user autograd, every phase of an update against the oracle on the agent's own parameters
(both schedules, detach_encoder, a prioritized buffer), the target soft update, update graphs, gradient clipping,
checkpoints and the flat layout."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests._util import RTOL, rel_err

pytestmark = pytest.mark.gpu

NAN = float("nan")


def check(name, got, ref, tol=RTOL):
    e = rel_err(got, ref)
    print(f"{name}: rel err {e:.3e} (bound {tol:.1e})")
    assert np.isfinite(e) and e <= tol, f"{name}: rel err {e:.3e} > {tol:.1e}"


class NullLogger:
    def __init__(self):
        self.scalars = {}

    def log(self, key, value, step, n=1):
        self.scalars[key] = float(value.item() if isinstance(value, torch.Tensor) else value)

    def log_histogram(self, *a, **k):
        pass

    log_param = log_image = log_histogram


HP = dict(discount=0.99, init_temperature=0.1, alpha_lr=1e-4, alpha_beta=0.5, actor_lr=1e-3, actor_beta=0.9,
          actor_log_std_min=-10, actor_log_std_max=2, actor_update_freq=2, critic_lr=1e-3, critic_beta=0.9,
          critic_tau=0.01, critic_target_update_freq=2, encoder_feature_dim=50, encoder_lr=1e-3, encoder_tau=0.05,
          num_layers=4, num_filters=32, log_interval=1)
IN_HW, OUT_HW = (40, 44), (32, 36)


def make_agent(hidden=96, seed=0, layer_norm=True, **kw):
    import curla_amd
    aug = curla_amd.RandomCrop(IN_HW, OUT_HW)
    torch.manual_seed(seed)
    agent = curla_amd.CurlSacAgent((9,) + OUT_HW, (2,), torch.device("cuda"), aug, hidden_dim=hidden,
                                   critic_layer_norm=layer_norm, **{**HP, **kw})
    return agent, aug


def perturb_layer_norms(agent, seed=3):
    """gamma = 1, beta = 0 hide a kernel that ignores them: move both, in the critic and the target alike."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for critic in (agent.critic, agent.critic_target):
            for q in (critic.Q1, critic.Q2):
                for i in (1, 4):
                    q.trunk[i].weight.add_((0.2 * torch.randn(q.trunk[i].weight.shape, generator=g)).cuda())
                    q.trunk[i].bias.add_((0.2 * torch.randn(q.trunk[i].bias.shape, generator=g)).cuda())


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------- 1. the kernels alone
GUARD = 16


def _strided(dense, strides, fill=NAN):
    """``dense`` [..., R, C] placed in a flat NaN buffer with the given element strides for its leading dims (rows
    dense), plus GUARD floats behind: (flat device buffer, boolean mask of the elements that belong to the tensor)."""
    lead = dense.shape[:-2]
    block = dense.shape[-2] * dense.shape[-1]
    size = sum((n - 1) * s for n, s in zip(lead, strides)) + block + GUARD
    flat = torch.full((size,), fill)
    mask = torch.zeros(size, dtype=torch.bool)
    for idx in np.ndindex(*lead):
        off = sum(i * s for i, s in zip(idx, strides))
        flat[off:off + block] = dense[idx].reshape(-1)
        mask[off:off + block] = True
    return flat.cuda(), mask


def _gather(flat, shape, strides):
    lead = shape[:-2]
    block = shape[-2] * shape[-1]
    out = torch.empty(shape)
    f = flat.cpu()
    for idx in np.ndindex(*lead):
        off = sum(i * s for i, s in zip(idx, strides))
        out[idx] = f[off:off + block].view(shape[-2:])
    return out


def _same_bits(a, b):
    return torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32))


KERNEL_CASES = [(H, B, 1, 0) for H in (64, 100, 513, 1024) for B in (3, 5)] + [(100, 5, 2, 0), (100, 5, 2, 1)]


@pytest.mark.parametrize("H,B,n2,first", KERNEL_CASES)
def test_kernels_alone(H, B, n2, first):
    """NF = 1 (H = 64), 2 with dead lanes (100), 16 with one feature in the ninth slot (513), 16 full (1024); B = 3 is
    less than a workgroup's four rows, 5 a second, partly filled workgroup; two twins a non-trivial stride apart, and
    once two groups of twins (outer = 2), saving from the first group and from the second only."""
    from curla_amd import ops
    nb = 2
    sH, sP = B * H + 8, H + 12           # twin strides of the activations / of the parameters
    sH2, sP2 = nb * sH + 24, nb * sP + 4  # group strides
    x = rnd(n2, nb, B, H, seed=H + B) * 1.5 + 0.3
    gamma = 1 + 0.3 * rnd(n2, nb, 1, H, seed=1)
    beta = 0.3 * rnd(n2, nb, 1, H, seed=2)
    x64 = x.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    mean, var = x64.mean(-1, keepdim=True), x64.var(-1, unbiased=False, keepdim=True)
    rstd_ref = (var + 1e-5).rsqrt()
    xhat_ref = (x64 - mean) * rstd_ref
    y_ref = torch.stack([torch.stack([F.relu(F.layer_norm(x64[o, z], (H,), g64[o, z, 0], b64[o, z, 0], 1e-5))
                                      for z in range(nb)]) for o in range(n2)])
    tag = f"H{H} B{B} n2={n2} first={first}"
    # ---- forward
    h, hmask = _strided(x, (sH2, sH))
    gm, _ = _strided(gamma, (sP2, sP))
    bt, _ = _strided(beta, (sP2, sP))
    before = h.clone()
    ns = n2 - first
    xhat = torch.full((ns * nb * B * H + GUARD,), NAN, device="cuda")
    rstd = torch.full((ns * nb * B + GUARD,), NAN, device="cuda")
    outer = None if n2 == 1 else (n2, sH2, sP2)
    ops.mlp_ln_relu_fwd(h, sH, gm, bt, sP, B, H, nb, xhat=xhat, rstd=rstd, outer=outer, save_first=first)
    torch.cuda.synchronize()
    assert _same_bits(h[~hmask.cuda()], before[~hmask.cuda()]), "the forward wrote between or behind the rows"
    assert torch.isnan(xhat[-GUARD:]).all() and torch.isnan(rstd[-GUARD:]).all()
    y = _gather(h, (n2, nb, B, H), (sH2, sH))
    check(f"critic ln fwd h {tag}", y, y_ref.detach())
    assert (y >= 0).all() and (y == 0).any()
    check(f"critic ln fwd xhat {tag}", xhat[:-GUARD].view(ns, nb, B, H), xhat_ref.detach()[first:])
    check(f"critic ln fwd rstd {tag}", rstd[:-GUARD].view(ns, nb, B), rstd_ref.detach()[first:, :, :, 0])
    # a no-grad pass (NULL xhat / rstd) computes the same bits
    h2, _ = _strided(x, (sH2, sH))
    ops.mlp_ln_relu_fwd(h2, sH, gm, bt, sP, B, H, nb, outer=outer)
    assert _same_bits(h2, h)
    if n2 > 1:
        return
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
        if params:
            ops.mlp_ln_bwd(dh, sD, xhat, rstd, gm, sP, B, H, nb, partial=part, dgamma=outs[0], dbeta=outs[1],
                           dbias=outs[2], sg=sG)
        else:
            ops.mlp_ln_bwd(dh, sD, xhat, rstd, gm, sP, B, H, nb)
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
    for (n, r), g in zip(refs, got):
        check(f"critic ln bwd {n} {tag}", g, r)
    dh_again, outs_again = run(True)
    assert _same_bits(dh_again, dh) and all(_same_bits(a, b) for a, b in zip(outs_again, outs))
    dh_only, _ = run(False)              # the actor phase's form: the data gradient alone, the same bits
    assert _same_bits(dh_only, dh)


# ------------------------------------------------------------------------------- 2. Critic.forward under user autograd
def _float64_trunk(trunk):
    H = trunk[0].out_features
    ref = nn.Sequential(nn.Linear(trunk[0].in_features, H), nn.LayerNorm(H), nn.ReLU(), nn.Linear(H, H), nn.LayerNorm(H),
                        nn.ReLU(), nn.Linear(H, 1)).double()
    ref.load_state_dict({k: v.detach().cpu().double() for k, v in trunk.state_dict().items()})
    return ref


def test_critic_forward_under_user_autograd():
    B, Fd, A = 5, 50, 2
    agent, _ = make_agent(hidden=96)
    perturb_layer_norms(agent)
    critic = agent.critic
    obs = torch.rand((B, 9) + OUT_HW, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)) * 255
    with torch.no_grad():
        z0 = critic.encoder(obs).clone()
        action0 = torch.tanh(rnd(B, A, seed=2)).cuda()
        q1_ng, q2_ng = (q.clone() for q in critic(obs, action0))
    z = z0.clone().requires_grad_(True)
    action = action0.clone().requires_grad_(True)
    hook = critic.encoder.register_forward_hook(lambda mod, args, out: z)  # the features as a leaf: d z is observable
    try:
        agent.critic_optimizer.zero_grad()
        q1, q2 = critic(obs, action)
        c1, c2 = rnd(B, 1, seed=3).cuda(), rnd(B, 1, seed=4).cuda()
        ((q1 * c1).sum() + (q2 * c2).sum()).backward()
    finally:
        hook.remove()
    assert torch.equal(q1.detach(), q1_ng) and torch.equal(q2.detach(), q2_ng)  # same launches, same bits
    z64 = z0.detach().cpu().double().requires_grad_(True)
    a64 = action0.detach().cpu().double().requires_grad_(True)
    refs = [_float64_trunk(critic.Q1.trunk), _float64_trunk(critic.Q2.trunk)]
    xa = torch.cat([z64, a64], 1)
    r1, r2 = refs[0](xa), refs[1](xa)
    ((r1 * c1.cpu().double()).sum() + (r2 * c2.cpu().double()).sum()).backward()
    check("autograd q1", q1, r1.detach())
    check("autograd q2", q2, r2.detach())
    check("autograd d z", z.grad, z64.grad)
    check("autograd d action", action.grad, a64.grad)
    n = 0
    for tag, q, ref in (("Q1", critic.Q1, refs[0]), ("Q2", critic.Q2, refs[1])):
        got = dict(q.trunk.named_parameters())
        for k, p in ref.named_parameters():
            assert got[k].grad is not None, (tag, k)
            check(f"autograd {tag}.trunk.{k} grad", got[k].grad, p.grad)
            n += 1
    assert n == 20  # per Q function 6 Linear tensors + 4 LayerNorm tensors
    # ... and they landed in the flat gradient buffer
    lo, hi = agent._critic_gflat.data_ptr(), agent._critic_gflat.data_ptr() + 4 * agent._critic_gflat.numel()
    assert all(lo <= p.grad.data_ptr() < hi for q in (critic.Q1, critic.Q2) for p in q.parameters())


# --------------------------------------------------------------- 3. the phases against the oracle, own parameters
def _ln_mlp3(O):
    real = O.mlp3

    def mlp3(p, prefix, x, plan=None, hidden=None):
        """oracle.mlp3 with a LayerNorm in front of each ReLU of the Q functions' trunks (keys 0, 1, 3, 4, 6); the
        actor's trunk is the oracle's own."""
        if prefix not in ("Q1.trunk.", "Q2.trunk."):
            return real(p, prefix, x, plan, hidden)
        ln = lambda h, i: F.layer_norm(h, (h.size(-1),), p[f"{prefix}{i}.weight"], p[f"{prefix}{i}.bias"], 1e-5)  # noqa: E731
        h1 = F.linear(x, p[f"{prefix}0.weight"], p[f"{prefix}0.bias"])
        h2 = F.linear(O._relu(ln(h1, 1), plan, (prefix, 0)), p[f"{prefix}3.weight"], p[f"{prefix}3.bias"])
        if hidden is not None:
            hidden += [h1.detach(), h2.detach()]
        return F.linear(O._relu(ln(h2, 4), plan, (prefix, 1)), p[f"{prefix}6.weight"], p[f"{prefix}6.bias"])
    return mlp3


def _grads_of(module):
    out = {}
    for n, p in module.named_parameters():
        g = p.grad
        if g is None:
            continue
        if n.endswith("encoder.fc.weight"):
            g = module.encoder.fc.to_reference_layout(g)
        out[n] = g.detach().cpu().clone()
    return out


def _snap(module, own_only=False):
    return {k: v.detach().cpu().clone() for k, v in module.state_dict().items() if not (own_only and ".convs." in k)}


def _data(n=48, seed=4):
    rs = np.random.RandomState(seed)
    return dict(obs=rs.randint(0, 256, (n, 9) + IN_HW, dtype=np.uint8), nxt=rs.randint(0, 256, (n, 9) + IN_HW, dtype=np.uint8),
                act=rs.uniform(-1, 1, (n, 2)).astype(np.float32), rew=rs.randn(n).astype(np.float32),
                done=(np.arange(n) % 7) == 6)


def _branches(O, ws, ref_enc, tag, layers=4):
    out = []
    for i in range(layers):
        dev_act = ws.acts_main[i].permute(0, 3, 1, 2).cpu()
        ref_act = ref_enc[f"conv{i + 1}"]
        check(f"{tag} activations conv{i + 1}", dev_act, ref_act)
        differ = (dev_act > 0) != (ref_act > 0)
        assert int(differ.sum()) <= 4
        if differ.any():
            assert float(torch.maximum(dev_act[differ].abs(), ref_act[differ].abs()).max()) <= 1e-5
        out.append(dev_act > 0)
    return out


@pytest.mark.parametrize("variant", ["four_q", "two_launches", "detach_encoder", "prioritized"])
def test_phases_vs_oracle_on_the_agents_own_parameters(variant, monkeypatch):
    """Two updates (one even, one odd) with every phase held to 1e-4 against the oracle's phase functions evaluated on
    the agent's own parameters, the oracle's Q trunks replaced by the LayerNorm ones: the critic loss and all 32 critic
    gradients (24 + 8 LayerNorm), the actor loss, alpha loss, the actor's 10 gradients and log_alpha's -- all of which
    pass through the LayerNorm critic's data gradient --, conv gradients along the device's ReLU branches."""
    import curla_amd
    from oracle import curla_oracle as O
    monkeypatch.setattr(O, "mlp3", _ln_mlp3(O))
    if variant == "two_launches":
        monkeypatch.setenv("CURLA_FOUR_Q", "0")
    torch.manual_seed(9)
    np.random.seed(9)
    B, layers = 16, 4
    detach = variant == "detach_encoder"
    per = variant == "prioritized"
    critic_only = detach or per
    agent, aug = make_agent(hidden=96, detach_encoder=detach)
    assert (agent._twin_outer is None) == (variant == "two_launches")
    perturb_layer_norms(agent)
    d = _data()
    rb = curla_amd.ReplayBuffer((9,) + IN_HW, (2,), 64, B, torch.device("cuda"), aug, **(dict(prioritized=True) if per else {}))
    rb.add_batch(d["obs"], d["act"], d["rew"], d["nxt"], d["done"])
    if per:
        rs = np.random.RandomState(2)
        rb.update_priorities(torch.arange(48, device="cuda"), torch.as_tensor(rs.randint(1, 20, 48).astype(np.float32)).cuda())
    L = NullLogger()
    kw = dict(num_layers=layers, log_std_min=-10, log_std_max=2)
    grads = {}

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
        rows = obs.per.rows.cpu().numpy() if per else idxs
        if variant == "four_q":  # (obs and next_obs as one handle: the schedule with the four Q functions in one launch)
            assert obs.pair is not None and obs.pair[1] is nxt and obs.pair[0].B == 2 * B
        crop = lambda src, j: torch.from_numpy(O.random_crop(src[rows], offs[2 * j], offs[2 * j + 1], OUT_HW)).float()  # noqa: E731
        o_obs, o_nxt = crop(d["obs"], 0), crop(d["nxt"], 1)
        o_act, o_rew = torch.from_numpy(d["act"][rows]), torch.from_numpy(d["rew"][rows])[:, None]
        o_nd = torch.from_numpy(1.0 - d["done"][rows].astype(np.float32))[:, None]
        ws = agent._ws(B)
        tag = f"critic-ln {variant} step{step}"
        # ---- critic
        pre = (_snap(agent.actor, True), _snap(agent.critic), _snap(agent.critic_target), agent.log_alpha.detach().cpu().clone())
        agent.update_critic(obs, act, rew, nxt, nd, L, step, noise=nc.cuda())
        args = (*pre, o_obs, o_act, o_rew, o_nxt, o_nd, nc)
        ref = O.critic_phase(*args, discount=0.99, detach_encoder=detach, **kw)
        br = _branches(O, ws, ref["enc"], tag + " critic")
        ref = O.critic_phase(*args, discount=0.99, detach_encoder=detach, relu_branches=br, **kw)
        if per:
            # the weighted loss of a prioritized minibatch, the importance weights read back from the device
            w = ws.per_w.detach().cpu().clone().view(-1, 1)
            assert float(w.min()) < 0.9 and float(w.max()) == 1.0
            c = O._leafify(pre[1])
            q1, q2 = O.critic_forward(c, o_obs, o_act, layers, plan=O._branch_plan(br))
            loss = (w * (q1 - ref["target_Q"]) ** 2).mean() + (w * (q2 - ref["target_Q"]) ** 2).mean()
            loss.backward()
            ref = dict(loss=loss.detach(), grads=O._grads(c))
        check(f"{tag} critic loss", L.scalars["train_critic/loss"], ref["loss"])
        want = {k: v for k, v in ref["grads"].items() if v is not None}
        assert len(grads["critic"]) == len(want) == (24 if detach else 32)
        assert sum(".trunk.1." in k or ".trunk.4." in k for k in want) == 8
        for k, v in want.items():
            check(f"{tag} critic grad {k}", grads["critic"][k], v)
        if step % 2 == 0 and not critic_only:
            # ---- actor / alpha (on the critic as its step left it)
            ref = O.actor_phase(_snap(agent.actor, True), _snap(agent.critic), agent.log_alpha.detach().cpu().clone(),
                                o_obs, na, target_entropy=float(agent.target_entropy), **kw)
            agent.update_actor_and_alpha(obs, L, step, noise=na.cuda())
            check(f"{tag} actor loss", L.scalars["train_actor/loss"], ref["actor_loss"])
            check(f"{tag} alpha loss", L.scalars["train_alpha/loss"], ref["alpha_loss"])
            got = {k: v for k, v in grads["actor"].items() if ".convs." not in k}
            assert len(got) == len(ref["grads"]) == 10
            for k, v in ref["grads"].items():
                check(f"{tag} actor grad {k}", got[k], v)
            check(f"{tag} log_alpha grad", grads["actor.extra"], ref["log_alpha_grad"])
            agent.soft_update_targets()


# ---------------------------------------------------------------------------------------------------- 4. soft update
def _ring(aug, B=16, seed=1, n=40, **kw):
    import curla_amd
    rb = curla_amd.ReplayBuffer((9,) + IN_HW, (2,), 64, B, torch.device("cuda"), aug, **kw)
    d = _data(n, seed)
    rb.add_batch(d["obs"], d["act"], d["rew"], d["nxt"], d["done"])
    return rb


def test_soft_update_moves_the_target_layer_norms_with_critic_tau():
    """One even update() whose step takes the critic phase, the actor phase and the target soft update but no CURL
    phase (cpc_update_freq = 4, step 2): the CURL phase would move the online encoder again behind the soft update,
    and the encoder tensors could no longer be compared."""
    np.random.seed(3)
    agent, aug = make_agent(hidden=96, seed=3, cpc_update_freq=4)
    perturb_layer_norms(agent)
    with torch.no_grad():  # (target != critic, so that the lerp shows)
        for q in (agent.critic_target.Q1, agent.critic_target.Q2):
            for i in (1, 4):
                q.trunk[i].weight.mul_(1.1)
                q.trunk[i].bias.add_(0.05)
    rb = _ring(aug)
    before = {k: v.detach().clone() for k, v in agent.critic_target.state_dict().items()}
    agent.update(rb, NullLogger(), 2)
    sd, st = agent.critic.state_dict(), agent.critic_target.state_dict()
    keys = [f"Q{q}.trunk.{i}.{t}" for q in (1, 2) for i in (1, 4) for t in ("weight", "bias")]
    for k in keys + ["Q1.trunk.3.weight", "encoder.convs.0.weight", "encoder.ln.weight"]:
        tau = HP["encoder_tau"] if k.startswith("encoder.") else HP["critic_tau"]
        assert not torch.equal(st[k], before[k]), k
        check(f"soft update {k}", st[k], tau * sd[k] + (1 - tau) * before[k], 1e-6)


# ---------------------------------------------------------------------------------------------------- 5. update graphs
def _state_of(agent):
    out = {"critic": agent._critic_flat.clone(), "target": agent._target_flat.clone(), "actor": agent._actor_flat.clone(),
           "log_alpha": agent.log_alpha.detach().clone()}
    for name, opt in agent._optimizers().items():
        for i, st in opt.state_dict()["state"].items():
            for k, v in st.items():
                if torch.is_tensor(v):
                    out[f"{name}.{i}.{k}"] = v.detach().clone()
    return out


def test_update_graphs_replay_a_layer_norm_agent_bit_identically():
    def run(graphs):
        np.random.seed(11)
        torch.manual_seed(11)
        torch.cuda.manual_seed_all(11)
        agent, aug = make_agent(hidden=96, seed=11, log_interval=100)
        perturb_layer_norms(agent)
        rb = _ring(aug)
        if graphs:
            agent.enable_update_graphs(rb, warm=1)
        L = NullLogger()
        for step in range(1, 5):  # odd, even (eager: warm), odd, even (captured and replayed)
            agent.update(rb, L, step)
        torch.cuda.synchronize()
        if graphs:
            assert len(agent._graphs) == 2 and all(st["graph"] is not None for ring in agent._graphs.values() for st in ring)
        return _state_of(agent)
    eager, graphed = run(False), run(True)
    assert set(eager) == set(graphed) and len(eager) > 20
    for k, v in eager.items():
        assert torch.equal(v, graphed[k]), k


# ---------------------------------------------------------------------------------------------------------- 6. clipping
def test_clipped_critic_norm_counts_the_layer_norm_gradients():
    np.random.seed(6)
    agent, aug = make_agent(hidden=96, seed=6)
    perturb_layer_norms(agent)
    agent.set_max_grad_norm(0.05)
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
    assert len(taken) == 12 + 20
    norm = lambda names: float(torch.sqrt(sum((taken[n] ** 2).sum() for n in names)))  # noqa: E731
    with_ln = norm(taken)
    without = norm([n for n in taken if ".trunk.1." not in n and ".trunk.4." not in n])
    logged = float(agent.grad_clip_stats[0, 0])
    print(f"critic gradient norm: logged {logged!r}, float64 {with_ln!r}, without the LayerNorm tensors {without!r}")
    assert with_ln > 0.05  # (the step was clipped)
    # the logged figure is a float32 (2^-24 relative) of a sum taken in double: 1e-5 relative is generous for "equal",
    # and "not equal to the norm without them" has to clear that same margin, by a factor of ten
    tol = 1e-5 * with_ln
    assert abs(logged - with_ln) <= tol
    assert abs(logged - without) > 10 * tol


# ------------------------------------------------------------------------------------------------------ 7. persistence
def test_checkpoint_round_trip_and_flag_mismatch(tmp_path):
    np.random.seed(5)
    agent, aug = make_agent(hidden=96, seed=5)
    rb, L = _ring(aug), NullLogger()
    for step in range(3):
        agent.update(rb, L, step)
    ck = tmp_path / "ln.pt"
    agent.save_checkpoint(str(ck), 3)
    for step in range(3, 5):
        agent.update(rb, L, step)
    want = _state_of(agent)

    np.random.seed(99)  # a different process state: everything must come from the file
    other, aug2 = make_agent(hidden=96, seed=99)
    rb2 = _ring(aug2)
    assert other.load_checkpoint(str(ck)) == 3
    for step in range(3, 5):
        other.update(rb2, L, step)
    torch.cuda.synchronize()
    got = _state_of(other)
    assert set(got) == set(want)
    for k, v in want.items():
        assert torch.equal(v, got[k]), k
    # the reference's three files round-trip too
    agent.save(str(tmp_path), "crop", 5)
    third, _ = make_agent(hidden=96, seed=7)
    third.load(str(tmp_path), "crop", 5)
    for k, v in agent.critic.state_dict().items():
        assert torch.equal(v, third.critic.state_dict()[k]) and torch.equal(v, third.critic_target.state_dict()[k]), k
    # a LayerNorm file does not load into a plain agent, nor a plain one into a LayerNorm agent
    plain, _ = make_agent(hidden=96, seed=5, layer_norm=False)
    with pytest.raises(RuntimeError, match="Missing key"):
        plain.load_checkpoint(str(ck))
    plain_ck = tmp_path / "plain.pt"
    plain2, _ = make_agent(hidden=96, seed=5, layer_norm=False)
    plain2.save_checkpoint(str(plain_ck), 0)
    with pytest.raises(RuntimeError, match="Missing key"):
        other.load_checkpoint(str(plain_ck))


# ------------------------------------------------------------------------------------------------------------ 8. layout
def test_layer_norm_tensors_lie_in_the_flat_q_block():
    agent, _ = make_agent(hidden=96)
    q0, q1 = agent._lay["q"]
    H = 96

    def offset(t, flat):
        off = (t.data_ptr() - flat.data_ptr()) // 4
        assert (t.data_ptr() - flat.data_ptr()) % 4 == 0 and q0 <= off and off + H <= q1, off
        return off
    for critic, flat, gflat in ((agent.critic, agent._critic_flat, agent._critic_gflat),
                                (agent.critic_target, agent._target_flat, None)):
        for i in (1, 4):
            for t in ("weight", "bias"):
                p1, p2 = getattr(critic.Q1.trunk[i], t), getattr(critic.Q2.trunk[i], t)
                assert offset(p2, flat) == offset(p1, flat) + critic.twin_stride
                if gflat is not None:
                    assert offset(p1.grad, gflat) == offset(p1, flat) and offset(p2.grad, gflat) == offset(p2, flat)
                else:
                    assert p1.grad is None and not p1.requires_grad
    assert agent._target_flat.data_ptr() + 4 * agent._lay["total"] == agent._critic_flat.data_ptr()
    ws = agent._ws(8)
    assert ws.q_xhat1.shape == ws.q_xhat2.shape == (2, 8, H) and ws.q_rstd1.shape == ws.q_rstd2.shape == (2, 8)
    plain, _ = make_agent(hidden=96, layer_norm=False)
    assert not hasattr(plain._ws(8), "q_xhat1")
