"""CurlSacAgent(policy="deterministic") on the MI355X: the head's forward alone against the float64
definition (tests/_det_policy_ref.py) -- shapes around the four-rows-per-workgroup boundary, the definition's seams, every
subset of optional outputs, the form fused into the last layer against the launch of its own, reruns --, the in-kernel
draw, the two backward kernels, Actor.forward under user autograd, acting, the critic and actor phases of two even and
two odd updates against float64 on the agent's own parameters over eight critic / buffer variants, and whole-agent cases:
update graphs under a std schedule, utd_ratio, one-rank data parallel, clipping, a reset, a ReDo pass, checkpoints,
refusals.  Buffers around the kernels' outputs are NaN-filled and checked untouched."""
import itertools
import socket

import numpy as np
import pytest
import torch

from tests import _det_policy_ref as R
from tests import _hlg_ref as RH
from tests import _tqc_ref as RT
from tests.test_gpu_critic_dropout import _drop_mlp3
from tests.test_gpu_critic_ln import HP, NAN, NullLogger, _branches, _grads_of, _same_bits, _snap, _state_of, perturb_layer_norms, rnd
from tests.test_gpu_critic_ln import check as _check
from tests.test_gpu_graph_aug import HEAD_VS_NUMPY
from tests.test_gpu_tqc import _Adam64, _assert_same_state
from tests.test_gpu_utd import _build, _lead_step, _state
from tests._util import RTOL, rel_err

pytestmark = pytest.mark.gpu

GUARD = 16
LIM32 = np.float32(1.0) - np.float32(1e-6)
WORST = {}  # the largest error each group of checks has seen: printed by the module's last test


def check(name, got, ref, tol=RTOL):
    group = "kernels alone" if name.startswith(("head ", "bwd ")) else "agent level"
    e = rel_err(got, ref)
    if np.isfinite(e) and e > WORST.get(group, (0.0, ""))[0]:
        WORST[group] = (e, name)
    _check(name, got, ref, tol)


def dev(t):
    return t.float().contiguous().cuda()


def nan(*shape):
    return torch.full(shape, NAN, device="cuda")


def std_t(s):
    return torch.full((1,), s, device="cuda", dtype=torch.float32)


# ------------------------------------------------------------------------------------------- 1. the head forward alone
OUTS = ("mu", "pi", "log_pi", "log_std", "xa")
FZ = 5  # feature columns in front of the action columns of the Q input rows


def _head(ops, o, noise, s, clip, want=OUTS, rng=None, std=None, fused=None):
    """One launch of the head on NaN-filled, guarded outputs: {name: tensor} of the outputs in ``want`` (xa: the action
    columns) and, with ``rng``, the stored noise.  ``fused`` = (h, W, bias): through the last layer's launch; returns the
    trunk output too."""
    B, A = o.shape
    size = dict(mu=B * A, pi=B * A, log_std=B * A, log_pi=B)
    buf = {k: nan(size[k] + GUARD) for k in want if k != "xa"}
    xa = nan(B * (FZ + A) + GUARD) if "xa" in want else None
    kw = {k: v[:size[k]].view(B, 1 if k == "log_pi" else A) for k, v in buf.items()}
    if xa is not None:
        kw["xa"] = xa[:B * (FZ + A)].view(B, FZ + A)
    sampled = "pi" in want or "xa" in want
    nz = None
    if sampled:
        nz = nan(B * A + GUARD) if rng is not None else torch.cat([dev(noise).view(-1), nan(GUARD)])
    nzv = None if nz is None else nz[:B * A].view(B, A)
    std = std_t(s) if std is None else std
    out = {}
    if fused is None:
        ops.det_head_fwd(dev(o), nzv, std, clip, B, A, rng=rng if sampled else None, **kw)
    else:
        h, W, bias = fused
        trunk = nan(B * A + GUARD)
        ops.mlp_out_det_head_fwd(dev(h), dev(W), dev(bias), trunk[:B * A].view(B, A), nzv, B, A, h.shape[1], std, clip,
                                 rng=rng if sampled else None, **kw)
        assert torch.isnan(trunk[B * A:]).all()
        out["trunk"] = trunk[:B * A].view(B, A).clone()
    torch.cuda.synchronize()
    for k, v in buf.items():
        assert torch.isnan(v[size[k]:]).all(), f"{k}: written behind its end"
        out[k] = kw[k].clone()
    if xa is not None:
        assert torch.isnan(xa[B * (FZ + A):]).all() and torch.isnan(kw["xa"][:, :FZ]).all(), "xa: feature columns written"
        out["xa"] = kw["xa"][:, FZ:].clone()
    if nz is not None:
        assert torch.isnan(nz[B * A:]).all()
        out["noise"] = nzv.clone()
    return out


def _check_head(tag, o, noise, s, clip, **kw):
    from curla_amd import ops
    ref = R.forward(o, noise, s, clip)
    got = _head(ops, o, noise, s, clip, **kw)
    check(f"head mu {tag}", got["mu"], ref["mu"])
    check(f"head pi {tag}", got["pi"], ref["pi"])
    assert _same_bits(got["xa"], got["pi"])
    assert not got["log_pi"].cpu().view(torch.int32).any(), "log_pi is not +0.0 everywhere"
    want_ls = np.float32(np.log(np.float64(np.float32(s))))
    assert _same_bits(got["log_std"], torch.full(o.shape, float(want_ls)))
    assert float(got["pi"].abs().max()) <= float(LIM32)
    again = _head(ops, o, noise, s, clip, **kw)
    assert all(_same_bits(again[k], got[k]) for k in got), "a rerun changed bits"
    return got, ref


@pytest.mark.parametrize("clip", [0.3, None])
@pytest.mark.parametrize("A", [1, 2, 8])
@pytest.mark.parametrize("B", [1, 3, 5])
def test_head_forward_against_float64(B, A, clip):
    """B = 1, 3: less than a workgroup's four rows of the fused form; 5: a second, partly filled one."""
    o, noise = 1.5 * rnd(B, A, seed=10 * B + A), rnd(B, A, seed=10 * B + A + 1)
    _check_head(f"B{B} A{A} clip {clip}", o, noise, 0.7, clip)


def test_head_forward_at_the_seams():
    """Rows built on the definition's seams, each held to float64: the noise clip binding on both sides, the outer clamp
    binding on both sides, m saturated at o = +-20, n = 0; then c = 0 (pi is mu wherever |mu| <= lim) and c = None."""
    s, c = 0.5, 0.3
    #                 o      n
    rows = [(0.2, 2.0), (0.2, -2.0),      # |s n| = 1 > c: e = +-c
            (0.2, 0.4), (-0.3, -0.5),     # |s n| < c: e = s n
            (3.0, 1.0), (-3.0, -1.0),     # m + e beyond +-lim: the outer clamp binds
            (20.0, 0.1), (-20.0, -0.1),   # m saturates to +-1 in float32
            (20.0, -2.0), (-20.0, 2.0),   # saturated m pulled back inside by the clipped noise
            (0.7, 0.0), (-0.7, 0.0),      # n = 0
            (1e-3, 0.6), (1e-4, -0.6)]
    o = torch.tensor([[r[0], -r[0]] for r in rows])
    n = torch.tensor([[r[1], r[1]] for r in rows])
    got, ref = _check_head("seams", o, n, s, c)
    pi = got["pi"].cpu()
    m02 = np.tanh(np.float64(np.float32(0.2)))
    assert abs(float(ref["pi"][0, 0]) - (m02 + c)) <= 1e-15 and abs(float(ref["pi"][1, 0]) - (m02 - c)) <= 1e-15
    assert pi[4, 0] == LIM32 and pi[5, 0] == -LIM32 and pi[6, 0] == LIM32 and pi[7, 0] == -LIM32  # exactly on the bound
    assert got["mu"][6, 0] == 1.0 and got["mu"][7, 0] == -1.0
    assert abs(float(pi[8, 0]) - 0.7) <= 1e-6 and abs(float(pi[9, 0]) + 0.7) <= 1e-6
    assert _same_bits(pi[10:12], got["mu"][10:12].cpu())  # n = 0: pi is mu
    big = 4.0 * rnd(9, 3, seed=5)  # larger |s n|, a wide clip, no clip and clip 0
    for clip in (5.0, None, 0.0):
        g, _ = _check_head(f"seams clip {clip}", torch.cat([o, 1.2 * rnd(9, 2, seed=3)]), torch.cat([n, big[:, :2]]), 1.3, clip)
        if clip == 0.0:
            assert _same_bits(g["pi"], g["mu"].clamp(-float(LIM32), float(LIM32)))
            inside = g["mu"].abs() <= float(LIM32)
            assert bool(inside.sum() >= 30) and torch.equal(g["pi"][inside], g["mu"][inside])


def test_head_forward_every_subset_of_outputs_absent():
    """All 32 subsets of (mu, pi, log_pi, log_std, xa): each output present carries the bits of the launch with all five;
    a subset without pi and xa runs without noise (compute_pi False)."""
    from curla_amd import ops
    B, A = 5, 3
    o, noise = 1.5 * rnd(B, A, seed=1), rnd(B, A, seed=2)
    full = _head(ops, o, noise, 0.4, 0.3)
    n = 0
    for r in range(len(OUTS) + 1):
        for want in itertools.combinations(OUTS, r):
            got = _head(ops, o, noise, 0.4, 0.3, want=want)
            assert set(got) - {"noise"} == set(want)
            for k in want:
                assert _same_bits(got[k], full[k]), (want, k)
            n += 1
    assert n == 32


@pytest.mark.parametrize("A", [1, 2, 8])
@pytest.mark.parametrize("B", [1, 3, 5])
def test_head_fused_into_the_last_layer_writes_the_launches_bits(B, A):
    """K = 64, the smallest hidden width the mlp_out tests run: the last layer's launch with the head in it against
    ops.mlp_out_fwd followed by ops.det_head_fwd -- the trunk output and every head output, bit for bit, explicit noise and
    the in-kernel draw alike -- and against float64 through the dot products."""
    from curla_amd import ops
    K = 64
    h, W, bias = torch.relu(rnd(B, K, seed=B)), 0.3 * rnd(A, K, seed=A + 20), 0.1 * rnd(A, seed=7)
    noise = rnd(B, A, seed=B + A)
    out = nan(B * A + GUARD)
    ops.mlp_out_fwd(dev(h), B * K, dev(W), 0, dev(bias), 0, out[:B * A].view(B, A), B * A, B, A, K, 1)
    o = out[:B * A].view(B, A).cpu()
    assert torch.isnan(out[B * A:]).all()
    o64 = h.double() @ W.double().T + bias.double()
    check(f"head fused trunk B{B} A{A}", o, o64)
    for rng in (None, (0xC0FFEE + B, 3 + A)):
        alone = _head(ops, o, noise, 0.6, 0.3, rng=rng)
        fused = _head(ops, o, noise, 0.6, 0.3, rng=rng, fused=(h, W, bias))
        assert _same_bits(fused.pop("trunk"), o)
        assert set(fused) == set(alone) and all(_same_bits(fused[k], alone[k]) for k in alone), rng
        ref = R.forward(o64, alone["noise"], 0.6, 0.3)
        check(f"head fused pi B{B} A{A} rng {rng is not None}", fused["pi"], ref["pi"])
        check(f"head fused mu B{B} A{A} rng {rng is not None}", fused["mu"], ref["mu"])


# ------------------------------------------------------------------------------------------------ 2. the in-kernel draw
@pytest.mark.parametrize("B,A", [(1, 1), (3, 2), (5, 8), (67, 3)])
def test_in_kernel_draw(B, A):
    """The stored noise is the reference stream's for (seed, offset), to the tolerance tests/test_gpu_graph_aug.py holds
    the Gaussian head's draws to (and bit for bit the Gaussian head's own); fed back as explicit noise it reproduces pi;
    rng_dev is read when the kernel runs; so is std."""
    from curla_amd import ops
    seed, off = 0x1234ABCD5 + B, 10 ** 12 + A
    o = 1.5 * rnd(B, A, seed=B)
    got = _head(ops, o, None, 0.5, 0.3, rng=(seed, off))
    want = R.philox_normals(seed, off, B * A)
    worst = float(np.abs(got["noise"].cpu().numpy().reshape(-1) - want).max())
    print(f"det head noise vs the NumPy restatement B{B} A{A}: worst |diff| = {worst:.3e}")
    assert worst <= HEAD_VS_NUMPY
    gauss = nan(B, A)
    ops.actor_head_fwd(torch.zeros(B, 2 * A, device="cuda"), gauss, B, A, -10.0, 2.0, pi=nan(B, A), rng=(seed, off))
    assert _same_bits(gauss, got["noise"])  # one stream, one set of counters
    fed = _head(ops, o, got["noise"].cpu(), 0.5, 0.3)
    assert all(_same_bits(fed[k], got[k]) for k in got)
    check(f"head pi of the drawn noise B{B} A{A}", got["pi"], R.forward(o, got["noise"], 0.5, 0.3)["pi"])
    # rng_dev: (seed, offset) from device memory at run time, the by-value pair ignored
    ctl = torch.tensor([seed, off], dtype=torch.int64, device="cuda")
    by_dev = _head(ops, o, None, 0.5, 0.3, rng=(99, 99, ctl.data_ptr()))
    assert all(_same_bits(by_dev[k], got[k]) for k in got)
    ctl[1] += 1
    moved = _head(ops, o, None, 0.5, 0.3, rng=(99, 99, ctl.data_ptr()))
    assert not torch.equal(moved["noise"], got["noise"])
    if B * A > 4:  # the next counter: the stream four elements on
        assert _same_bits(moved["noise"].view(-1)[:B * A - 4], got["noise"].view(-1)[4:])
    # std is data: an edit of the device scalar between two launches changes the result with no other call
    std = std_t(0.5)
    a = _head(ops, o, got["noise"].cpu(), None, None, std=std)
    std.fill_(1.25)
    b = _head(ops, o, got["noise"].cpu(), None, None, std=std)
    assert _same_bits(a["mu"], b["mu"]) and not torch.equal(a["pi"], b["pi"]) and not torch.equal(a["log_std"], b["log_std"])
    check(f"head pi after the std edit B{B} A{A}", b["pi"], R.forward(o, got["noise"], 1.25, None)["pi"])


# -------------------------------------------------------------------------------------------------------- 3. backward
@pytest.mark.parametrize("A", [1, 2, 8])
@pytest.mark.parametrize("B", [1, 3, 5, 300])
def test_backward_kernels(B, A):
    """Both kernels against float64; the twin-dxa addressing (the action columns of [2, B, F + A], summed over the twin in
    place) against the dense form on the float32 sum, bit for bit; upstream dmu only, dpi only and both; reruns."""
    from curla_amd import ops
    F_ = 7
    o = 1.5 * rnd(B, A, seed=B + A)
    o[0, 0] = 20.0  # a saturated mean: exactly no gradient
    mu = torch.tanh(o.double()).float()
    dxa = rnd(2, B, F_ + A, seed=B)
    dense = (dxa[0, :, F_:] + dxa[1, :, F_:]).contiguous()  # (the kernel's float32 sum)
    want = R.grad_o(o, dpi=dxa[0, :, F_:].double() + dxa[1, :, F_:].double())

    def run(fn):
        d = nan(B * A + GUARD)
        fn(d[:B * A].view(B, A))
        torch.cuda.synchronize()
        assert torch.isnan(d[B * A:]).all()
        return d[:B * A].view(B, A).clone()
    dxa_d, mu_d = dev(dxa), dev(mu)
    twin = run(lambda d: ops.det_head_bwd(None, mu_d, B, A, d, twin_dxa=dxa_d, F=F_))
    flat = run(lambda d: ops.det_head_bwd(dev(dense), mu_d, B, A, d))
    tag = f"B{B} A{A}"
    check(f"bwd twin dxa {tag}", twin, want)
    assert _same_bits(twin, flat) and _same_bits(twin, run(lambda d: ops.det_head_bwd(None, mu_d, B, A, d, twin_dxa=dxa_d, F=F_)))
    assert float(twin[0, 0]) == 0.0 and torch.equal(dxa_d.cpu(), dxa)
    dmu, dpi = rnd(B, A, seed=3), rnd(B, A, seed=4)
    for name, a, b in (("dmu", dmu, None), ("dpi", None, dpi), ("both", dmu, dpi)):
        got = run(lambda d: ops.det_policy_head_bwd(None if a is None else dev(a), None if b is None else dev(b), mu_d, B, A, d))
        check(f"bwd general {name} {tag}", got, R.grad_o(o, dpi=b, dmu=a))
        if name == "dpi":
            assert _same_bits(got, run(lambda d: ops.det_head_bwd(dev(dpi), mu_d, B, A, d)))


def test_entry_points_refuse_what_the_kernels_do_not_take():
    from curla_amd import ops
    from curla_amd._lib import CurlaHipError
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731

    def ok(B=4, A=2, clip=0.3, std=True):
        ops.det_head_fwd(z(4, 9), z(4, 9), std_t(0.2) if std else None, clip, B, A, pi=z(4, 9))
    ok()
    ok(clip=None)
    ok(clip=0.0)
    for bad in (dict(A=0), dict(A=9), dict(B=0), dict(clip=-1.0), dict(clip=float("nan")), dict(std=False)):
        with pytest.raises(CurlaHipError, match="CURLA_ERR_ARG"):
            ok(**bad)
    with pytest.raises(CurlaHipError, match="CURLA_ERR_ARG"):
        ops.det_head_bwd(z(4, 9), z(4, 9), 4, 9, z(4, 9))
    with pytest.raises(CurlaHipError, match="CURLA_ERR_UNSUPPORTED"):
        ops.mlp_out_det_head_fwd(z(4, 66), z(2, 66), z(2), z(4, 2), z(4, 2), 4, 2, 66, std_t(0.2), 0.3, pi=z(4, 2))


# ------------------------------------------------------------------------------------------------ 4. agents: helpers
IN_S, OUT_S = (24, 28), (20, 24)  # the smallest frame the suite runs whole agents at (tests/test_gpu_graph.py)
B_S = 6
STD, CLIP = 0.5, 0.3  # |s n| > c for about half the draws: the clip binds in every phase


def make_agent(hidden=96, seed=0, **kw):
    import curla_amd
    aug = curla_amd.RandomCrop(IN_S, OUT_S)
    torch.manual_seed(seed)
    kw = {"policy_std": STD, "policy_std_clip": CLIP, **kw}
    agent = curla_amd.CurlSacAgent((9,) + OUT_S, (2,), torch.device("cuda"), aug, hidden_dim=hidden, policy="deterministic",
                                   **{**HP, **kw})
    return agent, aug


def _data(n=40, seed=4):
    rs = np.random.RandomState(seed)
    return dict(obs=rs.randint(0, 256, (n, 9) + IN_S, dtype=np.uint8), nxt=rs.randint(0, 256, (n, 9) + IN_S, dtype=np.uint8),
                act=rs.uniform(-1, 1, (n, 2)).astype(np.float32), rew=rs.randn(n).astype(np.float32),
                done=(np.arange(n) % 7) == 6)


def _ring(aug, B=B_S, seed=1, n=40, **kw):
    import curla_amd
    rb = curla_amd.ReplayBuffer((9,) + IN_S, (2,), 64, B, torch.device("cuda"), aug, **kw)
    d = _data(n, seed)
    rb.add_batch(d["obs"], d["act"], d["rew"], d["nxt"], d["done"])
    return rb


def _alpha_untouched(agent, la0):
    """log_alpha bit for bit where construction left it, its gradient and both Adam moments all zeros."""
    torch.cuda.synchronize()
    assert _same_bits(agent.log_alpha.detach().view(1), la0.view(1)) and not agent.log_alpha.grad.any()
    st = agent.log_alpha_optimizer.state.get(agent.log_alpha, {})
    for k in ("exp_avg", "exp_avg_sq"):
        if k in st:
            assert not st[k].cpu().view(torch.int64).any(), k


# ---------------------------------------------------------------------------------------------- 5. user autograd, acting
def test_actor_forward_under_user_autograd():
    B, A = 5, 2
    agent, _ = make_agent()
    actor = agent.actor
    obs = torch.rand((B, 9) + OUT_S, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)) * 255
    noise = rnd(B, A, seed=2)
    with torch.no_grad():
        z0 = actor.encoder(obs).clone()
        mu_ng, pi_ng, lp_ng, ls_ng = (t.clone() for t in actor(obs, noise=noise.cuda()))
        only_mu = actor(obs, compute_pi=False, compute_log_pi=False)
    assert only_mu[1] is None and only_mu[2] is None and _same_bits(only_mu[0], mu_ng)
    assert mu_ng.shape == pi_ng.shape == ls_ng.shape == (B, A) and lp_ng.shape == (B, 1) and not lp_ng.any()
    assert _same_bits(ls_ng, torch.full((B, A), float(np.float32(np.log(np.float64(np.float32(STD)))))))
    z = z0.clone().requires_grad_(True)
    hook = actor.encoder.register_forward_hook(lambda mod, args, out: z)  # the features as a leaf: d z is observable
    c_mu, c_pi = rnd(B, A, seed=3), rnd(B, A, seed=4)
    try:
        agent.actor_optimizer.zero_grad()
        mu, pi, log_pi, log_std = actor(obs, noise=noise.cuda())
        assert mu.requires_grad and pi.requires_grad and not log_pi.requires_grad and not log_std.requires_grad
        ((mu * c_mu.cuda()).sum() + (pi * c_pi.cuda()).sum()).backward()
    finally:
        hook.remove()
    assert _same_bits(mu.detach(), mu_ng) and _same_bits(pi.detach(), pi_ng) and _same_bits(log_std, ls_ng) and not log_pi.any()
    z64 = z0.cpu().double().requires_grad_(True)
    p64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in actor.trunk.state_dict().items()}
    F = torch.nn.functional
    h = F.relu(F.linear(F.relu(F.linear(z64, p64["0.weight"], p64["0.bias"])), p64["2.weight"], p64["2.bias"]))
    o = F.linear(h, p64["4.weight"], p64["4.bias"])
    m64, pi64 = R.policy(o, noise, STD, None)  # (Actor.forward samples without the clip, as DrQ-v2 acts)
    ((m64 * c_mu.double()).sum() + (pi64 * c_pi.double()).sum()).backward()
    check("autograd mu", mu, m64.detach())
    check("autograd pi", pi, pi64.detach())
    check("autograd d z", z.grad, z64.grad)
    got = dict(actor.trunk.named_parameters())
    for k, p in p64.items():
        assert got[k].grad is not None and got[k].grad.shape == p.grad.shape, k
        check(f"autograd trunk.{k} grad", got[k].grad, p.grad)
    assert got["4.weight"].grad.shape == (A, 96)
    agent.actor_optimizer.zero_grad()
    actor(obs, compute_pi=False, compute_log_pi=False)[0].sum().backward()  # mu alone
    check("autograd mu-only trunk.4.bias grad", got["4.bias"].grad, (1 - m64.detach() ** 2).sum(0))


def test_acting():
    agent, _ = make_agent()
    A = 2
    frames = np.random.RandomState(3).randint(0, 256, (4, 9) + OUT_S, dtype=np.uint8)
    means = agent.select_actions(frames)
    assert means.shape == (4, A) and means.dtype == np.float32 and float(np.abs(means).max()) < 1.0
    for i in range(4):  # (a single frame takes other launch shapes: the suite's bar, as tests/test_gpu_acting_batch.py)
        check(f"acting select_action row {i}", agent.select_action(frames[i]), means[i])
    noise = rnd(4, A, seed=5)
    gen = torch.cuda.get_rng_state()
    pi = agent.sample_actions(frames, noise=noise)
    assert torch.equal(torch.cuda.get_rng_state(), gen)  # (explicit noise draws nothing)
    with torch.no_grad():
        mu = agent.select_actions(frames, as_tensor=True)
    want = (mu.cpu().double() + float(np.float32(STD)) * noise.double()).clamp(-R.LIM, R.LIM)  # no clip of the noise
    check("acting sample_actions", pi, want)
    assert float(np.abs(pi - means).max()) > CLIP  # (the update's clip is not applied when acting)
    check("acting sample_action row 1", agent.sample_action(frames[1], noise=noise[1:2].cuda()), pi[1])
    agent.set_policy_std(1e-3)
    assert float(np.abs(agent.sample_actions(frames, noise=noise) - means).max()) < 1e-2
    torch.manual_seed(7)
    a = agent.sample_actions(frames)
    torch.manual_seed(7)
    assert np.array_equal(a, agent.sample_actions(frames)) and not np.array_equal(a, agent.sample_actions(frames))


# ------------------------------------------------------------------ 6. the phases against float64, own parameters
PHASE_RANGE, PHASE_SIGMA, TQC_M, TQC_DROP, HLG_M = (-2.0, 3.0), 0.75, 5, 1, 5
VARIANTS = {
    "four_q": {},
    "two_launches": {},
    "ln_dropout": dict(critic_layer_norm=True, critic_dropout=0.1),
    "tqc": dict(critic_quantiles=TQC_M, critic_drop_quantiles=TQC_DROP),
    "hlg": dict(critic_bins=HLG_M, critic_value_range=PHASE_RANGE, critic_bin_sigma=PHASE_SIGMA),
    "views": dict(aug_views=2),
    "per": {},
    "n_step": {},
}


def _critic_loss64(variant, q1, q2, tq1, tq2, rew, nd, log_alpha, gamma, w=None):
    """(loss, entropy-free target [B] or None) of a variant from the float64 Q outputs: log_pi = 0 throughout."""
    B = q1.shape[0]
    zeros = torch.zeros(B, dtype=torch.float64)
    if variant == "tqc":
        out = RT.critic_loss(torch.stack([q1, q2]), torch.stack([tq1, tq2]), zeros, rew, nd, log_alpha, gamma, TQC_DROP)
        return out["loss"], None
    if variant == "hlg":
        sigma = PHASE_SIGMA * (PHASE_RANGE[1] - PHASE_RANGE[0]) / HLG_M
        out = RH.critic_loss(torch.stack([q1, q2]), torch.stack([tq1, tq2]), zeros, rew, nd, log_alpha, gamma, *PHASE_RANGE, sigma)
        y = (rew + nd * gamma * torch.minimum(RH.expected(tq1, HLG_M, *PHASE_RANGE), RH.expected(tq2, HLG_M, *PHASE_RANGE))[:, None])
        assert float((out["target_q"] - y.view(-1).clamp(*PHASE_RANGE)).abs().max()) <= 1e-12
        return out["loss"], out["target_q"]
    y = R.td_target(tq1, tq2, rew, nd, gamma)
    if variant == "views":
        H = B // 2
        y = 0.5 * (y[:H] + y[H:])
        y = torch.cat([y, y])
        return (((q1 - y) ** 2).sum() + ((q2 - y) ** 2).sum()) / H, y.view(-1)
    if w is not None:
        return (w * (q1 - y) ** 2).mean() + (w * (q2 - y) ** 2).mean(), y.view(-1)
    return ((q1 - y) ** 2).mean() + ((q2 - y) ** 2).mean(), y.view(-1)


def _actor_loss64(variant, q1, q2, log_std, log_alpha, target_entropy):
    B = q1.shape[0]
    zeros = torch.zeros(B, dtype=torch.float64)
    if variant == "tqc":
        return RT.actor_loss(torch.stack([q1, q2]), zeros, log_std, log_alpha, target_entropy)["actor_loss"]
    if variant == "hlg":
        return RH.actor_loss(torch.stack([q1, q2]), zeros, log_std, log_alpha, target_entropy, *PHASE_RANGE)["actor_loss"]
    return -torch.minimum(q1, q2).mean()


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_phases_vs_float64_on_the_agents_own_parameters(variant, monkeypatch):
    """Four updates (two even, two odd), B = 6: the critic loss, the TD target -- the entropy-free one -- and every critic
    gradient, the actor loss and the actor's ten gradients, all within RTOL of the float64 evaluation on the agent's own
    parameters (the oracle's encoder and MLPs, tests/_det_policy_ref.py's policy, the variants' own loss references at
    log_pi = 0), and the parameters each step leaves within RTOL of a float64 Adam step on the gradients it was handed.
    ``four_q`` / ``two_launches`` / ``ln_dropout`` draw through the buffer's handles (the two merged critic-forward
    routes), the others through its float tensors (the third route).  log_pi is +0.0 in every row; log_alpha, its
    gradient and its moments are bit for bit untouched."""
    import curla_amd
    from oracle import curla_oracle as O
    dropq = variant == "ln_dropout"
    state = dict(p=0.1, rng=None, actor=False)
    if dropq:
        monkeypatch.setattr(O, "mlp3", _drop_mlp3(O, state))
    monkeypatch.setenv("CURLA_FOUR_Q", "0" if variant == "two_launches" else "1")
    torch.manual_seed(9)
    np.random.seed(9)
    B, layers, gamma = B_S, 4, HP["discount"]
    handles = variant in ("four_q", "two_launches", "ln_dropout")
    agent, aug = make_agent(**VARIANTS[variant])
    if dropq:
        perturb_layer_norms(agent)
    la0 = agent.log_alpha.detach().clone()
    data = _data()
    rb_kw = dict(prioritized=True) if variant == "per" else dict(n_step=3, discount=gamma) if variant == "n_step" else \
        dict(aug_views=2) if variant == "views" else {}
    rb = curla_amd.ReplayBuffer((9,) + IN_S, (2,), 64, B, torch.device("cuda"), aug, **rb_kw)
    rb.add_batch(data["obs"], data["act"], data["rew"], data["nxt"], data["done"])
    if variant == "per":
        rs = np.random.RandomState(2)
        rb.update_priorities(torch.arange(40, device="cuda"), torch.as_tensor(rs.randint(1, 20, 40).astype(np.float32)).cuda())
    L = NullLogger()
    taken = {}

    def keep(name, module, opt):
        real = opt.step

        def step():
            taken[name] = _grads_of(module)
            taken[name + ".raw"] = ({n: p.detach().double().cpu() for n, p in module.named_parameters() if p.grad is not None},
                                    {n: p.grad.detach().double().cpu() for n, p in module.named_parameters() if p.grad is not None})
            real()
        opt.step = step
    keep("critic", agent.critic, agent.critic_optimizer)
    keep("actor", agent.actor, agent.actor_optimizer)
    adam_c, adam_a = _Adam64(HP["critic_lr"], HP["critic_beta"]), _Adam64(HP["actor_lr"], HP["actor_beta"])
    f64 = lambda x: O.as_dtype(x, torch.float64)  # noqa: E731
    la = agent.log_alpha.detach().cpu().clone()

    for step in range(4):
        nc, na = torch.randn(B, 2), torch.randn(B, 2)
        if handles:
            idxs, offs = rb.draw_indices()
            obs, act, rew, nxt, nd, _ = rb.sample_cpc_refs(indices=(idxs, offs))
            if variant != "two_launches":
                assert obs.pair is not None and obs.pair[1] is nxt and obs.pair[0].B == 2 * B
            crop = lambda src, j: torch.from_numpy(O.random_crop(src[idxs], offs[2 * j], offs[2 * j + 1], OUT_S)).double()  # noqa: E731
            o_obs, o_nxt = crop(data["obs"], 0), crop(data["nxt"], 1)
        else:
            obs, act, rew, nxt, nd, _ = rb.sample_cpc()
            o_obs, o_nxt = obs.detach().cpu().double(), nxt.detach().cpu().double()
        o_act, o_rew, o_nd = act.cpu().double(), rew.cpu().double().view(B, 1), nd.cpu().double().view(B, 1)
        ws = agent._ws(B)
        tag = f"det {variant} step{step}"
        rng_c, rng_a = ((0x1234ABCD + step, 7 + 10 * step), (0x1234ABCD + step, (1 << 40) + step)) if dropq else (None, None)
        # ---- critic
        p_actor, p_critic, p_target = f64((_snap(agent.actor, True), _snap(agent.critic), _snap(agent.critic_target)))
        agent.update_critic(obs, act, rew, nxt, nd, L, step, noise=nc.cuda(), dropout_rng=rng_c)
        assert not ws.log_pi.cpu().view(torch.int32).any(), "log_pi is not +0.0"
        state.update(rng=rng_c, actor=False)
        pa = R.next_action(O, p_actor, p_critic, o_nxt, nc, STD, CLIP, layers)
        unclipped = R.policy(R._trunk_out(O, p_actor, p_critic, o_nxt, layers), nc, STD, None)[1]
        assert bool(((unclipped - pa).abs() > 0.05).any())  # (the noise clip binds somewhere in the minibatch)
        four = handles and agent._twin_outer is not None  # (_q_four: a' goes straight into the target's input rows)
        check(f"{tag} next action", ws.xa2[0][:, -2:] if four else ws.pi, pa)
        with torch.no_grad():
            tq1, tq2 = O.critic_forward(p_target, o_nxt, pa, layers)
        w = ws.per_w.detach().cpu().double().view(B, 1) if variant == "per" else None

        def critic64(br):
            c = O._leafify(p_critic)
            enc = {}
            q1, q2 = O.critic_forward(c, o_obs, o_act, layers, outputs=enc, plan=O._branch_plan(br))
            loss, y = _critic_loss64(variant, q1, q2, tq1, tq2, o_rew, o_nd, la, gamma, w)
            loss.backward()
            return loss.detach(), y, O._grads(c), {k: v.detach() for k, v in enc.items()}
        br = _branches(O, ws, critic64(None)[3], tag + " critic")
        loss, y, grads, _ = critic64(br)
        check(f"{tag} critic loss", L.scalars["train_critic/loss"], loss)
        if y is not None:
            check(f"{tag} target_q is the entropy-free one", ws.target_q.view(-1), y)
        if variant == "per":
            assert float(w.min()) < 0.9 and float(w.max()) == 1.0
        want = {k: v for k, v in grads.items() if v is not None}
        assert len(taken["critic"]) == len(want) == (20 if dropq else 12) + 12
        for k, v in want.items():
            check(f"{tag} critic grad {k}", taken["critic"][k], v)
        now = dict(agent.critic.named_parameters())
        for k, v in adam_c.step(*taken["critic.raw"]).items():
            check(f"{tag} critic post-step {k}", now[k], v)
        if step % 2 == 0:
            # ---- actor (on the critic as its step left it)
            state.update(rng=rng_a, actor=True)
            a = O._leafify(f64(_snap(agent.actor, True)))
            c_now = f64(_snap(agent.critic))
            o = R._trunk_out(O, a, c_now, o_obs, layers, detach_encoder=True)
            mu, pi = R.policy(o, na, STD, CLIP)
            q1, q2 = O.critic_forward(c_now, o_obs, pi, layers, detach_encoder=True)
            log_std = torch.full((B, 2), float(np.log(np.float64(np.float32(STD)))), dtype=torch.float64)
            a_loss = _actor_loss64(variant, q1, q2, log_std, la, float(agent.target_entropy))
            a_loss.backward()
            agent.update_actor_and_alpha(obs, L, step, noise=na.cuda(), dropout_rng=rng_a)
            check(f"{tag} actor loss", L.scalars["train_actor/loss"], a_loss.detach())
            check(f"{tag} actor pi", ws.xa[:, -2:], pi.detach())
            assert L.scalars["train_actor/std"] == STD and "train_alpha/loss" not in L.scalars
            assert "train_actor/entropy" not in L.scalars and "train_alpha/value" not in L.scalars
            got = {k: v for k, v in taken["actor"].items() if ".convs." not in k}
            ref_g = {k: g for k, g in O._grads(a).items() if g is not None}
            assert len(got) == len(ref_g) == 10 and got["trunk.4.weight"].shape == (2, 96)
            for k, v in ref_g.items():
                check(f"{tag} actor grad {k}", got[k], v)
            params, grads_a = ({k: v for k, v in t.items() if ".convs." not in k} for t in taken["actor.raw"])
            now = dict(agent.actor.named_parameters())
            for k, v in adam_a.step(params, grads_a).items():
                check(f"{tag} actor post-step {k}", now[k], v)
            agent.soft_update_targets()
        _alpha_untouched(agent, la0)


# ------------------------------------------------------------------------------------------------- 7. whole-agent cases
DETP = dict(policy="deterministic", policy_std=STD, policy_std_clip=CLIP)
GRAPH_HP = dict(log_interval=10 ** 9, actor_update_freq=2, cpc_update_freq=1)


def _run_updates(steps, G=1, graphs=None, edit=None, dp=None, rb_kw=None, clip=None, hp=None):
    """test_gpu_utd's agent (B = 256, hidden 64, LayerNorm + dropout critics) with the deterministic policy, through
    ``steps``; ``graphs`` = dict(depth=...): update graphs, their captures counted; ``edit`` = (step, fn(agent))."""
    agent, rb, _ = _build(G, rb_kw=rb_kw, clip=clip, hp={**DETP, **(hp or {})})
    la0 = agent.log_alpha.detach().clone()
    captures, stds = [], []
    if dp is not None:
        agent.enable_data_parallel(single_rank_collectives=True, **dp)
    if graphs is not None:
        agent.enable_update_graphs(rb, warm=1, **graphs)
        agreed = agent._graph_capture_agreed

        def counted(ok):
            captures.append(bool(ok))
            return agreed(ok)
        agent._graph_capture_agreed = counted
    L = NullLogger()
    for step in steps:
        if edit is not None and step == edit[0]:
            edit[1](agent)
        agent.update(rb, L, step)
        stds.append(agent.policy_std)
    _alpha_untouched(agent, la0)
    state = _state(agent, rb)
    state["std"] = agent.actor.std.detach().cpu().clone()
    return state, dict(L.scalars), agent, captures, stds


def test_update_graphs_replay_bit_identically_under_a_std_schedule():
    """Ten updates, std changing at every one of the first six (the schedule ends at step 6): the graphed run is the
    eager run bit for bit, and its two graphs (one per kind of step, depth 1) are captured once -- at steps 3 and 4 --
    and replayed with every later std; an edit of policy_std_clip, which the launches hold by value, captures again."""
    hp = dict(policy_std_schedule=(1.0, 0.1, 6), **GRAPH_HP)
    steps = list(range(1, 11))
    eager, _, _, _, stds = _run_updates(steps, hp=hp)
    last = R.linear((1.0, 0.1, 6), 6)
    assert len(set(stds[:6])) == 6 and stds[5:] == [last] * 5 and abs(last - 0.1) < 1e-15
    graph, _, agent, captures, _ = _run_updates(steps, graphs=dict(depth=1), hp=hp)
    _assert_same_state(eager, graph)
    assert captures == [True, True], captures
    assert agent._graph_key_at_capture[-1] == ("policy", "deterministic", CLIP)
    assert float(graph["std"]) == float(np.float32(last)) and bool(torch.isfinite(graph["actor"]).all())
    flat, _, _, _, _ = _run_updates(steps, graphs=dict(depth=1), hp=GRAPH_HP)
    assert not torch.equal(flat["actor"], graph["actor"])  # (the std matters)

    def edit(a):
        a.policy_std_clip = 0.1
    e2, _, _, _, _ = _run_updates(steps, edit=(7, edit), hp=hp)
    g2, _, agent, captures, _ = _run_updates(steps, graphs=dict(depth=1), edit=(7, edit), hp=hp)
    _assert_same_state(e2, g2)
    assert agent._graph_key_at_capture[-1] == ("policy", "deterministic", 0.1) and len(captures) == 4 and all(captures)
    assert not torch.equal(g2["critic"], graph["critic"])  # (the clip matters)


def test_utd_ratio_2_is_a_critic_only_update_and_an_ordinary_one():
    steps, freq = [5, 20], 2  # (20: an actor step that logs, under test_gpu_utd's frequencies)
    hp = dict(critic_target_update_freq=freq)
    got, logged, _, _, _ = _run_updates(steps, G=2, hp=hp)
    twin, rb, _ = _build(1, hp={**DETP, **hp})
    L = NullLogger()
    for step in steps:
        twin.update(rb, NullLogger(), _lead_step(step, freq))
        twin.update(rb, L, step)
    want = _state(twin, rb)
    want["std"] = twin.actor.std.detach().cpu().clone()
    _assert_same_state(got, want)
    assert logged == L.scalars and "train_actor/std" in logged and "train_alpha/loss" not in logged
    assert float(got["critic_steps"][0]) == 4 and bool(torch.isfinite(got["critic"]).all())


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


def test_clipping_by_norm_clips_the_narrower_actor():
    got, _, agent, _, _ = _run_updates([2, 3, 4], clip=1e-4)
    stats = agent.grad_clip_stats.cpu()
    print("gradient norms and clip coefficients (critic, actor, cpc):", stats.tolist())
    assert bool(torch.isfinite(stats).all()) and float(stats[1, 0]) > 1e-4 and float(stats[1, 1]) < 1.0
    unclipped, _, _, _, _ = _run_updates([2, 3, 4])
    assert not torch.equal(unclipped["actor"], got["actor"]) and bool(torch.isfinite(got["actor"]).all())


def test_a_reset_and_a_redo_pass_leave_a_working_agent():
    np.random.seed(7)
    agent, aug = make_agent(seed=7, hidden=64)
    la0 = agent.log_alpha.detach().clone()
    rb, L = _ring(aug, B=16), NullLogger()
    for step in range(2):
        agent.update(rb, L, step)
    before = agent._actor_flat.clone()
    agent.reset_networks()
    assert agent.actor.trunk[-1].weight.shape == (2, 64) and not torch.equal(agent._actor_flat, before)
    w = agent.actor.trunk[-1].weight.detach().cpu()
    assert float((w @ w.T - torch.eye(2)).abs().max()) < 1e-5  # a freshly initialised A-row layer
    for step in range(2, 4):
        agent.update(rb, L, step)
    obs, act, _, _, _, _ = rb.sample_cpc_refs()
    agent.redo_tau = 0.5  # (a threshold that finds units to recycle)
    agent.redo_pass(obs, act)
    counts = agent.dormant_counts.cpu()
    assert counts.shape == (6,) and int(counts[4:].sum()) > 0
    for step in range(4, 7):
        agent.update(rb, L, step)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v.float()).all()) for v in _state_of(agent).values())
    assert np.isfinite(L.scalars["train_critic/loss"]) and np.isfinite(L.scalars["train_actor/loss"])
    _alpha_untouched(agent, la0)
    m = agent.select_actions(np.zeros((2, 9) + OUT_S, np.uint8))
    assert np.isfinite(m).all() and float(np.abs(m).max()) < 1.0


def test_checkpoint_resume_is_bit_for_bit(tmp_path):
    np.random.seed(5)
    sched = (0.8, 0.2, 4)
    agent, aug = make_agent(seed=5, policy_std_schedule=sched, policy_std_clip=0.25)
    rb, L = _ring(aug, B=16), NullLogger()
    for step in range(3):
        agent.update(rb, L, step)
    ck = tmp_path / "det.pt"
    agent.save_checkpoint(str(ck), 3)
    saved = torch.load(str(ck), map_location="cpu", weights_only=False)
    assert saved["policy"] == "deterministic" and saved["policy_std"] == R.linear(sched, 2) and saved["policy_std_clip"] == 0.25
    for step in range(3, 6):
        agent.update(rb, L, step)
    want = _state_of(agent)
    want["std"] = agent.actor.std.clone()

    np.random.seed(99)  # a different process state, another std, clip and no schedule: everything comes from the file
    other, aug2 = make_agent(seed=99, policy_std=0.05, policy_std_clip=None)
    rb2 = _ring(aug2, B=16)
    assert other.load_checkpoint(str(ck)) == 3
    assert other.policy_std == R.linear(sched, 2) and other.policy_std_clip == 0.25 and other.policy_std_schedule == sched
    for step in range(3, 6):
        other.update(rb2, L, step)
    torch.cuda.synchronize()
    got = _state_of(other)
    got["std"] = other.actor.std.clone()
    assert set(got) == set(want)
    for k, v in want.items():
        assert torch.equal(v, got[k]), k
    import curla_amd
    torch.manual_seed(5)
    gauss = curla_amd.CurlSacAgent((9,) + OUT_S, (2,), torch.device("cuda"), aug, hidden_dim=96, **HP)
    with pytest.raises(RuntimeError, match="size mismatch"):
        gauss.load_checkpoint(str(ck))


def test_refusals_stay_where_they_are():
    for kw, word in ((dict(critic_quantiles=5), "critic_quantiles"),
                     (dict(critic_bins=5, critic_value_range=PHASE_RANGE), "critic_bins")):
        agent, aug = make_agent(**kw)
        rb = _ring(aug, prioritized=True)
        before = (agent._critic_flat.clone(), agent._actor_flat.clone())
        with pytest.raises(ValueError, match="prioritized"):
            agent.update(rb, NullLogger(), 1)
        assert torch.equal(agent._critic_flat, before[0]) and torch.equal(agent._actor_flat, before[1])
    agent, aug = make_agent(aug_views=2)
    with pytest.raises(ValueError, match="prioritized"):  # (the buffer's own refusal)
        _ring(aug, prioritized=True, aug_views=2)
    with pytest.raises(ValueError, match="aug_views"):
        agent.update(_ring(aug, prioritized=True), NullLogger(), 1)
    agent, aug = make_agent()  # the MSE critic with a prioritized buffer works: its loss launch is the Gaussian agent's
    rb = _ring(aug, prioritized=True)
    la0 = agent.log_alpha.detach().clone()
    for step in range(4):
        agent.update(rb, NullLogger(), step)
    _alpha_untouched(agent, la0)
    assert bool(torch.isfinite(agent._critic_flat).all()) and float(np.ptp(rb.priorities())) > 0


def test_report_the_worst_errors_seen():
    """Prints, per group, the largest error against float64 that the checks of this module saw in this run (what
    DESIGN.md 7m quotes); each of them has already been held to RTOL."""
    print()
    for group, (e, name) in sorted(WORST.items()):
        print(f"worst {group}: {e:.3e} ({name})")
    assert all(e <= RTOL for e, _ in WORST.values())
