"""tests/_loss_head_ref.py checked on the CPU: every float64 reference against an independent float64 autograd statement
built from torch primitives (F.mse_loss, F.cross_entropy, torch.min, torch.distributions.Normal), the input builders'
conditions at every shape tests/test_gpu_loss_head_edges.py uses, and the derived bounds shown passable by a correct
float32 evaluation (torch on the CPU) before any kernel is involved."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _loss_head_ref as R
from tests._util import RTOL, rel_err

F64 = torch.float64
LO, HI = -10.0, 2.0
HEAD_SHAPES = R.HEAD_SHAPES  # every (B, A) tests/test_gpu_loss_head_edges.py runs the head at
EXACT = 1e-13  # two float64 statements of one formula


def _same(a, b, what):
    a, b = R.f64(a), R.f64(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(float(b.abs().max()), 1e-300)
    assert float((a - b).abs().max()) <= EXACT * scale, (what, float((a - b).abs().max()), scale)


@pytest.mark.parametrize("B", [1, 65, 257])
def test_critic_and_target_against_autograd(B):
    d = R.loss_inputs(B, B + 3, seed=B)
    target, S = R.td_target(d["tq1"], d["tq2"], d["log_pi"], d["reward"], d["not_done"], d["log_alpha"], 0.99)
    alpha = d["log_alpha"].exp()
    g = float(np.float32(0.99))
    want = d["reward"].double() + d["not_done"].double() * g * (torch.min(d["tq1"].double(), d["tq2"].double())
                                                               - alpha * d["log_pi"].double())
    _same(target, want, "td target")
    assert bool((S >= target.abs() - 1e-12).all())  # the magnitudes bound the value
    q = torch.stack([d["q1"], d["q2"]]).double().requires_grad_(True)
    loss = F.mse_loss(q[0], want) + F.mse_loss(q[1], want)
    loss.backward()
    ref = R.critic_loss(d["q1"], d["q2"], want)
    _same(ref["loss"], loss, "critic loss")
    _same(ref["dq"], q.grad, "critic dq")
    _same(ref["terms"].sum() / B, loss, "critic terms")
    assert bool((ref["dq_S"] >= ref["dq"].abs()).all())


def test_td_target_by_hand():
    # r + nd * g * (min - alpha * lp), alpha = exp(log 0.5) = 0.5, g = 0.5: 1 + 0.5 * (-2 - 0.5 * 4) = -1; nd = 0: r
    t, S = R.td_target(torch.tensor([-2.0, 3.0]), torch.tensor([5.0, 1.0]), torch.tensor([4.0, 4.0]),
                       torch.tensor([1.0, 7.0]), torch.tensor([1.0, 0.0]), torch.tensor(math.log(0.5), dtype=F64), 0.5)
    assert torch.allclose(t, torch.tensor([-1.0, 7.0], dtype=F64), rtol=0, atol=1e-15)
    assert torch.allclose(S, torch.tensor([1 + 0.5 * (2 + 2), 7.0], dtype=F64), rtol=0, atol=1e-15)


@pytest.mark.parametrize("B,A", [(1, 1), (70, 2), (257, 6)])
def test_actor_and_alpha_against_autograd(B, A):
    d = R.loss_inputs(B, B, seed=3 * B, A=A)
    te = -float(A)
    q = torch.stack([d["q1"], d["q2"]]).double().requires_grad_(True)
    la = d["log_alpha"].clone().requires_grad_(True)
    lp = d["log_pi"].double()
    actor_loss = (la.exp().detach() * lp - torch.min(q[0], q[1])).mean()  # torch.min's backward halves a tie
    actor_loss.backward()
    alpha_loss = (la.exp() * (-lp - te).detach()).mean()
    alpha_loss.backward()
    ent = (0.5 * A * (1.0 + np.log(2 * np.pi)) + d["log_std"].double().sum(-1)).mean()
    ref = R.actor_alpha_loss(d["q1"], d["q2"], d["log_pi"], d["log_std"], d["log_alpha"], te)
    _same(ref["actor_loss"], actor_loss, "actor loss")
    _same(ref["alpha_loss"], alpha_loss, "alpha loss")
    _same(ref["entropy"], ent, "entropy")
    _same(ref["dq"], q.grad, "actor dq")
    _same(ref["dlog_alpha"], la.grad, "dlog_alpha")
    _same(torch.tensor(ref["alpha"], dtype=F64), la.exp(), "alpha")
    ties = torch.arange(B) % 7 == 0
    assert bool((ref["dq"][:, ties] == -0.5 / B).all())  # -1/(2B) to both twins
    assert bool(((ref["dq"][:, ~ties] == -1.0 / B) | (ref["dq"][:, ~ties] == 0)).all())
    assert bool((ref["dq"].sum(0) == -1.0 / B).all())


def test_per_td_against_autograd():
    B = 65
    d = R.loss_inputs(B, B, seed=11)
    g = torch.Generator().manual_seed(5)
    prob = torch.rand(B, generator=g) * 0.9 + 1e-3
    t = torch.randn(B, generator=g)
    base = R.critic_loss(d["q1"], d["q2"], t)
    ref = R.per_td(d["q1"], d["q2"], t, prob, base["dq"].float(), 0.4, 1e-6, 0.6)
    q = torch.stack([d["q1"], d["q2"]]).double().requires_grad_(True)
    w = (prob.double().min() / prob.double()) ** float(np.float32(0.4))
    loss = (w * ((q[0] - t.double()) ** 2 + (q[1] - t.double()) ** 2)).mean()
    loss.backward()
    _same(ref["w"], w, "w")
    _same(ref["loss"], loss, "weighted loss")
    # the weighted loss's gradient is the unweighted one's times w (to the float32 rounding of the dq handed in)
    assert rel_err(ref["dq"], q.grad) <= 2.0 ** -23
    assert float(ref["w"].max()) == 1.0 and bool((ref["value"] > 0).all())


@pytest.mark.parametrize("scale", [3.0, 40.0])
@pytest.mark.parametrize("B", [1, 3, 65, 130])
def test_curl_ce_against_cross_entropy(B, scale):
    logits = torch.randn(B, B, generator=torch.Generator().manual_seed(B)) * scale
    l = logits.double().requires_grad_(True)
    rows = F.cross_entropy(l, torch.arange(B), reduction="none")
    rows.mean().backward()
    ref = R.curl_ce(logits)
    _same(ref["row_loss"], rows, "row losses")
    _same(ref["loss"], rows.mean(), "loss")
    assert float((ref["dlogits"] - l.grad).abs().max()) <= EXACT  # (entries are at most 1; lse is up to 2e2)
    if B == 1:
        assert float(ref["row_loss"][0]) == 0.0 and float(ref["dlogits"][0, 0]) == 0.0
    # a correct float32 evaluation passes the bounds
    b = R.curl_ce_bounds(ref, logits)
    l32 = logits.clone().requires_grad_(True)
    rows32 = F.cross_entropy(l32, torch.arange(B), reduction="none")
    rows32.mean().backward()
    assert bool(((rows32.detach().double() - ref["row_loss"]).abs() <= b["row_loss"]).all())
    assert bool(((l32.grad.double() - ref["dlogits"]).abs() <= b["dlogits"]).all())
    if scale == 40.0 and B >= 65:  # what the max subtraction is for: expf of these overflows
        assert float(logits.max()) > 89.0


def _head_by_distribution(x, noise, lo, hi):
    """The head again, through torch.distributions: log_pi = Normal(mu, std).log_prob(mu + std noise) summed, minus
    the squash correction."""
    A = noise.shape[1]
    mu, raw = x[:, :A], x[:, A:]
    log_std = lo + 0.5 * (hi - lo) * (torch.tanh(raw) + 1)
    std = log_std.exp()
    u = mu + std * noise
    # (the sample's dependence on mu and std cancels inside log_prob exactly as in the reference's residual form)
    logp = torch.distributions.Normal(mu, std).log_prob(mu + (std * noise)).sum(-1, keepdim=True)
    pi = torch.tanh(u)
    return dict(mu=torch.tanh(mu), pi=pi, log_std=log_std,
                log_pi=logp - torch.log(torch.clamp(1 - pi * pi, min=0) + 1e-6).sum(-1, keepdim=True))


SUBSETS = [s for s in [(a, b, c, d) for a in (0, 1) for b in (0, 1) for c in (0, 1) for d in (0, 1)] if any(s)]


@pytest.mark.parametrize("B,A", HEAD_SHAPES)
def test_head_against_the_distribution_form(B, A):
    out2a, noise = R.head_inputs(B, A, LO, HI, seed=100 + B)
    ref = R.head_fwd(out2a, noise, LO, HI)
    # log_prob's (x - mu)^2 / (2 var) is noise^2 / 2 only to rounding, and mu is up to 2e2: compare at 1e-9 of the scale
    alt = _head_by_distribution(out2a.double(), noise.double(), LO, HI)
    for k in ("mu", "pi", "log_std"):
        _same(ref[k], alt[k], k)
    assert rel_err(ref["log_pi"], alt["log_pi"]) <= 1e-9
    g = torch.Generator().manual_seed(B)
    ups = dict(dmu=torch.randn(B, A, generator=g), dpi=torch.randn(B, A, generator=g),
               dlog_pi=torch.randn(B, 1, generator=g), dlog_std=torch.randn(B, A, generator=g))
    for s in SUBSETS:
        kw = {k: v for (k, v), on in zip(ups.items(), s) if on}
        got = R.head_bwd(out2a, noise, LO, HI, **kw)
        x = out2a.double().requires_grad_(True)
        o = _head_by_distribution(x, noise.double(), LO, HI)
        sum((v.double() * o[k[1:]]).sum() for k, v in kw.items()).backward()
        assert bool(torch.isfinite(got).all())
        assert rel_err(got, x.grad) <= 1e-9, s


@pytest.mark.parametrize("B,A", HEAD_SHAPES)
def test_head_inputs_conditions_and_float32_passes_the_bounds(B, A):
    out2a, noise = R.head_inputs(B, A, LO, HI, seed=100 + B)
    assert out2a.dtype == torch.float32 and noise.dtype == torch.float32
    ref = R.head_fwd(out2a, noise, LO, HI)
    au = ref["u"].abs()
    assert int(((au > 3.001) & (au < 19.9)).sum()) == 0  # the cap: no in-between element
    raw = out2a[:, A:]
    if B * A >= 64:
        n = B * A
        assert 0.25 * n <= int((au >= 19.9).sum()) <= 0.55 * n
        assert int((ref["u"] >= 19.9).sum()) > 0 and int((ref["u"] <= -19.9).sum()) > 0
        for what in (raw == 20, raw == -20, noise == 0):
            assert 0.03 * n <= int(what.sum()) <= 0.2 * n
    assert bool((ref["log_std"][raw == 20] == HI).all()) and bool((ref["log_std"][raw == -20] == LO).all())
    assert bool((ref["pi"].abs()[au >= 19.9] == 1.0).all())  # float64 saturates there too
    # float32 on the CPU: finite, pi exactly +-1 on the saturated elements, inside every bound of the GPU test
    f32 = R.head_fwd(out2a, noise, LO, HI, dtype=torch.float32)
    assert all(bool(torch.isfinite(v).all()) for v in f32.values())
    assert bool((f32["pi"].abs()[au >= 19.9] == 1.0).all())
    bounds = R.head_fwd_bounds(ref, out2a, noise, LO, HI)
    for k, b in bounds.items():
        err = (f32[k].double() - ref[k]).abs()
        assert bool((err <= b).all()), (k, float((err / b.clamp_min(1e-300)).max()))
    e = rel_err(f32["log_pi"], ref["log_pi"])
    print(f"float32 CPU head B{B} A{A}: log_pi rel err {e:.2e}")
    assert e <= RTOL
    g = torch.Generator().manual_seed(B)
    gpi = torch.randn(B, A, generator=g)
    glp = torch.full((B, 1), 0.1 / B)
    want = R.head_bwd(out2a, noise, LO, HI, dpi=gpi, dlog_pi=glp)
    got = R.head_bwd(out2a, noise, LO, HI, dpi=gpi, dlog_pi=glp, dtype=torch.float32)
    assert bool(torch.isfinite(got).all())
    e = rel_err(got, want)
    print(f"float32 CPU head B{B} A{A}: gradient rel err {e:.2e}")
    assert e <= RTOL
    # what the formulas give exactly: no gradient to mu through a saturated sample, none to raw at the log_std bounds
    assert bool((want[:, :A][ref["pi"].abs() == 1.0] == 0).all())
    assert bool((want[:, A:][ref["tanh_ls"].abs() == 1.0] == 0).all())


@pytest.mark.parametrize("B", [1, 257, 1030])
def test_loss_inputs_conditions(B):
    for stride in (B, B + 3):
        d = R.loss_inputs(B, stride, seed=B)
        assert d["q"].numel() == 2 * stride
        assert torch.equal(d["q"][:B], d["q1"]) and torch.equal(d["q"][stride:stride + B], d["q2"])
        assert bool(torch.isnan(d["q"][B:stride]).all()) and bool(torch.isnan(d["q"][stride + B:]).all())
        assert bool(torch.isnan(d["tq"][B:stride]).all())
        ties, tties = torch.arange(B) % 7 == 0, torch.arange(B) % 5 == 0
        assert torch.equal(d["q1"][ties].view(torch.int32), d["q2"][ties].view(torch.int32))
        assert torch.equal(d["tq1"][tties].view(torch.int32), d["tq2"][tties].view(torch.int32))
        assert not bool((d["q1"][~ties] == d["q2"][~ties]).any())
    for nd, want in (("mixed", None), (0, 0.0), (1, 1.0)):
        got = R.loss_inputs(257, 257, seed=1, not_done=nd)["not_done"]
        if want is None:
            assert 0 < float(got.sum()) < 257 and set(got.tolist()) == {0.0, 1.0}
        else:
            assert bool((got == want).all())
    assert [round(math.exp(a), 6) for a in R.LOG_ALPHAS] == [1e-3, 0.1, 5.0]


@pytest.mark.parametrize("M,N,K,nb", [(7, 1, 5, 2), (33, 6, 20, 1)])
def test_mlp_out_bwd_against_autograd(M, N, K, nb):
    g = torch.Generator().manual_seed(M)
    pre = torch.randn(nb, M, K, generator=g)
    W, dy = torch.randn(nb, N, K, generator=g), torch.randn(nb, M, N, generator=g)
    pre64 = pre.double().requires_grad_(True)
    W64, b64 = W.double().requires_grad_(True), torch.zeros(nb, N, dtype=F64, requires_grad=True)
    bh64 = torch.zeros(nb, K, dtype=F64, requires_grad=True)  # the bias of the layer below
    out = torch.einsum("zmk,znk->zmn", torch.relu(pre64 + bh64[:, None, :]), W64) + b64[:, None, :]
    (out * dy.double()).sum().backward()
    ref = R.mlp_out_bwd(dy, torch.relu(pre), W)
    _same(ref["dh"], pre64.grad, "dh")
    _same(ref["dW"], W64.grad, "dW")
    _same(ref["db_out"], b64.grad, "db_out")
    _same(ref["db_hidden"], bh64.grad, "db_hidden")
