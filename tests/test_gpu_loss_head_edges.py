"""The SAC loss, policy-head, last-layer-backward, InfoNCE and layout kernels at their edges, on the MI355X, against the
float64 references of tests/_loss_head_ref.py (checked on the CPU by tests/test_loss_head_ref_host.py): batch sizes
around every loop stride (64 lanes, 256 and 1024 threads, 512 rows per pass), twin tensors whose stride is not the
batch, exact ties of the twin Q values, a policy head driven into saturation and onto the log_std bounds, padded leading
dimensions, logits that overflow expf without the max subtraction.

Every output buffer is NaN before the launch and every padding region must still be NaN after it.  Bounds are derived,
not tuned (tests/_loss_head_ref.py, "error bounds"): n * 2^-24 * S element by element for short formulas, 2^-18 of the
mean |term| for the scalars that are sums over the batch, the suite's RTOL per tensor for log_pi, the head gradients
and the last layer's products.  Every measured error goes, with its bound, into the parity report that
tests/test_gpu_kernels.py keeps, through that module's own report fixture.

Measured on the MI355X (worst error / bound per group, 125 cases in 3 s): a (loss kernels) 0.50 -- dq of the actor loss,
the one rounding of 1 / B; the TD target 0.15 of its 12 roundings, the scalars at most 0.03 of 2^-18 mean |term|;
b (last layer) 0.13 -- alpha; dh / dW / db at most 6.4e-7 of RTOL; c (policy head) 0.51 -- tanh_ls, 7.0e-8 of 1.4e-7; pi
0.30, log_std 0.05 of theirs; log_pi at most 9.3e-7 and the gradients at most 3.2e-6 of RTOL = 1e-4 (the float32 CPU
evaluation: 1.0e-6 and 3.3e-6); d (curl_ce) 0.18 -- dlogits; row losses 0.03."""
import itertools
import math

import numpy as np
import pytest
import torch

from tests import _loss_head_ref as R
from tests._util import RTOL, rel_err
from tests.test_gpu_kernels import REPORT as PARITY_LINES, _report as _kernel_parity_report  # noqa: F401

pytestmark = pytest.mark.gpu

LO, HI = -10.0, 2.0
HEAD_SHAPES = R.HEAD_SHAPES
BATCHES = [1, 63, 64, 65, 255, 256, 257, 515, 1030]
GAMMA = 0.99
TAIL = 5  # NaN floats behind every dense output

REPORT = []  # (group, name, error, bound)


@pytest.fixture(scope="module", autouse=True)
def _report(_kernel_parity_report):
    """The kernel parity report's writer (imported above: it appends its module's (name, error) list to the report
    when a module that uses it is done) gets this module's lines: set up behind it, so torn down in front of it.  The
    list is emptied first: what test_gpu_kernels.py left in it has been written by then (that module runs before this
    one)."""
    del PARITY_LINES[:]
    yield
    worst = {}
    for grp, n, e, b in REPORT:
        PARITY_LINES.append((f"{grp} {n} (bound {b:.3e})", e))
        r = e / b if b > 0 else (0.0 if e == 0 else float("inf"))
        if r >= worst.get(grp, (-1.0,))[0]:
            worst[grp] = (r, n, e, b)
    for grp in sorted(worst):
        r, n, e, b = worst[grp]
        print(f"loss/head edges group {grp}: worst error / bound {r:.3f} ({n}: {e:.3e} of {b:.3e})")
        PARITY_LINES.append((f"loss/head edges group {grp}: worst error / bound, at {n}", r))


@pytest.fixture(scope="module")
def ops():
    from curla_amd import ops as o
    return o


def dev(x):
    return torch.as_tensor(x).cuda().contiguous()


def nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def all_nan(t):
    return bool(torch.isnan(t).all())


def bits_equal(a, b):
    """Equal as torch.equal has it, with the NaN of the untouched padding in the same places.  (As in the rest of the
    suite a zero's sign is not compared: the loss-in-backward launch forms dh = 0 * w where the plain one adds that
    product to +0.)"""
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(0.0), b.nan_to_num(0.0))


def record(group, name, err, bound):
    print(f"{group} {name}: {err:.3e} (bound {bound:.3e})")
    REPORT.append((group, name, float(err), float(bound)))


def within(group, name, got, ref, bound):
    """|got - ref| <= bound element by element; records the element with the worst error / bound."""
    ref = R.f64(ref)
    got, bound = R.f64(got).reshape(ref.shape), R.f64(bound).expand(ref.shape)
    assert bool(torch.isfinite(got).all()), f"{group} {name}: not finite"
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    i = int(ratio.reshape(-1).argmax()) if ratio.numel() else 0
    record(group, name, float(err.reshape(-1)[i]), float(bound.reshape(-1)[i]))
    assert bool((err <= bound).all()), f"{group} {name}: error {float(err.reshape(-1)[i]):.3e} > bound {float(bound.reshape(-1)[i]):.3e}"


def rel(group, name, got, ref, tol=RTOL):
    assert bool(torch.isfinite(torch.as_tensor(got)).all()), f"{group} {name}: not finite"
    e = rel_err(R.f64(got).reshape(R.f64(ref).shape), R.f64(ref))
    record(group, name, e, tol)
    assert e <= tol, f"{group} {name}: rel err {e:.3e} > {tol:.1e}"


def twin_gaps_nan(t, B, stride):
    return all_nan(t[B:stride]) and all_nan(t[stride + B:])


def twin_rows(t, B, stride):
    return torch.stack([t[:B], t[stride:stride + B]])


# ===================================================================================================== a. loss kernels
def _critic(ops, d, dd):
    """td_target, critic_loss and critic_td_loss on the device tensors dd of loss_inputs' d.
    Returns (target, loss, dq) of the fused launch."""
    B, stride, tag = d["B"], d["stride"], f"B{d['B']} s{d['stride']}"
    tgt = nan(B + TAIL)
    ops.td_target(dd["tq"], stride, dd["log_pi"], dd["reward"], dd["not_done"], dd["log_alpha"], GAMMA, B, tgt)
    t_ref, S = R.td_target(d["tq1"], d["tq2"], d["log_pi"], d["reward"], d["not_done"], d["log_alpha"], GAMMA)
    within("a", f"td_target {tag}", tgt[:B], t_ref, R.N_TARGET * R.U * S)
    assert all_nan(tgt[B:])
    loss, dq = nan(1 + TAIL), nan(2 * stride)
    ops.critic_loss(dd["q"], stride, tgt, B, loss, dq)
    ref = R.critic_loss(d["q1"], d["q2"], tgt[:B].cpu())  # (on the float32 target the kernel was given)
    within("a", f"critic_loss {tag}", loss[:1], ref["loss"].reshape(1), R.scalar_bound(ref["terms"]))
    within("a", f"critic_loss dq {tag}", twin_rows(dq, B, stride), ref["dq"], R.N_CRITIC_DQ * R.U * ref["dq_S"])
    assert all_nan(loss[1:]) and twin_gaps_nan(dq, B, stride)
    # one launch for both: bit-identical, padding included
    tgt2, loss2, dq2 = nan(B + TAIL), nan(1 + TAIL), nan(2 * stride)
    ops.critic_td_loss(dd["q"], dd["tq"], stride, dd["log_pi"], dd["reward"], dd["not_done"], dd["log_alpha"], GAMMA, B,
                       tgt2, loss2, dq2)
    assert bits_equal(tgt2, tgt) and bits_equal(loss2, loss) and bits_equal(dq2, dq)
    return tgt2, loss2, dq2


def _actor(ops, d, dd):
    """actor_loss on the device tensors: scalars, the exact dq, dlog_alpha.  Returns (scalars, dq, dlog_alpha)."""
    B, A, stride, tag = d["B"], d["A"], d["stride"], f"B{d['B']} s{d['stride']} A{d['A']}"
    te = -float(A)
    sc, dq, dla = nan(4 + TAIL), nan(2 * stride), torch.zeros((), dtype=torch.float64, device="cuda")
    ops.actor_loss(dd["q"], stride, dd["log_pi"], dd["log_std"], A, dd["log_alpha"], te, B, sc, dq, dla)
    ref = R.actor_alpha_loss(d["q1"], d["q2"], d["log_pi"], d["log_std"], d["log_alpha"], te)
    _actor_scalars("a", f"actor_loss {tag}", sc, dla, ref)
    assert all_nan(sc[4:]) and twin_gaps_nan(dq, B, stride)
    _actor_dq_exact(twin_rows(dq, B, stride).cpu(), d)
    within("a", f"actor_loss dq {tag}", twin_rows(dq, B, stride), ref["dq"], 2 * R.U * ref["dq"].abs())  # 1 / B: 1 rounding
    return sc, dq, dla


def _actor_scalars(group, name, sc, dla, ref):
    within(group, f"{name} actor", sc[0:1], ref["actor_loss"].reshape(1), R.scalar_bound(ref["actor_terms"]))
    within(group, f"{name} alpha", sc[1:2], ref["alpha_loss"].reshape(1), R.scalar_bound(ref["alpha_terms"]))
    within(group, f"{name} entropy", sc[2:3], ref["entropy"].reshape(1), R.scalar_bound(ref["ent_terms"]))
    within(group, f"{name} alpha value", sc[3:4], torch.tensor([ref["alpha"]], dtype=torch.float64),
           R.N_ALPHA * R.U * ref["alpha"])
    within(group, f"{name} dlog_alpha", dla.reshape(1), ref["dlog_alpha"].reshape(1), R.scalar_bound(ref["alpha_terms"]))


def _actor_dq_exact(dq, d):
    """d(-min(Q1, Q2))/dQ in float32: exactly -(1 / B) to the smaller twin and 0 to the other, exactly -0.5 * (1 / B) to
    both on a tie (every 7th row of loss_inputs)."""
    B = d["B"]
    inv = np.float32(1.0) / np.float32(B)
    q1, q2 = d["q1"].numpy(), d["q2"].numpy()
    tie = q1 == q2
    assert tie[::7].all() and int(tie.sum()) == len(range(0, B, 7))
    want = np.zeros((2, B), np.float32)
    want[0][q1 < q2], want[1][q2 < q1] = -inv, -inv
    want[:, tie] = np.float32(-0.5) * inv
    assert np.array_equal(dq.numpy(), want)


def _loss_case(ops, B, stride, A, not_done="mixed", log_alpha=R.LOG_ALPHAS[1]):
    d = R.loss_inputs(B, stride, seed=1000 + B, A=A, not_done=not_done, log_alpha=log_alpha)
    dd = {k: dev(v) for k, v in d.items() if isinstance(v, torch.Tensor)}
    _critic(ops, d, dd)
    _actor(ops, d, dd)


@pytest.mark.parametrize("A", [1, 6])
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("B", BATCHES)
def test_loss_kernels(ops, B, pad, A):
    _loss_case(ops, B, B + pad, A)


@pytest.mark.parametrize("log_alpha", R.LOG_ALPHAS, ids=["alpha1e-3", "alpha0.1", "alpha5"])
@pytest.mark.parametrize("not_done", ["mixed", 0, 1])
def test_loss_kernels_not_done_and_alpha(ops, not_done, log_alpha):
    _loss_case(ops, 257, 260, 2, not_done, log_alpha)


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("B", BATCHES)
def test_split_sum(ops, B, pad):
    """dxa [2][B][F + A], the twins `stride` floats apart -> dz, dact: one float32 addition per element, so the result
    is the correctly rounded sum, bit for bit."""
    Fd, A = 5, 2
    n = B * (Fd + A)
    stride = n + pad
    g = torch.Generator().manual_seed(B)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    dxa = dev(R.twin(a, b, stride))
    dz, da = nan(B * Fd + TAIL), nan(B * A + TAIL)
    ops.split_sum(dxa, stride, B, Fd, A, dz=dz, dact=da)
    want = (a + b).view(B, Fd + A)
    assert torch.equal(dz[:B * Fd].cpu().view(B, Fd), want[:, :Fd]) and torch.equal(da[:B * A].cpu().view(B, A), want[:, Fd:])
    assert all_nan(dz[B * Fd:]) and all_nan(da[B * A:])
    dz2 = nan(B * Fd + TAIL)
    ops.split_sum(dxa, stride, B, Fd, A, dz=dz2)  # either output alone
    assert bits_equal(dz2, dz)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1025])
def test_mean(ops, n):
    x = torch.randn(n, generator=torch.Generator().manual_seed(n)) * 3 + 1
    out = nan(1 + TAIL)
    ops.mean(dev(x), n, out)
    within("a", f"mean n{n}", out[:1], x.double().mean().reshape(1), R.scalar_bound(x))
    assert all_nan(out[1:])


@pytest.mark.parametrize("B", [65, 257])
def test_per_td_twin_stride(ops, B):
    """curla_per_td with the twins B + 3 apart (sizes: tests/test_gpu_per.py, whose 2^-20 relative bound this keeps)."""
    stride = B + 3
    d = R.loss_inputs(B, stride, seed=2000 + B)
    g = torch.Generator().manual_seed(B)
    t, prob = torch.randn(B, generator=g) * 2, torch.rand(B, generator=g) * 0.999 + 1e-3
    dq1, dq2 = torch.randn(B, generator=g), torch.randn(B, generator=g)
    beta, eps, alpha = 0.4, 1e-6, 0.6
    dq, loss, w, val = dev(R.twin(dq1, dq2, stride)), nan(1 + TAIL), nan(B + TAIL), nan(B + TAIL)
    ops.per_td(dev(d["q"]), stride, dev(t), dev(prob), beta, eps, alpha, B, dq, loss, w, val)
    ref = R.per_td(d["q1"], d["q2"], t, prob, torch.stack([dq1, dq2]), beta, eps, alpha)
    within("a", f"per_td w B{B}", w[:B], ref["w"], R.PER_TD_TOL * ref["w"].abs())
    within("a", f"per_td dq B{B}", twin_rows(dq, B, stride), ref["dq"], R.PER_TD_TOL * ref["dq"].abs())
    within("a", f"per_td value B{B}", val[:B], ref["value"], R.PER_TD_TOL * ref["value"].abs())
    within("a", f"per_td loss B{B}", loss[:1], ref["loss"].reshape(1), R.scalar_bound(ref["terms"]))
    assert twin_gaps_nan(dq, B, stride) and all_nan(loss[1:]) and all_nan(w[B:]) and all_nan(val[B:])


# ===================================================================================== b. the last layer's backward
@pytest.mark.parametrize("M,N,K,nb", [(513, 1, 64, 2), (515, 6, 100, 1), (1030, 16, 72, 2), (1025, 3, 20, 1)])
def test_mlp_out_bwd_past_one_pass(ops, M, N, K, nb):
    """More than 512 rows (a second pass over the rows) and K of 100, 72, 20 (a ragged last block of 16 columns)."""
    g = torch.Generator().manual_seed(M)
    h = torch.relu(torch.randn(nb, M, K, generator=g))
    W, dy = torch.randn(nb, N, K, generator=g) * 0.2, torch.randn(nb, M, N, generator=g)
    ref = R.mlp_out_bwd(dy, h, W)
    tag = f"{M}x{N}x{K} nb{nb}"
    pad = 8  # the twins' parameter blocks are `stride` floats apart, not dense
    sW = N * K + pad
    Wd = torch.zeros(nb, sW, device="cuda")
    Wd[:, :N * K] = dev(W).view(nb, -1)
    dh, dWd = nan(nb * M * K + TAIL), nan(nb, sW)
    ops.mlp_out_bwd(dev(dy), M * N, dev(h), M * K, Wd, sW, dh, M * K, dWd, sW, M, N, K, nb)
    rel("b", f"mlp_out dh {tag}", dh[:nb * M * K].view(nb, M, K), ref["dh"])
    rel("b", f"mlp_out dW {tag}", dWd[:, :N * K].reshape(nb, N, K), ref["dW"])
    assert all_nan(dh[nb * M * K:]) and all_nan(dWd[:, N * K:])
    dh2 = nan(nb * M * K + TAIL)
    ops.mlp_out_bwd(dev(dy), M * N, dev(h), M * K, Wd, sW, dh2, M * K, None, 0, M, N, K, nb)  # data gradient only
    assert bits_equal(dh2, dh)
    # with the two bias gradients from the same launch: db_out at 0, db_hidden at 32 of a block of S floats per twin
    S = 32 + K + 7
    for with_out, with_hidden in ((True, True), (True, False), (False, True)):
        dh3, dW3, gb = nan(nb * M * K + TAIL), nan(nb, sW), nan(nb, S)
        ops.mlp_out_bwd(dev(dy), M * N, dev(h), M * K, Wd, sW, dh3, M * K, dW3, sW, M, N, K, nb,
                        db_out=gb if with_out else None, db_hidden=gb[0, 32:] if with_hidden else None, sdb=S)
        assert bits_equal(dh3, dh) and bits_equal(dW3, dWd)
        if with_out:
            rel("b", f"mlp_out db_out {tag}", gb[:, :N], ref["db_out"])
        if with_hidden:
            rel("b", f"mlp_out db_hidden {tag}", gb[:, 32:32 + K], ref["db_hidden"])
        first, last = (N if with_out else 0), (32 + K if with_hidden else 32)  # the floats in between stay untouched
        assert all_nan(gb[:, first:32]) and all_nan(gb[:, last:])


@pytest.mark.parametrize("kind", [1, 2])
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("K", [64, 100])
@pytest.mark.parametrize("B", [257, 515, 1030])
def test_mlp_out_bwd_with_the_loss_inside(ops, B, K, pad, kind):
    """curla_mlp_out_bwd_loss: dq and the target bit-identical to the stand-alone loss kernels, dh / dW / db
    bit-identical to mlp_out_bwd fed that dq, the scalars and all of it against float64 -- past one pass of 512 rows, past
    one step of the 1024-thread scalar loops, the twins B or B + 3 apart, tie rows included."""
    stride, A = B + pad, 2
    d = R.loss_inputs(B, stride, seed=3000 + B + K, A=A)
    dd = {k: dev(v) for k, v in d.items() if isinstance(v, torch.Tensor)}
    tag = f"kind{kind} B{B} K{K} s{stride}"
    if kind == 1:
        tgt_s, _, dq_s = _critic(ops, d, dd)
        fields = dict(q=dd["q"], target_q_twin=dd["tq"], log_pi=dd["log_pi"], reward=dd["reward"], not_done=dd["not_done"],
                      discount=GAMMA)
    else:
        _, dq_s, _ = _actor(ops, d, dd)
        fields = dict(q=dd["q"], log_pi=dd["log_pi"], log_std=dd["log_std"], A=A, target_entropy=-float(A))
    g = torch.Generator().manual_seed(B + K)
    h = torch.relu(torch.randn(2, B, K, generator=g))
    S = K + 8  # a twin's block: the K weights (and gradients), then 8 floats that belong to someone else
    W = torch.randn(2, 1, K, generator=g) * 0.2
    Wf = torch.zeros(2, S, device="cuda")
    Wf[:, :K] = dev(W).view(2, K)
    hd = dev(h)
    dh_r, dW_r, gb_r = nan(2 * B * K + TAIL), nan(2, S), nan(2, S)
    ops.mlp_out_bwd(dq_s, stride, hd, B * K, Wf, S, dh_r, B * K, dW_r, S, B, 1, K, 2, db_out=gb_r, db_hidden=gb_r[0, 4:], sdb=S)
    dh_f, dW_f, gb_f = nan(2 * B * K + TAIL), nan(2, S), nan(2, S)
    dq_f, sc_f, tgt_f = nan(2 * stride), nan(4 + TAIL), nan(B + TAIL)
    dla_f = torch.zeros((), dtype=torch.float64, device="cuda")
    ops.mlp_out_bwd_loss(dict(kind=kind, twin_stride=stride, log_alpha=dd["log_alpha"], scalars=sc_f, dq=dq_f,
                              target_q=tgt_f, dlog_alpha=dla_f, **fields),
                         hd, B * K, Wf, S, dh_f, B * K, dW_f, S, B, K, db_out=gb_f, db_hidden=gb_f[0, 4:], sdb=S)
    assert bits_equal(dq_f, dq_s), "dq differs from the stand-alone loss kernel's"
    assert bits_equal(dh_f, dh_r) and bits_equal(dW_f, dW_r) and bits_equal(gb_f, gb_r)
    assert all_nan(dh_f[2 * B * K:]) and all_nan(dW_f[:, K:]) and all_nan(gb_f[:, 1:4]) and all_nan(gb_f[:, 4 + K:])
    if kind == 1:
        assert bits_equal(tgt_f, tgt_s) and all_nan(sc_f[1:])
        ref = R.critic_loss(d["q1"], d["q2"], tgt_f[:B].cpu())
        within("b", f"loss-in-backward {tag} loss", sc_f[:1], ref["loss"].reshape(1), R.scalar_bound(ref["terms"]))
    else:
        assert all_nan(tgt_f) and all_nan(sc_f[4:])
        ref = R.actor_alpha_loss(d["q1"], d["q2"], d["log_pi"], d["log_std"], d["log_alpha"], -float(A))
        _actor_scalars("b", f"loss-in-backward {tag}", sc_f, dla_f, ref)
    # (dq itself is held to float64 and, kind 2, to its exact values by the stand-alone checks above: same bits)
    dy = twin_rows(dq_f, B, stride).cpu().reshape(2, B, 1)
    ref = R.mlp_out_bwd(dy, h, W)
    rel("b", f"loss-in-backward {tag} dh", dh_f[:2 * B * K].view(2, B, K), ref["dh"])
    rel("b", f"loss-in-backward {tag} dW", dW_f[:, :K].reshape(2, 1, K), ref["dW"])
    rel("b", f"loss-in-backward {tag} db_out", gb_f[:, :1], ref["db_out"])
    rel("b", f"loss-in-backward {tag} db_hidden", gb_f[:, 4:4 + K], ref["db_hidden"])


# ============================================================================================== c. the policy head
def _head_forward(ops, out2a, noise, B, A):
    o = dict(mu=nan(B * A + TAIL), pi=nan(B * A + TAIL), log_pi=nan(B + TAIL), log_std=nan(B * A + TAIL),
             tanh_ls=nan(B * A + TAIL))
    ops.actor_head_fwd(dev(out2a), dev(noise), B, A, LO, HI, **o)
    for k, v in o.items():
        n = B if k == "log_pi" else B * A
        assert all_nan(v[n:]), k
        o[k] = v[:n].view(B, 1 if k == "log_pi" else A)
    return o


@pytest.mark.parametrize("B,A", HEAD_SHAPES)
def test_policy_head_forward_saturated(ops, B, A):
    out2a, noise = R.head_inputs(B, A, LO, HI, seed=100 + B)
    ref = R.head_fwd(out2a, noise, LO, HI)
    o = _head_forward(ops, out2a, noise, B, A)
    tag = f"B{B} A{A}"
    bounds = R.head_fwd_bounds(ref, out2a, noise, LO, HI)
    for k in ("mu", "tanh_ls", "log_std", "pi"):
        within("c", f"actor_head_fwd {k} {tag}", o[k], ref[k], bounds[k])
    rel("c", f"actor_head_fwd log_pi {tag}", o["log_pi"], ref["log_pi"])
    raw = out2a[:, A:]
    ls, tl, pi = o["log_std"].cpu(), o["tanh_ls"].cpu(), o["pi"].cpu()
    assert bool((tl[raw == 20] == 1).all()) and bool((tl[raw == -20] == -1).all())
    assert bool((ls[raw == 20] == HI).all()) and bool((ls[raw == -20] == LO).all())  # exactly on the bounds
    sat = ref["u"].abs() >= 19.9
    assert bool((pi[sat] == torch.sign(ref["u"][sat]).float()).all())  # exactly +-1, as float64 rounds it
    if B * A >= 64:
        assert int(sat.sum()) > 0.25 * B * A
    # the head inside the trunk's last-layer launch, K = 64: h holds [mu | raw] doubled in its first 2A columns and W
    # one half on that diagonal, so h @ W^T reproduces [mu | raw] exactly (products with a power of two, sums with zeros)
    K, Fz = 64, 5
    g = torch.Generator().manual_seed(B)
    h = torch.relu(torch.randn(B, K, generator=g))
    h[:, :2 * A] = 2 * out2a
    W = torch.zeros(2 * A, K)
    W[torch.arange(2 * A), torch.arange(2 * A)] = 0.5
    trunk = nan(B * 2 * A + TAIL)
    f = dict(mu=nan(B, A), pi=nan(B, A), log_pi=nan(B, 1), log_std=nan(B, A), tanh_ls=nan(B, A))
    xa = nan(B, Fz + A)
    ops.mlp_out_head_fwd(dev(h), dev(W), torch.zeros(2 * A, device="cuda"), trunk, dev(noise), B, A, K, LO, HI, xa=xa, **f)
    assert torch.equal(trunk[:B * 2 * A].cpu().view(B, 2 * A), out2a) and all_nan(trunk[B * 2 * A:])
    for k in ("mu", "pi", "log_std", "tanh_ls"):
        assert bits_equal(f[k], o[k].contiguous()), k
    rel("c", f"fused head log_pi vs the head launch {tag}", f["log_pi"], o["log_pi"].cpu(), 1e-6)
    rel("c", f"fused head log_pi {tag}", f["log_pi"], ref["log_pi"])
    assert torch.equal(xa[:, Fz:], f["pi"]) and all_nan(xa[:, :Fz])


def _exact_zeros(dout, o, A, sampled_only_mu=True):
    """What the formulas give exactly: d/dmu through a sample whose pi is exactly +-1 is 0 (1 - pi^2 == 0), d/draw at
    tanh_ls exactly +-1 is 0 (log_std sits on a bound)."""
    dout = dout.cpu()
    assert bool(torch.isfinite(dout).all())
    if sampled_only_mu:
        assert bool((dout[:, :A][o["pi"].cpu().abs() == 1] == 0).all())
    assert bool((dout[:, A:][o["tanh_ls"].cpu().abs() == 1] == 0).all())


@pytest.mark.parametrize("B,A", HEAD_SHAPES)
def test_policy_head_backward_saturated(ops, B, A):
    out2a, noise = R.head_inputs(B, A, LO, HI, seed=100 + B)
    o = _head_forward(ops, out2a, noise, B, A)
    oc = {k: v.contiguous() for k, v in o.items()}
    tag = f"B{B} A{A}"
    g = torch.Generator().manual_seed(7 * B)
    gpi = torch.randn(B, A, generator=g)
    log_alpha = torch.tensor(R.LOG_ALPHAS[1], dtype=torch.float64)
    glp = torch.full((B, 1), math.exp(R.LOG_ALPHAS[1]) / B, dtype=torch.float64)
    want = R.head_bwd(out2a, noise, LO, HI, dpi=gpi, dlog_pi=glp)
    dout = nan(B * 2 * A + TAIL)
    ops.actor_head_bwd(dev(gpi), dev(log_alpha), 1.0 / B, dev(noise), oc["pi"], oc["log_std"], oc["tanh_ls"], B, A, LO, HI,
                       dout)
    rel("c", f"actor_head_bwd {tag}", dout[:B * 2 * A].view(B, 2 * A), want)
    assert all_nan(dout[B * 2 * A:])
    _exact_zeros(dout[:B * 2 * A].view(B, 2 * A), o, A)
    assert int((o["pi"].abs() == 1).sum()) > 0 or B == 1
    # d(loss)/d(pi) read in place from the twin-Q input gradient [2][B][F + A], action columns summed over the twin
    Fz = 5
    dxa = torch.randn(2, B, Fz + A, generator=g)
    dxa[1, :, Fz:] = gpi - dxa[0, :, Fz:]
    want2 = R.head_bwd(out2a, noise, LO, HI, dpi=dxa[0, :, Fz:].double() + dxa[1, :, Fz:].double(), dlog_pi=glp)
    dout2 = nan(B * 2 * A + TAIL)
    ops.actor_head_bwd(None, dev(log_alpha), 1.0 / B, dev(noise), oc["pi"], oc["log_std"], oc["tanh_ls"], B, A, LO, HI,
                       dout2, twin_dxa=dev(dxa), F=Fz)
    rel("c", f"actor_head_bwd twin {tag}", dout2[:B * 2 * A].view(B, 2 * A), want2)
    assert all_nan(dout2[B * 2 * A:])
    _exact_zeros(dout2[:B * 2 * A].view(B, 2 * A), o, A)
    # the general backward: every subset of the four upstream gradients
    ups = dict(dmu=torch.randn(B, A, generator=g), dpi=torch.randn(B, A, generator=g),
               dlog_pi=torch.randn(B, 1, generator=g), dlog_std=torch.randn(B, A, generator=g))
    for subset in itertools.product((0, 1), repeat=4):
        kw = {k: v for (k, v), on in zip(ups.items(), subset) if on}
        want = R.head_bwd(out2a, noise, LO, HI, **kw)
        dk = {k: (dev(v) if k in kw else None) for k, v in ups.items()}
        d3 = nan(B * 2 * A + TAIL)
        ops.policy_head_bwd(dk["dmu"], dk["dpi"], dk["dlog_pi"], dk["dlog_std"], dev(noise), oc["mu"], oc["pi"],
                            oc["log_std"], oc["tanh_ls"], B, A, LO, HI, d3)
        got = d3[:B * 2 * A].view(B, 2 * A)
        rel("c", f"policy_head_bwd {''.join(map(str, subset))} {tag}", got, want)
        assert all_nan(d3[B * 2 * A:])
        _exact_zeros(got, o, A, sampled_only_mu="dmu" not in kw)
        if not kw:
            assert not bool(got.any())


# ======================================================================================================= d. curl_ce
@pytest.mark.parametrize("scale", [3.0, 40.0])
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("B", [1, 3, 65, 130])
def test_curl_ce_edges(ops, B, pad, scale):
    ld = B + pad
    logits = torch.randn(B, B, generator=torch.Generator().manual_seed(B)) * scale
    ref = R.curl_ce(logits)
    bounds = R.curl_ce_bounds(ref, logits)
    lg = torch.full((B, ld), float("nan"))
    lg[:, :B] = logits
    rl, loss, dl = nan(B + TAIL), nan(1 + TAIL), nan(B, ld)
    ops.curl_ce(dev(lg), B, ld, rl, loss, dl)
    tag = f"B{B} ld{ld} x{scale:g}"
    within("d", f"curl_ce row_loss {tag}", rl[:B], ref["row_loss"], bounds["row_loss"])
    within("d", f"curl_ce dlogits {tag}", dl[:, :B], ref["dlogits"], bounds["dlogits"])
    # the mean of the float32 row losses: their own errors on average, and the sum's
    within("d", f"curl_ce loss {tag}", loss[:1], ref["loss"].reshape(1),
           float(bounds["row_loss"].mean()) + R.scalar_bound(ref["row_loss"]))
    assert all_nan(rl[B:]) and all_nan(loss[1:]) and all_nan(dl[:, B:])
    if B == 1:
        assert float(rl[0]) == 0.0 and float(loss[0]) == 0.0 and float(dl[0, 0]) == 0.0


# ================================================================================================== e. nhwc_to_nchw
@pytest.mark.parametrize("shape", [(2, 5, 7, 32), (3, 1, 9, 12)])
def test_nhwc_to_nchw(ops, shape):
    B, H, W, C = shape
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(C))
    n = x.numel()
    out = nan(n + TAIL)
    ops.nhwc_to_nchw(dev(x), out)
    assert torch.equal(out[:n].cpu().view(B, C, H, W), x.permute(0, 3, 1, 2)) and all_nan(out[n:])


# =============================================================================================== argument checks
def test_twin_stride_below_the_batch_fails_loudly(ops):
    """A twin stride shorter than one twin's block is refused on the host, before any launch."""
    from curla_amd._lib import CurlaHipError
    B, A, Fd = 8, 2, 5
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    la, dla = torch.zeros((), dtype=torch.float64, device="cuda"), torch.zeros((), dtype=torch.float64, device="cuda")
    bad = B - 1
    calls = [
        lambda: ops.td_target(z(2 * B), bad, z(B), z(B), z(B), la, GAMMA, B, z(B)),
        lambda: ops.critic_loss(z(2 * B), bad, z(B), B, z(1), z(2 * B)),
        lambda: ops.critic_td_loss(z(2 * B), z(2 * B), bad, z(B), z(B), z(B), la, GAMMA, B, z(B), z(1), z(2 * B)),
        lambda: ops.actor_loss(z(2 * B), bad, z(B), z(B, A), A, la, -2.0, B, z(4), z(2 * B), dla),
        lambda: ops.split_sum(z(2 * B * (Fd + A)), B * (Fd + A) - 1, B, Fd, A, dz=z(B, Fd), dact=z(B, A)),
        lambda: ops.per_td(z(2 * B), bad, z(B), z(B) + 0.5, 0.4, 1e-6, 0.6, B, z(2 * B), z(1), z(B), z(B)),
        lambda: ops.mlp_out_bwd_loss(dict(kind=2, A=A, twin_stride=bad, q=z(2 * B), log_pi=z(B), log_std=z(B, A),
                                          log_alpha=la, scalars=z(4), dq=z(2 * B), target_entropy=-2.0),
                                     z(2, B, 16), B * 16, z(2, 16), 16, z(2, B, 16), B * 16, z(2, 16), 16, B, 16),
    ]
    for c in calls:
        with pytest.raises(CurlaHipError):
            c()
    torch.cuda.synchronize()
