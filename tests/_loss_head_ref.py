"""Float64 statements of the SAC loss, policy-head, InfoNCE and last-layer formulas, and the input builders of
tests/test_gpu_loss_head_edges.py.  CPU only; checked by tests/test_loss_head_ref_host.py against independent autograd
statements of the same quantities.

The formulas are the reference's (curl_sac.py:20-35, 87-108, 353-359, 378-399, 411-413) as tests/test_gpu_kernels.py
(`_head_ref`, `test_losses`) and oracle/curla_oracle.py state them.  Every function takes the float32 tensors a kernel
is given and evaluates on their values cast to float64; alpha is exp(log_alpha) in double (log_alpha is a float64
scalar in the reference, curl_sac.py:292).  Besides the value, the loss functions return the magnitudes that the
tests' error bounds are relative to: the sum of |term| entering an element, or the per-row |term| of a mean."""
import math

import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64
U = 2.0 ** -24          # one float32 rounding, relative (half an ulp)
SUM_TOL = 2.0 ** -18    # scalars that are sums of B <= 1030 float32 terms, relative to the mean |term| (see scalar_bound)


def f64(x):
    return torch.as_tensor(x).detach().cpu().to(F64)


def f32c(x):
    """A Python / NumPy scalar as the float32 a kernel receives, in double."""
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------ SAC losses
def td_target(tq1, tq2, log_pi, reward, not_done, log_alpha, discount):
    """target_Q = r + not_done * discount * (min(tq1, tq2) - alpha * log_pi) (curl_sac.py:353-355).
    Returns (target, S): S = |r| + not_done * discount * (|min tq| + alpha * |log_pi|), the magnitudes entering an element."""
    tq1, tq2, log_pi, reward, not_done = (f64(t).reshape(-1) for t in (tq1, tq2, log_pi, reward, not_done))
    alpha, g = math.exp(float(log_alpha)), f32c(discount)
    mn = torch.min(tq1, tq2)
    target = reward + not_done * g * (mn - alpha * log_pi)
    S = reward.abs() + not_done.abs() * g * (mn.abs() + alpha * log_pi.abs())
    return target, S


def critic_loss(q1, q2, target):
    """loss = mse(q1, t) + mse(q2, t), dq_i = 2 (q_i - t) / B (curl_sac.py:359).
    Returns dict(loss, terms [B] = the per-row summands, dq [2, B], dq_S [2, B] = 2 (|q_i| + |t|) / B)."""
    q1, q2, t = (f64(x).reshape(-1) for x in (q1, q2, target))
    B = t.numel()
    d1, d2 = q1 - t, q2 - t
    terms = d1 * d1 + d2 * d2
    return dict(loss=terms.sum() / B, terms=terms, dq=torch.stack([2 * d1 / B, 2 * d2 / B]),
                dq_S=torch.stack([2 * (q1.abs() + t.abs()) / B, 2 * (q2.abs() + t.abs()) / B]))


def actor_alpha_loss(q1, q2, log_pi, log_std, log_alpha, target_entropy):
    """actor_loss = mean(alpha * log_pi - min(q1, q2)), alpha_loss = mean(alpha * (-log_pi - target_entropy)),
    entropy = mean(A (1 + log 2 pi) / 2 + sum_a log_std) (curl_sac.py:378-399); d(actor_loss)/dq: -1/B to the smaller
    twin, an exact tie is split -1/(2B) each (the backward of torch.min(q1, q2)); d(alpha_loss)/d(log_alpha) =
    alpha_loss (alpha = exp(log_alpha)).  `*_terms` [B]: the per-row summands of each mean."""
    q1, q2, log_pi = (f64(x).reshape(-1) for x in (q1, q2, log_pi))
    log_std = f64(log_std)
    B, A = log_pi.numel(), log_std.shape[1]
    alpha, te = math.exp(float(log_alpha)), f32c(target_entropy)
    actor_terms = alpha * log_pi - torch.min(q1, q2)
    alpha_terms = alpha * (-log_pi - te)
    ent_terms = 0.5 * A * (1.0 + math.log(2 * math.pi)) + log_std.sum(-1)
    tie = (q1 == q2).to(F64)
    dq1 = -((q1 < q2).to(F64) + 0.5 * tie) / B
    dq2 = -((q2 < q1).to(F64) + 0.5 * tie) / B
    return dict(actor_loss=actor_terms.mean(), alpha_loss=alpha_terms.mean(), entropy=ent_terms.mean(), alpha=alpha,
                dlog_alpha=alpha_terms.mean(), dq=torch.stack([dq1, dq2]), actor_terms=actor_terms,
                alpha_terms=alpha_terms, ent_terms=ent_terms)


def per_td(q1, q2, target, prob, dq_in, beta, eps, alpha):
    """Prioritized replay's weighting of the critic loss (Schaul et al. 2016; include/curla_hip.h, curla_per_td):
    w_k = (min_j P_j / P_k)^beta, dq_k *= w_k, loss = mean_k w_k ((q1_k - t_k)^2 + (q2_k - t_k)^2),
    value_k = (0.5 (|q1_k - t_k| + |q2_k - t_k|) + eps)^alpha."""
    q1, q2, t, p = (f64(x).reshape(-1) for x in (q1, q2, target, prob))
    w = (p.min() / p) ** f32c(beta)
    d1, d2 = q1 - t, q2 - t
    terms = w * (d1 * d1 + d2 * d2)
    return dict(w=w, dq=f64(dq_in).reshape(2, -1) * w, loss=terms.mean(), terms=terms,
                value=(0.5 * (d1.abs() + d2.abs()) + f32c(eps)) ** f32c(alpha))


def scalar_bound(terms):
    """|got - ref64| allowed for a float32 sum of B <= 1030 terms divided by B: 2^-18 of the mean |term|.  The longest
    chain of adds in the kernels is ceil(B / 256) <= 5 serial adds in a thread, six shuffle levels and three LDS adds
    (fifteen in the 1024-thread form), a few roundings inside each term on top: under 64 roundings of 2^-24, each
    relative to a partial sum that the mean |term| bounds.  Relative to the terms, not to the scalar: the actor loss
    cancels and can be near zero."""
    return SUM_TOL * float(f64(terms).abs().mean())


# ------------------------------------------------------------------------------------------------ policy head
def head_fwd(out2a, noise, lo, hi, dtype=F64):
    """The squashed-Gaussian head (curl_sac.py:20-35, 87-108) on the trunk output [mu | raw log_std]:
    returns dict(mu, pi, log_pi [B, 1], log_std, tanh_ls, u = the pre-squash sample), differentiable in out2a."""
    out2a = out2a if out2a.dtype == dtype else out2a.to(dtype)
    noise = torch.as_tensor(noise).detach().to(dtype)
    A = noise.shape[1]
    mu, raw = out2a.chunk(2, dim=-1)
    t = torch.tanh(raw)
    log_std = lo + 0.5 * (hi - lo) * (t + 1)
    u = mu + noise * log_std.exp()
    log_pi = (-0.5 * noise.pow(2) - log_std).sum(-1, keepdim=True) - 0.5 * math.log(2 * math.pi) * A
    mu_t, pi = torch.tanh(mu), torch.tanh(u)
    log_pi = log_pi - torch.log(F.relu(1 - pi.pow(2)) + 1e-6).sum(-1, keepdim=True)
    return dict(mu=mu_t, pi=pi, log_pi=log_pi, log_std=log_std, tanh_ls=t, u=u)


def head_bwd(out2a, noise, lo, hi, dmu=None, dpi=None, dlog_pi=None, dlog_std=None, dtype=F64):
    """d/d(out2a) of sum(dmu * mu) + sum(dpi * pi) + sum(dlog_pi * log_pi) + sum(dlog_std * log_std) for any subset of
    the four upstream gradients (None = zero), by autograd through head_fwd."""
    x = torch.as_tensor(out2a).detach().cpu().to(dtype).requires_grad_(True)
    o = head_fwd(x, noise, lo, hi, dtype)
    total = x.sum() * 0
    for g, name in ((dmu, "mu"), (dpi, "pi"), (dlog_pi, "log_pi"), (dlog_std, "log_std")):
        if g is not None:
            total = total + (torch.as_tensor(g).detach().cpu().to(dtype).reshape(o[name].shape) * o[name]).sum()
    total.backward()
    return x.grad


HEAD_SHAPES = [(1, 1), (257, 6), (33, 8), (64, 1)]  # (B, A) of the GPU file's head cases and of the host checks


def head_inputs(B, A, lo, hi, seed):
    """out2a [B, 2A] = [mu | raw] and noise [B, A] (float32) whose pre-squash sample u = mu + noise * exp(log_std) has
    |u| <= 3 or |u| >= 20 in every element, nothing in between: the reference's own log(relu(1 - pi^2) + 1e-6) is
    ill-conditioned in ANY float32 evaluation where 1 - pi^2 is near 1e-6; at |u| <= 3 it is >= 0.0098, at |u| >= 20
    below 2e-17 and both precisions give log(1e-6).  About 40 % of the elements are saturated (both signs); about 10 %
    each have raw = +20 (log_std exactly hi), raw = -20 (exactly lo), noise = 0.  u, raw and noise are chosen first (raw
    and noise as float32 values), mu = u - noise * exp(log_std) is formed in float64 and rounded; u is then re-derived
    in float64 from the rounded inputs and must still keep out of (3.001, 19.9)."""
    rs = np.random.RandomState(seed)
    sat = rs.rand(B, A) < 0.4
    sign = np.where(rs.rand(B, A) < 0.5, -1.0, 1.0)
    u = np.where(sat, sign * rs.uniform(20.0, 30.0, (B, A)), rs.uniform(-3.0, 3.0, (B, A)))
    raw = rs.randn(B, A).astype(np.float32)
    noise = rs.randn(B, A).astype(np.float32)
    kind = rs.rand(B, A)
    raw[kind < 0.1] = 20.0
    raw[(kind >= 0.1) & (kind < 0.2)] = -20.0
    noise[(kind >= 0.2) & (kind < 0.3)] = 0.0
    log_std = lo + 0.5 * (hi - lo) * (np.tanh(raw.astype(np.float64)) + 1)
    mu = (u - noise.astype(np.float64) * np.exp(log_std)).astype(np.float32)
    out2a = torch.from_numpy(np.concatenate([mu, raw], axis=1))
    noise = torch.from_numpy(noise)
    au = head_fwd(out2a, noise, lo, hi)["u"].abs()
    assert not bool(((au > 3.001) & (au < 19.9)).any()), "head_inputs: a pre-squash value between the two regimes"
    return out2a, noise


# ------------------------------------------------------------------------------------------------ loss inputs
LOG_ALPHAS = (math.log(1e-3), math.log(0.1), math.log(5.0))


def twin(a, b, stride):
    """Two [B] float32 blocks `stride` floats apart in one [2 * stride] tensor, NaN in the gaps [B, stride) of both."""
    B = a.numel()
    t = torch.full((2 * stride,), float("nan"), dtype=torch.float32)
    t[:B], t[stride:stride + B] = a.reshape(-1), b.reshape(-1)
    return t


def loss_inputs(B, stride, seed, A=2, not_done="mixed", log_alpha=LOG_ALPHAS[1]):
    """The tensors of the loss kernels at batch B (CPU, float32; log_alpha float64): q, tq as twin tensors (see twin())
    with q1 == q2 bit for bit on every 7th row and tq1 == tq2 on every 5th; log_pi, reward, not_done ("mixed", 0 or 1)
    [B]; log_std [B, A]."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    q1, q2, tq1, tq2 = r(B) * 2, r(B) * 2, r(B) * 2, r(B) * 2
    q2[::7] = q1[::7]
    tq2[::5] = tq1[::5]
    nd = (torch.rand(B, generator=g) > 0.3).float() if not_done == "mixed" else torch.full((B,), float(not_done))
    return dict(B=B, A=A, stride=stride, q1=q1, q2=q2, tq1=tq1, tq2=tq2, q=twin(q1, q2, stride), tq=twin(tq1, tq2, stride),
                log_pi=r(B) * 3 - 2, reward=r(B), not_done=nd, log_std=r(B, A) * 2 - 4,
                log_alpha=torch.tensor(log_alpha, dtype=F64))


# ------------------------------------------------------------------------------------------------ InfoNCE
def curl_ce(logits):
    """CrossEntropyLoss(logits, arange(B)) row by row and its gradient (curl_sac.py:221, 411-413):
    row_loss[a] = logsumexp(l[a, :]) - l[a, a], loss = their mean, dlogits = (softmax(l) - I) / B.
    Also the row maxima `mx` and `lse` (the bounds' magnitudes)."""
    l = f64(logits)
    B = l.shape[0]
    mx = l.max(1).values
    lse = (l - mx[:, None]).exp().sum(1).log() + mx
    p = (l - lse[:, None]).exp()
    return dict(row_loss=lse - l.diagonal(), loss=(lse - l.diagonal()).mean(), p=p,
                dlogits=(p - torch.eye(B, dtype=F64)) / B, mx=mx, lse=lse)


# ------------------------------------------------------------------------------------------------ last layer backward
def mlp_out_bwd(dy, h, W):
    """Backward of out[z] = h[z] @ W[z]^T + b[z] with the ReLU of the layer below fused (h = relu(pre)): dh = (dy @ W)
    masked by h > 0, dW = dy^T @ h, db_out = column sums of dy, db_hidden = column sums of dh.  [nb, M, N], [nb, M, K],
    [nb, N, K]."""
    dy, h, W = f64(dy), f64(h), f64(W)
    dh = torch.einsum("zmn,znk->zmk", dy, W) * (h > 0)
    return dict(dh=dh, dW=torch.einsum("zmn,zmk->znk", dy, h), db_out=dy.sum(1), db_hidden=dh.sum(1))


# ------------------------------------------------------------------------------------------------ error bounds
# Elementwise: |got - ref64| <= n * 2^-24 * S, S = the magnitudes entering the element, n = twice the float32 roundings
# on the path counted from the formula (the factor two is the margin for expf / tanhf / logf being a few ulp and not
# correctly rounded).  A library call counts as two roundings: its own approximation and the rounding of its result.
N_TARGET = 12    # alpha -> float32, alpha * log_pi, min - that, not_done * discount, * v, reward + : 6 roundings
N_CRITIC_DQ = 6  # q - t, 1 / B, 2 d * (1 / B) (the factor 2 is exact): 3 roundings; S = 2 (|q| + |t|) / B
N_ALPHA = 2      # (float)exp(log_alpha): 1 rounding
N_TANH = 4       # tanhf of an input: 2 roundings; S = |tanh|
N_LOG_STD = 12   # tanhf (2), t + 1, 0.5 * (hi - lo), the product, lo + : 6 roundings; S = |lo| + (hi - lo) / 2 * (|t| + 1)
PER_TD_TOL = 2.0 ** -20  # tests/test_gpu_per.py's bound for curla_per_td's elementwise outputs, relative


def head_fwd_bounds(ref, out2a, noise, lo, hi):
    """Elementwise bounds for the head outputs away from the log, from head_fwd's float64 result `ref`.
    pi = tanh(u), u = mu + noise * exp(log_std): log_std carries its own bound b_ls (absolute), which exp turns into a
    relative one of the product |noise| exp(log_std), plus expf (2) and the product (1), doubled: 6; the sum rounds
    once relative to at most |mu| + |noise| exp(log_std), doubled: 2; all of it reaches pi through tanh' = 1 - pi^2;
    tanhf itself is N_TANH relative to |pi| (which is all that is left where pi saturates: there tanhf must return
    exactly what float64 rounds to, +-1)."""
    mu_in = f64(out2a)[:, :noise.shape[1]]
    n = f64(noise).abs()
    t, ls, pi = ref["tanh_ls"].detach(), ref["log_std"].detach(), ref["pi"].detach()
    b_ls = N_LOG_STD * U * (abs(lo) + 0.5 * (hi - lo) * (t.abs() + 1))
    ne = n * ls.exp()
    b_u = ne * (b_ls + 6 * U) + 2 * U * (mu_in.abs() + ne)
    return dict(mu=N_TANH * U * ref["mu"].detach().abs(), tanh_ls=N_TANH * U * t.abs(), log_std=b_ls,
                pi=(1 - pi * pi) * b_u + N_TANH * U * pi.abs())


def curl_ce_bounds(ref, logits, adds=None):
    """Bounds for row_loss [B] and dlogits [B, B] from curl_ce's result.  se = sum_j exp(l_j - mx) in float32: the
    subtraction rounds by u |l_j - mx| absolute, which exp makes relative, expf adds 2 u, the sum `adds` adds -- by
    default curl_ce_kernel's ceil(B / 64) + 6 (a lane's serial adds, six shuffle levels); another kernel that evaluates
    the same formula hands in the length of its own chain (tests/_curl_head_ref.py); weighted by p_j the first is u E_p|l - mx| <= u log B (E_p[mx - l] =
    H(p) - (lse - mx) <= log B).  log turns se's relative error into an absolute one, logf adds 2 u |lse - mx|, the sum
    with mx u |lse|.  So lse is within (adds + 6) u E, E = |mx| + |lse| + 1 + log B, doubled: n_lse.
    row_loss = lse - l_aa: one more rounding, relative to at most |lse| + |l_aa|.
    dlogits = (exp(l_j - lse) - [j == a]) / B: lse's error, the subtraction (1, relative to |l_j| + |lse|) and expf (2)
    scale with p_j; then the subtraction of 1, 1 / B and the product: 3 roundings relative to (p_j + [j == a]) / B.
    A p_j below the smallest normal float32 may come out as a denormal or as zero: 2^-126 absolute on top."""
    l = f64(logits)
    B = l.shape[0]
    adds = (B + 63) // 64 + 6 if adds is None else adds
    n_lse = 2 * (adds + 6)
    E = ref["mx"].abs() + ref["lse"].abs() + 1 + math.log(B)
    eye = torch.eye(B, dtype=F64)
    row = (n_lse + 2) * U * (E + l.diagonal().abs())
    dl = ((n_lse + 6) * U * ref["p"] * (E[:, None] + l.abs()) + 6 * U * (ref["p"] + eye) + 2.0 ** -126) / B
    return dict(row_loss=row, dlogits=dl)
