"""The categorical HL-Gauss critic (Imani & White 2018; Farebrother et al. 2024) as DESIGN.md 7l defines it, in torch
float64 with autograd: what csrc/hlgauss.h and the agent's bins phases are held to.  Inputs are taken as they are
(float32 values are cast up, never rounded again).

  w = (v_max - v_min) / M,  e_j = v_min + j w (j = 0 .. M),  c_j = v_min + (j + 1/2) w,  sigma = bin_sigma w
  Q = sum_j softmax(l)_j c_j,  Phi(x) = (1 + erf(x / sqrt 2)) / 2,  alpha = float32(exp(log_alpha))
Critic, per row b:
  y = reward + not_done * discount * (min(Q'_0, Q'_1) - alpha * log_pi);  views (H = B / 2): positions p and p + H both
  take 0.5 (y_p + y_{p+H});  y <- clamp(y, v_min, v_max)
  t_j = (Phi((e_{j+1} - y) / sigma) - Phi((e_j - y) / sigma)) / (Phi((e_M - y) / sigma) - Phi((e_0 - y) / sigma))
  row_loss[b] = -sum_n sum_j t_j log_softmax(q[n][b])_j,  loss = sum_b row_loss[b] / N,  N = B (H with views)
Actor:
  actor_loss = mean_b(alpha log_pi_b - min(Q_0, Q_1)): torch.min's backward gives the smaller network the gradient and
  splits it on an exact tie."""
import math

import numpy as np
import torch

from tests._tqc_ref import alpha_of


def _f64(t):
    return torch.as_tensor(t).to(torch.float64)


def grid(M, v_min, v_max):
    """(w, edges [M + 1], centres [M]) in float64."""
    w = (float(v_max) - float(v_min)) / M
    j = torch.arange(M + 1, dtype=torch.float64)
    return w, float(v_min) + j * w, float(v_min) + (j[:M] + 0.5) * w


def expected(logits, M, v_min, v_max):
    """Q = sum_j softmax(logits)_j c_j over the last dim."""
    return (torch.softmax(_f64(logits), dim=-1) * grid(M, v_min, v_max)[2]).sum(-1)


def target_probs(y, M, v_min, v_max, sigma):
    """t [B, M] of the (already clamped) targets y [B]."""
    _, e, _ = grid(M, v_min, v_max)
    cdf = 0.5 * (1 + torch.erf((e[None, :] - _f64(y).reshape(-1, 1)) / (float(sigma) * math.sqrt(2.0))))
    return (cdf[:, 1:] - cdf[:, :-1]) / (cdf[:, -1:] - cdf[:, :1])


def critic_loss(q, tq, log_pi, reward, not_done, log_alpha, discount, v_min, v_max, sigma, views=False):
    """q, tq [2, B, M] logits; log_pi, reward, not_done [B] (or [B, 1]); ``sigma`` the smoothing's standard deviation
    itself.  Returns dict(loss, dq [2, B, M], row_loss [B], target_q [B] (clamped), y_raw [B], t [B, M]); ``q`` may be
    part of a graph (requires_grad): then ``loss`` is differentiable and dq is None."""
    in_graph = torch.is_tensor(q) and q.requires_grad
    l = _f64(q) if in_graph else _f64(q).detach().clone().requires_grad_(True)
    tq = _f64(tq).detach()
    _, B, M = l.shape
    log_pi, reward, not_done = (_f64(t).detach().reshape(B) for t in (log_pi, reward, not_done))
    qt = expected(tq, M, v_min, v_max)                                               # [2, B]
    y = reward + not_done * float(discount) * (torch.minimum(qt[0], qt[1]) - alpha_of(log_alpha) * log_pi)
    N = B
    if views:
        assert B % 2 == 0
        N = B // 2
        y = (0.5 * (y[:N] + y[N:])).repeat(2)
    yc = y.clamp(float(v_min), float(v_max))
    t = target_probs(yc, M, v_min, v_max, sigma)
    rows = -(t[None] * torch.log_softmax(l, dim=-1)).sum(dim=(0, 2))                 # [B]
    loss = rows.sum() / N
    out = dict(loss=loss, row_loss=rows.detach(), target_q=yc, y_raw=y, t=t, dq=None)
    if not in_graph:
        loss.backward()
        out["dq"], out["loss"] = l.grad.detach(), loss.detach()
    return out


def critic_loss_loops(q, tq, log_pi, reward, not_done, log_alpha, discount, v_min, v_max, sigma, views=False):
    """The same definition as plain Python loops on Python floats: (loss, dq [2, B, M], row_loss [B], t [B, M])."""
    q, tq = np.asarray(q, dtype=np.float64), np.asarray(tq, dtype=np.float64)
    _, B, M = q.shape
    alpha = float(alpha_of(log_alpha))
    log_pi, reward, not_done = (np.asarray(x, dtype=np.float64).reshape(B) for x in (log_pi, reward, not_done))
    v_min, v_max, sigma = float(v_min), float(v_max), float(sigma)
    w = (v_max - v_min) / M
    Phi = lambda x: 0.5 * (1.0 + math.erf(x / math.sqrt(2.0)))  # noqa: E731

    def softmax(row):
        m = max(row)
        ex = [math.exp(v - m) for v in row]
        s = sum(ex)
        return [v / s for v in ex], m + math.log(s)

    def q_of(row):
        p, _ = softmax([float(v) for v in row])
        return sum(p[j] * (v_min + (j + 0.5) * w) for j in range(M))

    ys = [float(reward[b]) + float(not_done[b]) * discount * (min(q_of(tq[0, b]), q_of(tq[1, b])) - alpha * float(log_pi[b]))
          for b in range(B)]
    N = B
    if views:
        N = B // 2
        ys = [0.5 * (ys[b % N] + ys[b % N + N]) for b in range(B)]
    dq, rows, ts, total = np.zeros((2, B, M)), np.zeros(B), np.zeros((B, M)), 0.0
    for b in range(B):
        y = min(max(ys[b], v_min), v_max)
        z = Phi((v_min + M * w - y) / sigma) - Phi((v_min - y) / sigma)
        t = [(Phi((v_min + (j + 1) * w - y) / sigma) - Phi((v_min + j * w - y) / sigma)) / z for j in range(M)]
        ts[b] = t
        for n in range(2):
            p, lse = softmax([float(v) for v in q[n, b]])
            for j in range(M):
                rows[b] -= t[j] * (float(q[n, b, j]) - lse)
                dq[n, b, j] = (p[j] - t[j]) / N
        total += rows[b]
    return total / N, dq, rows, ts


def actor_loss(q, log_pi, log_std, log_alpha, target_entropy, v_min, v_max):
    """q [2, B, M] logits, log_pi [B] (or [B, 1]), log_std [B, A].  Returns dict(scalars [actor_loss, alpha_loss,
    entropy, alpha], dq [2, B, M], dlog_alpha, q_values [2, B]); ``q`` / ``log_pi`` in a graph: ``actor_loss`` /
    ``alpha_loss`` stay differentiable (alpha_loss in a float64 ``log_alpha`` that requires grad) and dq is None."""
    in_graph = torch.is_tensor(q) and q.requires_grad
    l = _f64(q) if in_graph else _f64(q).detach().clone().requires_grad_(True)
    _, B, M = l.shape
    lp = _f64(log_pi).reshape(B)
    alpha = alpha_of(log_alpha)
    qv = expected(l, M, v_min, v_max)
    a_loss = (alpha * lp - torch.min(qv[0], qv[1])).mean()
    A = log_std.shape[1]
    entropy = (0.5 * A * (1.0 + np.log(2 * np.pi)) + _f64(log_std).detach().sum(-1)).mean()
    c = (-lp.detach() - float(target_entropy)).mean()
    if in_graph:
        la = log_alpha if torch.is_tensor(log_alpha) and log_alpha.requires_grad else _f64(log_alpha)
        return dict(actor_loss=a_loss, alpha_loss=la.exp() * c, entropy=entropy, alpha=alpha, dq=None)
    a_loss.backward()
    return dict(scalars=torch.stack([a_loss.detach(), alpha * c, entropy, alpha]), dq=l.grad.detach(),
                dlog_alpha=alpha * c, actor_loss=a_loss.detach(), alpha_loss=alpha * c, entropy=entropy, alpha=alpha,
                q_values=qv.detach())


def actor_loss_loops(q, log_pi, log_alpha, v_min, v_max):
    """The actor loss and dq of the definition as plain loops: the smaller network takes -1 / B, a tie splits it."""
    q = np.asarray(q, dtype=np.float64)
    _, B, M = q.shape
    alpha = float(alpha_of(log_alpha))
    lp = np.asarray(log_pi, dtype=np.float64).reshape(B)
    w = (float(v_max) - float(v_min)) / M
    c = [float(v_min) + (j + 0.5) * w for j in range(M)]
    total, dq = 0.0, np.zeros((2, B, M))
    for b in range(B):
        ps, qs = [], []
        for n in range(2):
            m = max(q[n, b])
            ex = [math.exp(float(v) - m) for v in q[n, b]]
            p = [v / sum(ex) for v in ex]
            ps.append(p)
            qs.append(sum(p[j] * c[j] for j in range(M)))
        total += alpha * float(lp[b]) - min(qs)
        for n in range(2):
            g = -1.0 / B if qs[n] < qs[1 - n] else (-0.5 / B if qs[0] == qs[1] else 0.0)
            for j in range(M):
                dq[n, b, j] = g * ps[n][j] * (c[j] - qs[n])
    return total / B, dq
