"""Truncated quantile critics (Kuznetsov et al., ICML 2020) as DESIGN.md 7h defines them, in torch float64 with autograd:
what csrc/tqc.h and the agent's quantile phases are held to.  Inputs are taken as they are (float32 values are cast up,
never rounded again).

Per row b, with theta[n][b][i] the critic's atoms, z[n][b][i] the target critic's, alpha = float32(exp(log_alpha)):
  tau_i = (2 i + 1) / (2 M),  K = 2 (M - d)
  z'_(0..K-1): the K smallest of the row's 2M pooled target atoms
  y_j = reward + not_done * discount * (z'_(j) - alpha * log_pi)
  u = y_j - theta[n][i],  h(u) = 0.5 u^2 if |u| <= 1 else |u| - 0.5,  w = |tau_i - [u < 0]|
  loss = mean over (b, n, i, j) of w h(u)
  actor_loss = mean_b(alpha log_pi_b - mean_{n,i} theta[n][b][i])"""
import numpy as np
import torch


def alpha_of(log_alpha):
    """float32(exp(log_alpha)) of the float64 log_alpha, as a float64 tensor: the kernels' alpha."""
    la = torch.as_tensor(log_alpha, dtype=torch.float64).detach()
    return la.exp().to(torch.float32).to(torch.float64)


def critic_loss(theta, z, log_pi, reward, not_done, log_alpha, discount, d):
    """theta, z [2, B, M]; log_pi, reward, not_done [B] (or [B, 1]).  Returns dict(loss, dq [2, B, M], row_loss [B],
    y [B, K]); ``theta`` may itself be part of a graph (requires_grad): then ``loss`` is differentiable and dq is None."""
    f64 = lambda t: torch.as_tensor(t).to(torch.float64)  # noqa: E731
    in_graph = torch.is_tensor(theta) and theta.requires_grad
    th = f64(theta) if in_graph else f64(theta).detach().clone().requires_grad_(True)
    z = f64(z).detach()
    _, B, M = th.shape
    K = 2 * (M - d)
    log_pi, reward, not_done = (f64(t).detach().reshape(B, 1) for t in (log_pi, reward, not_done))
    pooled = z.permute(1, 0, 2).reshape(B, 2 * M)
    kept = torch.sort(pooled, dim=1).values[:, :K]                                  # [B, K]
    y = reward + not_done * float(discount) * (kept - alpha_of(log_alpha) * log_pi)  # [B, K]
    tau = (2 * torch.arange(M, dtype=torch.float64) + 1) / (2 * M)
    u = y[:, None, None, :] - th.permute(1, 0, 2)[:, :, :, None]                    # [B, 2, M, K]
    au = u.abs()
    huber = torch.where(au <= 1, 0.5 * u * u, au - 0.5)
    w = (tau[None, None, :, None] - (u.detach() < 0).to(torch.float64)).abs()
    terms = w * huber
    loss = terms.mean()
    out = dict(loss=loss, row_loss=terms.detach().mean(dim=(1, 2, 3)), y=y, dq=None)
    if not in_graph:
        loss.backward()
        out["dq"], out["loss"] = th.grad.detach(), loss.detach()
    return out


def critic_loss_loops(theta, z, log_pi, reward, not_done, log_alpha, discount, d):
    """The same definition as plain Python loops over (b, n, i, j) on Python floats: (loss, dq as nested lists)."""
    theta, z = np.asarray(theta, dtype=np.float64), np.asarray(z, dtype=np.float64)
    _, B, M = theta.shape
    K = 2 * (M - d)
    alpha = float(alpha_of(log_alpha))
    log_pi, reward, not_done = (np.asarray(t, dtype=np.float64).reshape(B) for t in (log_pi, reward, not_done))
    total, scale = 0.0, 1.0 / (B * 2 * M * K)
    dq = np.zeros((2, B, M))
    for b in range(B):
        pooled = sorted([float(z[n, b, i]) for n in range(2) for i in range(M)])[:K]
        ys = [float(reward[b]) + float(not_done[b]) * discount * (v - alpha * float(log_pi[b])) for v in pooled]
        for n in range(2):
            for i in range(M):
                tau = (2 * i + 1) / (2 * M)
                for y in ys:
                    u = y - float(theta[n, b, i])
                    w = abs(tau - (1.0 if u < 0 else 0.0))
                    total += w * (0.5 * u * u if abs(u) <= 1 else abs(u) - 0.5)
                    dq[n, b, i] -= scale * w * max(-1.0, min(1.0, u))
    return total * scale, dq


def actor_loss(theta, log_pi, log_std, log_alpha, target_entropy):
    """theta [2, B, M], log_pi [B] (or [B, 1]), log_std [B, A].  Returns dict(scalars [actor_loss, alpha_loss, entropy,
    alpha], dq [2, B, M], dlog_alpha); ``theta`` / ``log_pi`` in a graph: ``actor_loss`` / ``alpha_loss`` stay
    differentiable (alpha_loss in a float64 ``log_alpha`` that requires grad) and dq is None."""
    f64 = lambda t: torch.as_tensor(t).to(torch.float64)  # noqa: E731
    in_graph = torch.is_tensor(theta) and theta.requires_grad
    th = f64(theta) if in_graph else f64(theta).detach().clone().requires_grad_(True)
    _, B, M = th.shape
    lp = f64(log_pi).reshape(B)
    alpha = alpha_of(log_alpha)
    a_loss = (alpha * lp - th.mean(dim=(0, 2))).mean()
    A = log_std.shape[1]
    entropy = (0.5 * A * (1.0 + np.log(2 * np.pi)) + f64(log_std).detach().sum(-1)).mean()
    c = (-lp.detach() - float(target_entropy)).mean()
    if in_graph:
        la = log_alpha if torch.is_tensor(log_alpha) and log_alpha.requires_grad else f64(log_alpha)
        return dict(actor_loss=a_loss, alpha_loss=la.exp() * c, entropy=entropy, alpha=alpha, dq=None)
    a_loss.backward()
    return dict(scalars=torch.stack([a_loss.detach(), alpha * c, entropy, alpha]), dq=th.grad.detach(),
                dlog_alpha=alpha * c, actor_loss=a_loss.detach(), alpha_loss=alpha * c, entropy=entropy, alpha=alpha)
