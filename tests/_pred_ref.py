"""The self-predictive latent loss as a user would write it in torch -- ``F.normalize`` of both vectors,
the squared distance per row, the mean over rows, autograd for the gradient --, evaluated in float64 (the reference) or in
float32 (what the kernel's error is measured against); the kernel test's inputs; and ``curla_mean``'s summation order
restated in NumPy float32."""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-12  # F.normalize's default


def loss(p, t, dtype=torch.float64):
    """(row_loss [B], mean, dp [B, F]) of p against the constant t, evaluated in ``dtype``."""
    p = p.detach().to(dtype).clone().requires_grad_(True)
    t = t.detach().to(dtype)
    rows = ((F.normalize(p, dim=-1, eps=EPS) - F.normalize(t, dim=-1, eps=EPS)) ** 2).sum(-1)
    total = rows.mean()
    total.backward()
    return rows.detach(), total.detach(), p.grad.detach()


def loss_of(p, t):
    """The differentiable loss alone, in the tensors' own dtype (t is detached: the target gets no gradient)."""
    return ((F.normalize(p, dim=-1, eps=EPS) - F.normalize(t.detach(), dim=-1, eps=EPS)) ** 2).sum(-1).mean()


def dp_scale(p, B):
    """The size of a row's gradient at unit distance, (2 / B) / max(|p|, eps): what a row's dp error is measured against
    beside the row's own largest |dp| -- rows whose exact gradient is zero (p = t, p = -t, every row at F = 1) have no
    scale of their own."""
    return (2.0 / B) / p.double().norm(dim=-1).clamp_min(EPS)


HAND_ROWS = ("p_is_t", "p_is_minus_t", "orthogonal", "p_zero", "t_zero", "scaled_down", "scaled_up")


def inputs(B, Fd, seed=0):
    """float32 (p, t, {name: row}): fixed-seed normal rows whose magnitudes spread up to about 1e3, and, as far as B
    reaches, the hand-made rows from the last row backwards (row B - 1 - i holds HAND_ROWS[i]; row 0 stays a random one)."""
    g = torch.Generator().manual_seed(1000 * B + Fd + seed)
    mag = 10.0 ** (3.0 * torch.rand(B, 1, generator=g) - 1.0)  # 0.1 .. 100 per row, entries to about 1e3 at 3 sigma
    p = torch.randn(B, Fd, generator=g) * mag / 3.0
    t = torch.randn(B, Fd, generator=g) * mag.flip(0) / 3.0
    where = {}
    for i, name in enumerate(HAND_ROWS):
        b = B - 1 - i
        if b < 1:
            break
        where[name] = b
        if name == "p_is_t":
            p[b] = t[b]
        elif name == "p_is_minus_t":
            p[b] = -t[b]
        elif name == "orthogonal" and Fd >= 2:  # (p on the even features, t on the odd ones)
            p[b, 1::2] = 0
            t[b, 0::2] = 0
        elif name == "p_zero":
            p[b] = 0
        elif name == "t_zero":
            t[b] = 0
        elif name == "scaled_down":
            p[b] *= 1e-6
        elif name == "scaled_up":
            p[b] *= 1e6
    return p.contiguous(), t.contiguous(), where


def errors(rows, dp, ref_rows, ref_dp, p):
    """(row_loss error, dp error) of a float32 evaluation against the float64 reference: the row loss in absolute terms
    (it lies in [0, 4]), dp per row relative to max(the row's largest |dp|, dp_scale); the largest over the rows."""
    B = p.shape[0]
    e_rows = float((rows.double() - ref_rows).abs().max())
    scale = torch.maximum(ref_dp.abs().amax(dim=-1), dp_scale(p, B))
    e_dp = float(((dp.double() - ref_dp).abs().amax(dim=-1) / scale).max())
    return e_rows, e_dp


def fixed_order_mean(x):
    """``curla_mean`` over n float32 values, restated: 256 threads, thread i adds x[i], x[i + 256], ... in that order;
    each of the four waves adds its 64 lanes by the xor butterfly (32, 16, ..., 1); then (w0 + w1) + (w2 + w3), divided
    by n.  Every operation in float32."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    n = x.size
    acc = np.zeros(256, dtype=np.float32)
    for i in range(0, n, 256):
        chunk = x[i:i + 256]
        acc[:chunk.size] = acc[:chunk.size] + chunk
    lanes = np.arange(256)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[lanes ^ o]
    s = np.float32(np.float32(acc[0] + acc[64]) + np.float32(acc[128] + acc[192]))
    return np.float32(s / np.float32(n))
