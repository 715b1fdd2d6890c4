"""Float64 CPU statements of the encoder fc layer (encoder.py: z = LayerNorm(fc(h)), optionally tanh) as its kernels
cut it up (tests/test_gpu_fc_edges.py): split-K partial products, the two backward products, the LayerNorm forward
that adds up the partials.  Plain double matmuls and F.layer_norm; nothing here is written to by a test."""
import torch
import torch.nn.functional as F


def d(t):
    return t.detach().cpu().double()


def split_ranges(K, nsplit):
    """the k range [k0, k1) of every split of fc_fwd_kernel: K / 32 slices cut by floor(nslices * s / nsplit)"""
    nsl = K // 32
    return [(32 * (nsl * s // nsplit), 32 * (nsl * (s + 1) // nsplit)) for s in range(nsplit)]


def fwd_ref(x, W, k0=0, k1=None):
    """x[:, k0:k1] @ W[:, k0:k1]^T: x [B, K], W [F, K] -> [B, F]"""
    return d(x)[:, k0:k1] @ d(W)[:, k0:k1].t()


def dx_ref(dz, W, mask=None):
    """(dz @ W) where mask > 0 (-0.0 and +0.0 both mask): dz [B, F], W [F, K] -> [B, K]"""
    out = d(dz) @ d(W)
    return out if mask is None else out * (d(mask) > 0)


def dw_ref(dz, x):
    """dz^T @ x: dz [B, F], x [B, K] -> [F, K]"""
    return d(dz).t() @ d(x)


def ln_fwd_ref(partial, bias, gamma, beta, eps=1e-5, tanh_out=False):
    """partial [nsplit, B, F] -> (fc = sum of the partials + bias, y = LayerNorm(fc) (tanh'ed if asked), xhat, rstd)"""
    fc = d(partial).sum(0) + d(bias)
    y = F.layer_norm(fc, fc.shape[-1:], d(gamma), d(beta), eps)
    rstd = 1.0 / torch.sqrt(fc.var(-1, unbiased=False) + eps)
    xhat = (fc - fc.mean(-1, keepdim=True)) * rstd[:, None]
    return fc, (torch.tanh(y) if tanh_out else y), xhat, rstd
