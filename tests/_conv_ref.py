"""Float64 CPU statements of the stride-1 3x3 convolutions (encoder.py's Conv2d(k=3) + ReLU and their autograd), of the
first layer (crop -> / 255 -> Conv2d(k=3, stride=2) -> ReLU, its weight / bias gradient and its observation gradient)
and the guard bands the conv kernel tests put round every device tensor (tests/test_gpu_conv_s1_edges.py,
tests/test_gpu_conv1_edges.py).  Tensors here are NHWC, as the kernels take them; weights OIHW."""
import torch
import torch.nn.functional as F

from tests.test_gpu_critic_ln import NAN, _same_bits  # noqa: F401  (re-exported: one bit comparison for the kernel tests)

# Floats of NaN in front of and behind a guarded tensor.  At least 64 (a wave's 16-byte store one row, or a 16-wide lane
# group's pixel pair, past the end lands inside); a multiple of 4, because the entry points require 16-byte alignment;
# no multiple of 32, so that a guarded NHWC tensor does not start on a pixel boundary of its buffer.
GUARD = 68


def _nchw64(x):
    return x.detach().cpu().double().permute(0, 3, 1, 2)


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def fwd_ref(x, w, b):
    """relu(conv2d(x, w, b)): x [B, H, W, C] -> [B, H-2, W-2, F], float64"""
    return _nhwc(torch.relu(F.conv2d(_nchw64(x), w.detach().cpu().double(), b.detach().cpu().double())))


def dgrad_ref(g, w, act_below):
    """conv_transpose2d(g, w) * (act_below > 0): g [B, H, W, F] -> [B, H+2, W+2, C], float64 (-0.0 and +0.0 both mask)"""
    gin = F.conv_transpose2d(_nchw64(g), w.detach().cpu().double())
    return _nhwc(gin) * (act_below.detach().cpu().double() > 0)


def wgrad_ref(x, g, nf=None):
    """dW [F, C, 3, 3] and db [F] of conv2d(x, W, b) under the output gradient g, by autograd in double"""
    C, Fo = x.shape[-1], g.shape[-1]
    w = torch.zeros(Fo, C, 3, 3, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(Fo, dtype=torch.float64, requires_grad=True)
    F.conv2d(_nchw64(x), w, b).backward(_nchw64(g))
    return w.grad, b.grad


def crop_ref(ring, idx, h1, w1, Hc, Wc):
    """the sampled crops of a uint8 ring [N, Hs, Ws, C]: [B, Hc, Wc, C] uint8"""
    return torch.stack([ring[int(i), int(y):int(y) + Hc, int(x):int(x) + Wc] for i, y, x in zip(idx, h1, w1)])


def conv1_fwd_ref(x, w, b):
    """relu(conv2d(x / 255, w, b, stride=2)): crops x [B, Hc, Wc, C] (uint8 or float) -> [B, Ho, Wo, F], float64"""
    return _nhwc(torch.relu(F.conv2d(_nchw64(x) / 255.0, w.detach().cpu().double(), b.detach().cpu().double(), stride=2)))


def conv1_wgrad_ref(x, g):
    """dW [F, C, 3, 3] and db [F] of conv2d(x / 255, W, b, stride=2) under the output gradient g [B, Ho, Wo, F], by
    autograd in double"""
    C, Fo = x.shape[-1], g.shape[-1]
    w = torch.zeros(Fo, C, 3, 3, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(Fo, dtype=torch.float64, requires_grad=True)
    F.conv2d(_nchw64(x) / 255.0, w, b, stride=2).backward(_nchw64(g))
    return w.grad, b.grad


def conv1_dgrad_ref(g, w, H, W):
    """d / d obs of conv2d(obs / 255, w, stride=2) under the output gradient g [B, Ho, Wo, F]: float64 NCHW [B, C, H, W],
    as the kernel writes it (the last row / column of an even size, which no output touches, is zero)"""
    obs = torch.zeros(g.shape[0], w.shape[1], H, W, dtype=torch.float64, requires_grad=True)
    F.conv2d(obs / 255.0, w.detach().cpu().double(), stride=2).backward(_nchw64(g))
    return obs.grad


def guarded(shape=None, data=None, guard=GUARD, shift=0):
    """A device tensor of ``shape`` (or a copy of the CPU / device tensor ``data``) in the middle of a NaN-filled flat
    buffer, ``guard`` floats in front and at least ``guard`` behind; without data the tensor itself is NaN too.  ``shift``
    more floats of NaN in front put its start 4 * shift bytes past a 16-byte boundary.  Returns (the view, a function that
    asserts that both guards are still all NaN)."""
    assert guard >= 64 and guard % 4 == 0 and 0 <= shift < 4
    if data is not None:
        shape = tuple(data.shape)
    n = 1
    for s in shape:
        n *= s
    front = guard + shift
    back = guard + (-(n + shift)) % 4
    flat = torch.full((front + n + back,), NAN, device="cuda")
    view = flat[front:front + n].view(shape)
    if data is not None:
        view.copy_(data)
    assert view.data_ptr() % 16 == 4 * shift

    def intact(what=""):
        ok = bool(torch.isnan(flat[:front]).all()) and bool(torch.isnan(flat[front + n:]).all())
        assert ok, f"{what}: a store outside the tensor ({int((~torch.isnan(flat[:front])).sum())} floats in front, " \
                   f"{int((~torch.isnan(flat[front + n:])).sum())} behind)"

    return view, intact
