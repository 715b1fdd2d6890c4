"""The restatement of ``curla_affine_u8`` that tests/test_affine_host.py and tests/test_gpu_affine.py share, written
from the formula in include/curla_hip.h and independently of ``RandomAffine.warp``: one pixel in plain Python integers
(``affine_pixel``), the same vectorised over a frame in int64 with an explicit wrap32 (``affine_nhwc``), and the word
sets the kernel test runs."""
import math

import numpy as np

IDENTITY = (65536, 0, 0, 0, 65536, 0)
GARBAGE = (0x7FFFFFF5, -1, -2 ** 31, 12345678, -7, 2 ** 31 - 1)


def wrap32(v):
    """Two's-complement wrap-around of Python ints or int64 arrays into [-2^31, 2^31)."""
    v = v & 0xFFFFFFFF
    return v - ((v >> 31) << 32)


def affine_pixel(frame, words, fill, y, x):
    """The C output bytes of pixel (y, x) of one uint8 [H, W, C] frame, in Python integers."""
    H, W, C = frame.shape
    m00, m01, m02, m10, m11, m12 = (wrap32(int(w)) for w in words)
    X, Y = wrap32(m00 * x + m01 * y + m02), wrap32(m10 * x + m11 * y + m12)
    x0, y0, fx, fy = X >> 16, Y >> 16, (X >> 8) & 255, (Y >> 8) & 255

    def P(yy, xx, c):
        if fill == 0 and not (0 <= yy < H and 0 <= xx < W):
            return 0
        return int(frame[min(max(yy, 0), H - 1), min(max(xx, 0), W - 1), c])
    return [(P(y0, x0, c) * (256 - fx) * (256 - fy) + P(y0, x0 + 1, c) * fx * (256 - fy)
             + P(y0 + 1, x0, c) * (256 - fx) * fy + P(y0 + 1, x0 + 1, c) * fx * fy + 32768) >> 16 for c in range(C)]


def affine_nhwc(frames, words, fill):
    """uint8 [n, H, W, C] frames under per-sample words (n rows of six, any integers: the transpose of the [6][n] the
    kernel takes) and ``fill`` (1 edge, 0 zero): the four taps gathered per sample, int64 throughout."""
    frames = np.asarray(frames)
    n, H, W, C = frames.shape
    per_sample = [[int(v) for v in w] for w in words]
    assert len(per_sample) == n and all(len(w) == 6 for w in per_sample)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.int64)
    out = np.empty_like(frames)
    for s in range(n):
        m = [wrap32(int(v)) for v in per_sample[s]]
        X = wrap32(np.int64(m[0]) * xx + np.int64(m[1]) * yy + np.int64(m[2]))
        Y = wrap32(np.int64(m[3]) * xx + np.int64(m[4]) * yy + np.int64(m[5]))
        x0, y0 = np.floor_divide(X, 65536), np.floor_divide(Y, 65536)
        fx, fy = np.floor_divide(X, 256) % 256, np.floor_divide(Y, 256) % 256
        acc = np.full((H, W, C), 32768, dtype=np.int64)
        for dy in (0, 1):
            for dx in (0, 1):
                ty, tx = y0 + dy, x0 + dx
                tap = frames[s][np.minimum(np.maximum(ty, 0), H - 1), np.minimum(np.maximum(tx, 0), W - 1)].astype(np.int64)
                if fill == 0:
                    inside = (ty >= 0) & (ty <= H - 1) & (tx >= 0) & (tx <= W - 1)
                    tap = np.where(inside[..., None], tap, 0)
                weight = (fx if dx else 256 - fx) * (fy if dy else 256 - fy)
                acc += tap * weight[..., None]
        assert acc.min() >= 0 and acc.max() <= 255 * 65536 + 32768
        out[s] = acc // 65536
    return out


def words_of(H, W, theta_deg, s, ty, tx):
    """The six words of a rotation by theta (degrees, counter-clockwise) about the centre, a zoom by s and a shift by
    (ty, tx) pixels: the issue's formulas with Python floats."""
    th = math.radians(theta_deg)
    a, b = math.cos(th) / s, -math.sin(th) / s
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    ux, uy = cx + tx, cy + ty
    r = lambda v: int(np.rint(65536.0 * v))  # noqa: E731
    return (r(a), r(b), r(cx - a * ux - b * uy), r(-b), r(a), r(cy + b * ux - a * uy))


def kernel_word_sets(H, W):
    """(name, words) per sample of the kernel test."""
    return [
        ("identity", IDENTITY),
        ("180", words_of(H, W, 180.0, 1.0, 0.0, 0.0)),
        ("+90", words_of(H, W, 90.0, 1.0, 0.0, 0.0)),
        ("-90", words_of(H, W, -90.0, 1.0, 0.0, 0.0)),
        ("integer shift", (65536, 0, 1 << 16, 0, 65536, -(1 << 16))),           # inside the frame (H, W >= 2)
        ("shift out of the frame", (65536, 0, (W + 3) << 16, 0, 65536, -((H + 5) << 16))),  # all taps outside: pure fill
        ("half a pixel", (65536, 0, 0x8000, 0, 65536, 0x8000)),
        ("7.3 degrees, s 1.07, t (0.4, -0.6)", words_of(H, W, 7.3, 1.07, 0.4, -0.6)),
        ("33 degrees, s 0.5", words_of(H, W, 33.0, 0.5, 0.0, 0.0)),             # minification, source stride 2
        ("s 2", words_of(H, W, 0.0, 2.0, 0.0, 0.0)),                            # magnification
        ("garbage", GARBAGE),
        # beyond the issue's list: angles at which a band's source box is large (the band is narrowed, or gathered directly)
        ("20 degrees", words_of(H, W, 20.0, 1.0, 0.0, 0.0)),
        ("45 degrees", words_of(H, W, 45.0, 1.0, 0.0, 0.0)),
    ]
