"""High-precision references and edge-case inputs for the float augmentation kernels (``curla_amd/csrc/augment.hip``).

``color_jiggle_f64`` is the colour jitter that the docstring of ``oracle.curla_oracle.color_jiggle`` states, written
out again in NumPy float64 (it shares no code with the oracle: the two are compared in tests/test_augment_edges_host.py,
and their distance on a set of inputs -- the FLOOR, what float32 rounding alone costs -- is the unit in which
tests/test_gpu_augment_edges.py bounds the kernels).  ``noisy_cover_f32`` is the noisy cover in exactly the float32
operations the kernels perform, so the kernels are compared to it bit for bit.  ``edge_pixels`` / ``edge_params`` /
``jiggle_case`` build inputs that reach the branches uniformly random bytes practically never reach: grey, black, white,
primaries, ties for the maximum, saturation 0 and saturation that clamps, contrast that clamps, hue shifts of whole and
half turns."""
import itertools
import math

import numpy as np

TWO_PI = 2.0 * math.pi
ORDERS = [list(p) for p in itertools.permutations(range(4))]  # all 24 orders of (brightness, contrast, saturation, hue)
LEVELS = (0, 1, 2, 127, 128, 254, 255)
N_PIXELS = 512  # 343 level triples + seeded random ones up to this
CASE_HW = (23, 29)  # 667 pixels: every edge pixel in every image; two 256-pixel blocks, two whole waves and 27 lanes


# ------------------------------------------------------------------------------------------------ colour jitter
def _rgb_to_hsv(r, g, b):
    """h in [0, 2 pi), s = (max - min) / max (0 for black), v = max; among equal maxima the first of (r, g, b) decides.
    The float32 codes divide by max + 1e-8 to keep 0 / 0 away; that guard is their device, not part of the colour
    space: it moves s by at most 1e-8 / max of itself, an output by at most 255 e-8 times the saturation factor, which
    is far inside float32 rounding and is counted with it in the floor.  Without it the HSV round trip is the identity
    to float64 rounding, which the host test asserts."""
    mx = np.maximum(r, np.maximum(g, b))
    mn = np.minimum(r, np.minimum(g, b))
    d = mx - mn
    s = d / np.where(mx > 0.0, mx, 1.0)
    d = np.where(d == 0.0, 1.0, d)
    rc, gc, bc = mx - r, mx - g, mx - b
    h = np.where(r == mx, bc - gc, np.where(g == mx, (rc - bc) + 2.0 * d, (gc - rc) + 4.0 * d)) / d
    h = np.mod(h / 6.0, 1.0)  # (NumPy's mod is Python's: the result has the divisor's sign)
    return TWO_PI * h, s, mx


def _hsv_to_rgb(h, s, v):
    h6 = h / TWO_PI * 6.0
    hi = np.mod(np.floor(h6), 6.0)
    f = np.mod(h6, 6.0) - hi
    p, q, t = v * (1.0 - s), v * (1.0 - f * s), v * (1.0 - (1.0 - f) * s)
    hi = hi.astype(np.int64)
    r = np.choose(hi, [v, q, p, p, t, v])
    g = np.choose(hi, [t, v, v, q, p, p])
    b = np.choose(hi, [p, p, t, v, v, q])
    return r, g, b


def color_jiggle_f64(imgs_u8, params, order):
    """imgs_u8 uint8 [B, C, H, W] (C = 3 k: k RGB frames per sample, each its own image); params [B k, 4] =
    (apply, contrast, saturation, hue in radians), taken as given (float32 values enter exactly, float64 values are
    not rounded); order = a permutation of 0 brightness (factor 0: nothing), 1 contrast (x c, clamp to [0, 1]),
    2 saturation (HSV, s f clamped to [0, 1]), 3 hue (HSV, h + d mod 2 pi).  Returns float64 [B, C, H, W] in
    [0, 255]; images with apply == 0 come back as the bytes."""
    imgs_u8 = np.asarray(imgs_u8)
    assert imgs_u8.dtype == np.uint8 and imgs_u8.ndim == 4 and imgs_u8.shape[1] % 3 == 0
    B, C, H, W = imgs_u8.shape
    n = B * (C // 3)
    par = np.asarray(params, dtype=np.float64).reshape(n, 4, 1, 1)
    x = imgs_u8.astype(np.float64).reshape(n, 3, H, W) / 255.0
    r, g, b = x[:, 0], x[:, 1], x[:, 2]
    con, sat, hue = par[:, 1], par[:, 2], par[:, 3]
    assert sorted(int(o) for o in order) == [0, 1, 2, 3]
    for op in (int(o) for o in order):
        if op == 1:
            r, g, b = (np.clip(c * con, 0.0, 1.0) for c in (r, g, b))
        elif op == 2:
            h, s, v = _rgb_to_hsv(r, g, b)
            r, g, b = _hsv_to_rgb(h, np.clip(s * sat, 0.0, 1.0), v)
        elif op == 3:
            h, s, v = _rgb_to_hsv(r, g, b)
            r, g, b = _hsv_to_rgb(np.mod(h + hue, TWO_PI), s, v)
    out = np.where(par[:, 0:1] == 0.0, x, np.stack([r, g, b], 1))
    return (out * 255.0).reshape(B, C, H, W)


def color_jiggle_oracle_f32(imgs_u8, params, order):
    """``oracle.curla_oracle.color_jiggle`` (float32) as a float64 array, for the floor
    max |oracle_f32 - color_jiggle_f64|.  The oracle walks the images one by one with tiny tensors, which PyTorch's
    thread pool only slows down (3 s against 0.1 s per call at 8 threads): one thread for the duration of the call."""
    import torch
    from oracle import curla_oracle as O
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        out = O.color_jiggle(np.ascontiguousarray(imgs_u8), torch.from_numpy(np.asarray(params, dtype=np.float32)), order)
    finally:
        torch.set_num_threads(threads)
    return out.numpy().astype(np.float64)


_tables = {}  # edge_pixels() is asked for once per launch by the path tests: built once, handed out as copies


def edge_pixels():
    """uint8 [N_PIXELS, 3]: every triple over LEVELS (black, white, five more greys, the primaries and secondaries,
    every pattern of ties, max - min = 1 at both ends of the range), then seeded random triples."""
    if "pixels" not in _tables:
        grid = np.array(list(itertools.product(LEVELS, repeat=3)), dtype=np.uint8)
        rest = np.random.RandomState(343).randint(0, 256, (N_PIXELS - len(grid), 3)).astype(np.uint8)
        _tables["pixels"] = np.concatenate([grid, rest])
    return _tables["pixels"].copy()


def edge_params():
    """float32 [115, 4], rows (apply, contrast, saturation, hue): apply = 1 over contrast {0, .8, 1.2, 2} x saturation
    {0, .5, 1.5, 4} x hue {-2 pi, -pi, -1, 0, pi / 3, pi, 7}, then three apply = 0 rows whose other values must not
    matter."""
    rows = [(1.0, c, s, h) for c in (0.0, 0.8, 1.2, 2.0) for s in (0.0, 0.5, 1.5, 4.0)
            for h in (-TWO_PI, -math.pi, -1.0, 0.0, math.pi / 3.0, math.pi, 7.0)]
    rows += [(0.0, 2.0, 4.0, 7.0), (0.0, 0.0, 0.0, -math.pi), (0.0, 1.2, 1.5, 1.0)]
    return np.array(rows, dtype=np.float32)


def jiggle_case(C, H, W, B=None, shift=0):
    """(frames uint8 [B, H, W, C], params float32 [B k, 4]) with k = C // 3.  Image i = b k + fr (sample b, stack
    position fr) holds the edge pixels tiled over H x W, starting 61 i + shift pixels into the list, and gets row
    (i + shift) of the parameter table (both taken modulo their lengths).  B = None: as many samples as give every
    parameter row an image, and H W must hold every edge pixel -- then every image holds every pixel, every stack
    position sees about a k-th of the parameter rows, and every (pixel, parameter row) pair occurs.  A given B (the small
    geometries of the path tests) takes what fits; ``shift`` moves on through both tables from call to call."""
    pix, table = edge_pixels(), edge_params()
    k = C // 3
    assert C == 3 * k and k >= 1
    if B is None:
        B = -(-len(table) // k)
        assert H * W >= len(pix), "every image must hold every edge pixel"
    img = np.arange(B * k)
    which = (np.arange(H * W)[None, :] + 61 * img[:, None] + shift) % len(pix)  # [B k, H W]
    frames = pix[which].reshape(B, k, H, W, 3).transpose(0, 2, 3, 1, 4).reshape(B, H, W, C)
    params = table[(img + shift) % len(table)]
    return np.ascontiguousarray(frames), np.ascontiguousarray(params)


# ------------------------------------------------------------------------------------------------ noisy cover
def noisy_cover_f32(frames_nhwc_u8, rows, noise, colors, top, bottom):
    """frames uint8 [n, H, W, C]; rows = the B frame indices of the minibatch (None: the first B frames, B from the
    noise); noise float32 [B, H, W, C].  Rows y < top or y >= H - bottom of every sample are float32(colors[c % 3]),
    the others float32(byte); then ONE float32 addition of the noise and the clamp to [0, 255]."""
    noise = np.asarray(noise)
    assert noise.dtype == np.float32
    B, H, W, C = noise.shape
    src = frames_nhwc_u8[:B] if rows is None else frames_nhwc_u8[np.asarray(rows)]
    assert src.shape == noise.shape and src.dtype == np.uint8
    v = src.astype(np.float32)
    y = np.arange(H)
    cover = (y < top) | (y >= H - bottom)
    col = np.array([colors[c % 3] for c in range(C)], dtype=np.float32)
    v[:, cover] = col
    out = v + noise
    assert out.dtype == np.float32
    return np.minimum(np.maximum(out, np.float32(0.0)), np.float32(255.0))
