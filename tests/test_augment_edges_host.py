"""The references of tests/_augment_ref.py, checked on the host: the float64 colour jitter against the float32 oracle
(their distance is the floor that tests/test_gpu_augment_edges.py multiplies), the contents of the edge-case tables,
the float64 jitter's own invariants, and the float32 noisy cover against the reference-generated fixture and the
oracle.  No GPU."""
import math

import numpy as np
import torch

from oracle import curla_oracle as O
from tests import _augment_ref as R
from tests._util import load

FLOOR_CAP = 2e-3  # absolute, outputs in [0, 255]: a condition on the inputs and the restatement, not a kernel figure


def _nchw(frames_nhwc):
    return np.ascontiguousarray(frames_nhwc.transpose(0, 3, 1, 2))


def test_float32_oracle_agrees_with_the_float64_restatement_on_the_edge_set():
    """All 24 orders on jiggle_case(3, ...): 115 images, one per parameter row, every one holding every edge pixel.
    The floor max |oracle_f32 - f64| is printed per order; the oracle's own formulas in double gave 1.17e-3 on this
    parameter set, so the cap of 2e-3 leaves a restatement that differs in substance (a wrong sector on a tie, a lost
    clamp: errors of whole grey levels) nowhere to hide."""
    frames, params = R.jiggle_case(3, *R.CASE_HW)
    imgs = _nchw(frames)
    assert imgs.shape[0] == len(R.edge_params()) and imgs.shape[2] * imgs.shape[3] >= R.N_PIXELS
    worst = 0.0
    for order in R.ORDERS:
        floor = float(np.abs(R.color_jiggle_oracle_f32(imgs, params, order) - R.color_jiggle_f64(imgs, params, order)).max())
        print(f"order {order}: floor max |oracle_f32 - f64| = {floor:.3e}")
        worst = max(worst, floor)
    print(f"floor over all 24 orders = {worst:.3e} (cap {FLOOR_CAP:.0e})")
    assert 0.0 < worst <= FLOOR_CAP


def test_edge_pixels_hold_the_cases_hsv_code_gets_wrong():
    pix = R.edge_pixels()
    assert pix.shape == (R.N_PIXELS, 3) and pix.dtype == np.uint8
    have = {tuple(int(v) for v in p) for p in pix}
    assert len({p for p in have if set(p) <= set(R.LEVELS)}) == 343
    assert (0, 0, 0) in have and (255, 255, 255) in have
    assert len({p for p in have if p[0] == p[1] == p[2] and 0 < p[0] < 255}) >= 5
    assert {(255, 0, 0), (0, 255, 0), (0, 0, 255)} <= have
    # two-way ties for the maximum, in each pair of channels, the third one lower
    assert any(r == g > b for r, g, b in have) and any(r == b > g for r, g, b in have) and any(g == b > r for r, g, b in have)
    assert any(max(p) - min(p) == 1 for p in have)
    assert len(have) > 343 + 100  # ... and the random ones are not repeats of the grid


def test_edge_params_reach_both_clamps_on_the_edge_pixels():
    table = R.edge_params()
    assert table.dtype == np.float32 and table.shape[1] == 4
    on = table[table[:, 0] == 1]
    assert len(on) == 4 * 4 * 7
    assert {float(v) for v in on[:, 1]} == {0.0, float(np.float32(0.8)), float(np.float32(1.2)), 2.0}
    assert {float(v) for v in on[:, 2]} == {0.0, 0.5, 1.5, 4.0}
    want_hues = [-2 * math.pi, -math.pi, -1.0, 0.0, math.pi / 3, math.pi, 7.0]
    assert {float(v) for v in on[:, 3]} == {float(np.float32(v)) for v in want_hues}
    off = table[table[:, 0] == 0]
    assert len(off) >= 1 and bool((off[:, 1:] != np.array([1, 1, 0], np.float32)).any())
    x = R.edge_pixels().astype(np.float64) / 255.0
    mx, mn = x.max(1), x.min(1)
    s = (mx - mn) / np.where(mx > 0, mx, 1.0)
    for sat in (1.5, 4.0):  # some pixels clamp at s' = 1, others do not: both sides of the min() run
        assert bool((s * sat > 1).any()) and bool(((s * sat < 1) & (s > 0)).any())
    for con in (1.2, 2.0):  # some channels clamp at 1, others do not
        assert bool((x * con > 1).any()) and bool(((x * con < 1) & (x > 0)).any())


def test_float64_jitter_invariants():
    frames, params = R.jiggle_case(6, *R.CASE_HW)
    imgs = _nchw(frames)
    x = imgs.astype(np.float64)
    n = params.shape[0]
    for order in ([0, 1, 2, 3], [3, 2, 1, 0], [2, 0, 3, 1]):
        out = R.color_jiggle_f64(imgs, params, order)
        assert out.dtype == np.float64 and out.shape == imgs.shape
        assert out.min() >= 0.0 and out.max() <= 255.0
        per_img = out.reshape(n, 3, *R.CASE_HW)
        assert np.array_equal(per_img[params[:, 0] == 0], x.reshape(per_img.shape)[params[:, 0] == 0])
        assert int((params[:, 0] == 0).sum()) >= 1
        const = lambda con, sat, hue: np.tile(np.array([[1.0, con, sat, hue]]), (n, 1))  # noqa: E731
        assert np.abs(R.color_jiggle_f64(imgs, const(1.0, 1.0, 0.0), order) - x).max() <= 1e-9
        grey = R.color_jiggle_f64(imgs, const(1.0, 0.0, 0.0), order).reshape(n, 3, *R.CASE_HW)
        v = x.reshape(n, 3, *R.CASE_HW).max(1, keepdims=True)
        assert np.abs(grey - v).max() <= 1e-9
        turn = R.color_jiggle_f64(imgs, const(1.2, 1.5, 2.0 * math.pi), order)
        assert np.abs(turn - R.color_jiggle_f64(imgs, const(1.2, 1.5, 0.0), order)).max() <= 1e-9


def test_noisy_cover_f32_reproduces_the_reference_fixture():
    """The comparison tests/test_gpu_augment.py makes for the kernel (the fixture is stored as float16)."""
    g = load("noisy_cover.npz")
    rs = np.random.RandomState(int(g["imgs_seed"]))
    imgs = rs.randint(0, 256, (5, 9, 34, 40), dtype=np.uint8)
    noise = rs.randn(5, 9, 34, 40).astype(np.float32) * 10.0
    out = R.noisy_cover_f32(np.ascontiguousarray(imgs.transpose(0, 2, 3, 1)), None,
                            np.ascontiguousarray(noise.transpose(0, 2, 3, 1)), list(g["colors"]), int(g["top"]),
                            int(g["bottom"])).transpose(0, 3, 1, 2)
    assert out.dtype == np.float32
    assert abs(out.astype(np.float64).sum() - float(g["out_sum"])) <= 1e-6 * abs(float(g["out_sum"]))
    assert np.abs(out - g["out"].astype(np.float32)).max() <= 0.13


def test_noisy_cover_f32_equals_the_oracle_at_the_cover_edges():
    """The oracle takes ratios: (ratio, ratio) -> ceil(H ratio) rows, chosen to give the (top, bottom) named.  (It
    indexes rows, so it cannot state top > H; those geometries are checked kernel against restatement only.)"""
    cases = [(21, 0.0, 0.0, 0, 0), (21, 0.33, 0.2, 7, 5), (21, 1.0, 0.0, 21, 0), (21, 0.0, 1.0, 0, 21),
             (21, 0.7, 0.45, 15, 10), (21, 0.0, 0.01, 0, 1), (21, 0.01, 0.0, 1, 0), (1, 1.0, 0.0, 1, 0), (1, 0.0, 0.0, 0, 0)]
    colors = (17.5, -3.0, 300.25)
    for C in (4, 9):
        for H, tr, br, top, bottom in cases:
            assert (int(np.ceil(H * tr)), int(np.ceil(H * br))) == (top, bottom)
            rs = np.random.RandomState(100 * H + top + C)
            frames = rs.randint(0, 256, (6, H, 23, C), dtype=np.uint8)
            rows = np.array([4, 0, 4, 5, 2])
            noise = (rs.randn(5, H, 23, C) * 60.0).astype(np.float32)
            got = R.noisy_cover_f32(frames, rows, noise, colors, top, bottom)
            want = O.noisy_cover(torch.from_numpy(_nchw(frames[rows])).float(), colors, torch.from_numpy(_nchw(noise)), tr, br)
            assert np.array_equal(_nchw(got), want.numpy()), (C, H, top, bottom)
            assert got.min() == 0.0 and got.max() == 255.0
