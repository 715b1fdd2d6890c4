#!/usr/bin/env python3
"""curla_random_conv against curla_color_jiggle at the same geometry (both read the same bytes of the ring and write the
same float NHWC minibatch):
python tools/random_conv_bench.py [--jiggle-lib PATH]
One launch per minibatch tensor, gathered rows, at B = 1024, 168 x 168 x 12 (BASELINE configs[4]) and B = 512,
84 x 84 x 9.  The two kernels alternate; each sample is 10 back-to-back repetitions between two HIP events (launch gaps
hidden behind the queue); medians of 15 samples are printed with min - max, the algorithmic bytes per second
(B H W C * 5: one byte read, one float written) and the ratio conv / jitter.  ``--jiggle-lib``: take the jitter from
another build of the library (the parent commit's), called through ctypes with the same arguments."""
import ctypes, os, statistics, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import curla_amd
from curla_amd import _lib, ops

REP, SAMPLES = 10, 15
GEOMETRIES = ((168, 168, 12, 1024), (84, 84, 9, 512))
dev = torch.device("cuda")

other = None
if "--jiggle-lib" in sys.argv:
    other = ctypes.CDLL(os.path.abspath(sys.argv[sys.argv.index("--jiggle-lib") + 1]))
    other.curla_color_jiggle.argtypes = _lib.SIGNATURES["curla_color_jiggle"]
    other.curla_color_jiggle.restype = ctypes.c_int


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REP):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / REP * 1e3  # us


def stats(ts):
    return f"median {statistics.median(ts):.1f} us (min {min(ts):.1f}, max {max(ts):.1f})"


for (H, W, C, B) in GEOMETRIES:
    frame, cap = H * W * C, 4 * B
    store = torch.zeros(cap * frame + 32, dtype=torch.uint8, device=dev)
    store.random_(0, 256)
    ring = store[:cap * frame].view(cap, H, W, C)
    idx = torch.randint(0, cap, (B,), device=dev)
    torch.manual_seed(1)
    weights = curla_amd.RandomConv((H, W)).draw_weights(B).to(dev)
    params, order = curla_amd.ColorJiggle((H, W)).draw_params(B * (C // 3))
    params, order = params.to(dev), order.to(dev)
    out = torch.empty((B, H, W, C), dtype=torch.float32, device=dev)

    def conv():
        ops.random_conv(ring, idx, weights, B, out)

    if other is None:
        def jiggle():
            ops.color_jiggle(ring, idx, params, order, B, out)
    else:
        stream = torch.cuda.current_stream().cuda_stream
        args = (ring.data_ptr(), idx.data_ptr(), params.data_ptr(), order.data_ptr(), B, C, H, W, out.data_ptr(), stream)

        def jiggle():
            assert other.curla_color_jiggle(*args) == 0

    for _ in range(3):
        conv(), jiggle()
    torch.cuda.synchronize()
    tc, tj = [], []
    for _ in range(SAMPLES):
        tc.append(timed(conv)), tj.append(timed(jiggle))
    mc, mj = statistics.median(tc), statistics.median(tj)
    nbytes = 5 * B * frame
    print(f"{H}x{W}x{C} B={B} ({nbytes / 1e6:.0f} MB read + written): random_conv {stats(tc)} {nbytes / mc / 1e6:.2f} TB/s | "
          f"color_jiggle{' (--jiggle-lib)' if other else ''} {stats(tj)} {nbytes / mj / 1e6:.2f} TB/s | "
          f"ratio conv / jitter {mc / mj:.3f}", flush=True)
    del store, ring, out
