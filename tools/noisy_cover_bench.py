#!/usr/bin/env python3
"""curla_noisy_cover_rng against the pair it replaces (torch.randn * std, then curla_noisy_cover), one minibatch tensor:
python tools/noisy_cover_bench.py            84 x 84 x 9, B = 512 (BASELINE.json configs[1]) and 168 x 168 x 12, B = 1024
The two forms alternate; each sample is 10 back-to-back repetitions between two HIP events (launch gaps hidden behind
the queue), medians of 15 samples are printed with the bytes each form moves."""
import os, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from curla_amd import ops

REP, SAMPLES = 10, 15


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REP):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / REP * 1e3  # us


for (H, W, C, B) in ((84, 84, 9, 512), (168, 168, 12, 1024)):
    n = B * H * W * C
    store = torch.zeros(4096 * H * W * C + 32, dtype=torch.uint8, device="cuda")
    store.random_(0, 256)
    ring = store[:4096 * H * W * C].view(4096, H, W, C)
    idx = torch.randint(0, 4096, (B,), device="cuda")
    out = torch.empty((B, H, W, C), device="cuda")
    top, bottom, std, colors = int(0.31 * H) + 1, int(0.2 * H) + 1, 10.0, [10.0, 100.0, 200.0]
    state = {"off": 0}

    def pair():
        noise = torch.randn((B, H, W, C), device="cuda") * std
        ops.noisy_cover(ring, idx, noise, colors, top, bottom, B, out)

    def fused():
        ops.noisy_cover_rng(ring, idx, std, (7, state["off"]), colors, top, bottom, B, out)
        state["off"] += (n + 3) // 4

    for _ in range(3):
        pair(), fused()
    torch.cuda.synchronize()
    tp, tf = [], []
    for _ in range(SAMPLES):
        tp.append(timed(pair)), tf.append(timed(fused))
    mp, mf = statistics.median(tp), statistics.median(tf)
    print(f"{H}x{W}x{C} B={B}: randn*std + noisy_cover median {mp:.1f} us (min {min(tp):.1f}, max {max(tp):.1f}; 17 B/element = "
          f"{17 * n / mp / 1e6:.2f} TB/s) | noisy_cover_rng median {mf:.1f} us (min {min(tf):.1f}, max {max(tf):.1f}; 5 B/element = "
          f"{5 * n / mf / 1e6:.2f} TB/s, {n / 4 / mf / 1e3:.1f} G counters/s) | ratio {mf / mp:.3f}", flush=True)
