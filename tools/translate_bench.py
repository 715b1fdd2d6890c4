#!/usr/bin/env python3
"""curla_translate_u8 against curla_random_shift_u8 (the yardstick) at the training geometry, as bytes WRITTEN per second:
python tools/translate_bench.py [--launches K]
One launch for a 3B minibatch (obs | next_obs | pos from a double ring, period 2B, as ReplayBuffer issues it), B = 512,
so n = 1536: the translate 84 x 84 x 9 -> 92 x 92 (offsets in [0, 8]^2) and the shift 84 x 84 x 9 (pad 4).  The two
alternate; each sample is 10 back-to-back repetitions between two HIP events, medians of 15 samples are printed with
min - max.  ``--kinds`` adds a third form to the alternation, the translate onto a canvas of the frame's own size (a plain
gather: every group is an inside group, one load and one store), to tell what the margin and mixed groups cost; leave it
out under the profiler, whose statistics go by kernel name.  For kernel times proper run it under the profiler, in a
run of its own, and read translate_u8_kernel and random_shift_u8_kernel from kernel_stats.csv
(tools/summarize_rocprof.py):
rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/translate_bench.py"""
import os, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from curla_amd import ops

REP, SAMPLES = 10, 15
if "--launches" in sys.argv:
    SAMPLES = max(1, int(sys.argv[sys.argv.index("--launches") + 1]) // REP)
H, W, C, Ho, Wo, B, pad, cap = 84, 84, 9, 92, 92, 512, 4, 4096
dev = torch.device("cuda")
frame, oframe, n = H * W * C, Ho * Wo * C, 3 * B


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REP):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / REP * 1e3  # us


def stats(ts, nbytes):
    m = statistics.median(ts)
    return f"median {m:.1f} us (min {min(ts):.1f}, max {max(ts):.1f}), {nbytes / m / 1e6:.2f} TB/s written"


store = torch.zeros(2 * cap * frame + 32, dtype=torch.uint8, device=dev)
store.random_(0, 256)
ring = store[:2 * cap * frame].view(2 * cap, H, W, C)
idx = torch.randint(0, cap, (B,), device=dev)
idx2 = torch.cat([idx, idx + cap])
ty = torch.randint(0, Ho - H + 1, (n,), device=dev, dtype=torch.int32)
tx = torch.randint(0, Wo - W + 1, (n,), device=dev, dtype=torch.int32)
dy = torch.randint(0, 2 * pad + 1, (n,), device=dev, dtype=torch.int32)
dx = torch.randint(0, 2 * pad + 1, (n,), device=dev, dtype=torch.int32)
out_t = torch.zeros(n * oframe + 32, dtype=torch.uint8, device=dev)
out_s = torch.zeros(n * frame + 32, dtype=torch.uint8, device=dev)
out_tv, out_sv = out_t[:n * oframe].view(n, Ho, Wo, C), out_s[:n * frame].view(n, H, W, C)


def translate():
    ops.translate_u8(ring, idx2, 2 * B, ty, tx, n, out_tv)


def shift():
    ops.random_shift_u8(ring, idx2, 2 * B, dy, dx, pad, n, out_sv)


def gather():
    ops.translate_u8(ring, idx2, 2 * B, ty, tx, n, out_sv)


KINDS = "--kinds" in sys.argv
for _ in range(3):
    translate(), shift()
    if KINDS:
        gather()
torch.cuda.synchronize()
tt, ts, tg = [], [], []
for _ in range(SAMPLES):
    tt.append(timed(translate)), ts.append(timed(shift))
    if KINDS:
        tg.append(timed(gather))
rate_t, rate_s = n * oframe / statistics.median(tt), n * frame / statistics.median(ts)
print(f"n={n} translate_u8 {H}x{W}x{C} -> {Ho}x{Wo} ({n * oframe / 1e6:.1f} MB written, {n * frame / 1e6:.1f} MB read): "
      f"{stats(tt, n * oframe)} | random_shift_u8 {H}x{W}x{C} pad {pad} ({n * frame / 1e6:.1f} MB written and read): "
      f"{stats(ts, n * frame)} | bytes written per second, translate / shift: {rate_t / rate_s:.3f}", flush=True)
if KINDS:
    print(f"n={n} translate_u8 {H}x{W}x{C} -> {H}x{W} (inside groups only, {n * frame / 1e6:.1f} MB written and read): "
          f"{stats(tg, n * frame)}", flush=True)
