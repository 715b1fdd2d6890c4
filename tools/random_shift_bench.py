#!/usr/bin/env python3
"""curla_random_shift_u8 against a plain device-to-device copy of the same bytes, and whole updates with RandomShift
against identity:
python tools/random_shift_bench.py [--no-updates]
Kernel: one shift launch for a 3B minibatch (obs | next_obs | pos from a double ring, period 2B, as ReplayBuffer issues
it) against ``copy_`` of a uint8 tensor of the same 3B * frame bytes, at 84 x 84 x 9 and 90 x 160 x 9, B = 512.  The two
forms alternate; each sample is 10 back-to-back repetitions between two HIP events (launch gaps hidden behind the
queue); medians of 15 samples are printed with min - max and the ratio shift / copy.
Updates (tools/host_overhead.py's loop): 60 updates back to back, three times, eager and replayed from update graphs,
``random_shift`` against ``identity`` at the same geometry."""
import os, statistics, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import curla_amd
from curla_amd import ops

REP, SAMPLES = 10, 15
GEOMETRIES = ((84, 84, 9, 512), (90, 160, 9, 512))
dev = torch.device("cuda")


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REP):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / REP * 1e3  # us


for (H, W, C, B) in GEOMETRIES:
    frame, cap, pad = H * W * C, 4096, 4
    store = torch.zeros(2 * cap * frame + 32, dtype=torch.uint8, device=dev)
    store.random_(0, 256)
    ring = store[:2 * cap * frame].view(2 * cap, H, W, C)
    idx = torch.randint(0, cap, (B,), device=dev)
    idx2 = torch.cat([idx, idx + cap])
    dy = torch.randint(0, 2 * pad + 1, (3 * B,), device=dev, dtype=torch.int32)
    dx = torch.randint(0, 2 * pad + 1, (3 * B,), device=dev, dtype=torch.int32)
    out = torch.zeros(3 * B * frame + 32, dtype=torch.uint8, device=dev)
    out_v = out[:3 * B * frame].view(3 * B, H, W, C)
    src = torch.zeros(3 * B * frame, dtype=torch.uint8, device=dev).random_(0, 256)
    dst = torch.empty_like(src)

    def shift():
        ops.random_shift_u8(ring, idx2, 2 * B, dy, dx, pad, 3 * B, out_v)

    def copy():
        dst.copy_(src)

    for _ in range(3):
        shift(), copy()
    torch.cuda.synchronize()
    ts, tc = [], []
    for _ in range(SAMPLES):
        ts.append(timed(shift)), tc.append(timed(copy))
    ms, mc = statistics.median(ts), statistics.median(tc)
    nbytes = 3 * B * frame
    print(f"{H}x{W}x{C} B={B} ({nbytes / 1e6:.1f} MB read + written): random_shift_u8 median {ms:.1f} us (min {min(ts):.1f}, "
          f"max {max(ts):.1f}; {2 * nbytes / ms / 1e6:.2f} TB/s) | copy_ median {mc:.1f} us (min {min(tc):.1f}, max {max(tc):.1f}; "
          f"{2 * nbytes / mc / 1e6:.2f} TB/s) | ratio shift / copy {ms / mc:.3f}", flush=True)
    del store, ring, out, out_v, src, dst

if "--no-updates" in sys.argv:
    sys.exit(0)


class L:
    def log(self, *a, **k):
        pass


for (H, W, C, B) in GEOMETRIES:
    for graphs in (False, True):
        for name in ("identity", "random_shift"):
            curla_amd.set_seed_everywhere(1)
            aug = curla_amd.make_augmentor(name, (H, W))
            agent = curla_amd.CurlSacAgent((C, H, W), (2,), dev, aug, hidden_dim=1024, log_interval=10 ** 9)
            rb = curla_amd.ReplayBuffer((C, H, W), (2,), 20000, B, dev, aug)
            rb._obs_store.random_(0, 256); rb._next_store.random_(0, 256)
            rb.actions.uniform_(-1, 1); rb.rewards.normal_(); rb.not_dones.fill_(1.0); rb.idx, rb.full = 0, True
            if graphs:
                agent.enable_update_graphs(rb)
            step = 1  # (never a logging step)
            for _ in range(20):
                agent.update(rb, L(), step); step += 1
            times = []
            for rep in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(60):
                    agent.update(rb, L(), step); step += 1
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) / 60 * 1e3)
            print(f"{H}x{W}x{C} B={B} {name:12s} graphs {graphs}: 60 updates back to back, median {statistics.median(times):.3f} "
                  f"ms/update (min {min(times):.3f}, max {max(times):.3f})", flush=True)
            del agent, rb
            torch.cuda.empty_cache()
