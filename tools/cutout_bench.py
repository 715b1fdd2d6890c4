#!/usr/bin/env python3
"""curla_cutout_u8 against a plain device-to-device copy of the same bytes and against curla_random_shift_u8 at the same
geometry, and whole updates with cutout_color against identity and random_shift:
python tools/cutout_bench.py [--no-updates]
Kernels: one launch for a 3B minibatch (obs | next_obs | pos from a double ring, period 2B, as ReplayBuffer issues it)
of the cutout (boxes drawn by RandomCutout's defaults, min_cut 10, max_cut 30, random colours), of the shift (pad 4) and
``copy_`` of a uint8 tensor of the same 3B * frame bytes, at 84 x 84 x 9 and 90 x 160 x 9, B = 512.  The three forms
alternate; each sample is 10 back-to-back repetitions between two HIP events (launch gaps hidden behind the queue);
medians of 15 samples are printed with min - max and the ratios cutout / copy and cutout / shift.
Updates (tools/host_overhead.py's loop): 60 updates back to back, three times, eager and replayed from update graphs,
``identity``, ``random_shift`` and ``cutout_color`` at the same geometry."""
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


def stats(ts):
    return f"median {statistics.median(ts):.1f} us (min {min(ts):.1f}, max {max(ts):.1f})"


for (H, W, C, B) in GEOMETRIES:
    frame, cap, pad = H * W * C, 4096, 4
    store = torch.zeros(2 * cap * frame + 32, dtype=torch.uint8, device=dev)
    store.random_(0, 256)
    ring = store[:2 * cap * frame].view(2 * cap, H, W, C)
    idx = torch.randint(0, cap, (B,), device=dev)
    idx2 = torch.cat([idx, idx + cap])
    dy = torch.randint(0, 2 * pad + 1, (3 * B,), device=dev, dtype=torch.int32)
    dx = torch.randint(0, 2 * pad + 1, (3 * B,), device=dev, dtype=torch.int32)
    np.random.seed(1)
    y0, x0, bh, bw, rgb = curla_amd.RandomCutout((H, W), color=True).draw_boxes(3 * B)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)  # noqa: E731
    box = [i32(y0), i32(x0), i32(bh | (bw << 16)), i32(rgb[:, 0] | (rgb[:, 1] << 8) | (rgb[:, 2] << 16))]
    out = torch.zeros(3 * B * frame + 32, dtype=torch.uint8, device=dev)
    out_v = out[:3 * B * frame].view(3 * B, H, W, C)
    src = torch.zeros(3 * B * frame, dtype=torch.uint8, device=dev).random_(0, 256)
    dst = torch.empty_like(src)

    def cutout():
        ops.cutout_u8(ring, idx2, 2 * B, *box, 3 * B, out_v)

    def shift():
        ops.random_shift_u8(ring, idx2, 2 * B, dy, dx, pad, 3 * B, out_v)

    def copy():
        dst.copy_(src)

    for _ in range(3):
        cutout(), shift(), copy()
    torch.cuda.synchronize()
    tk, ts, tc = [], [], []
    for _ in range(SAMPLES):
        tk.append(timed(cutout)), ts.append(timed(shift)), tc.append(timed(copy))
    mk, ms, mc = statistics.median(tk), statistics.median(ts), statistics.median(tc)
    nbytes = 3 * B * frame
    inside = float((bh * bw).sum()) / (3 * B * H * W)
    print(f"{H}x{W}x{C} B={B} ({nbytes / 1e6:.1f} MB written, {100 * inside:.1f} % of it inside a box): cutout_u8 {stats(tk)} "
          f"{2 * nbytes / mk / 1e6:.2f} TB/s | random_shift_u8 {stats(ts)} {2 * nbytes / ms / 1e6:.2f} TB/s | copy_ {stats(tc)} "
          f"{2 * nbytes / mc / 1e6:.2f} TB/s | ratio cutout / copy {mk / mc:.3f}, cutout / shift {mk / ms:.3f}", flush=True)
    del store, ring, out, out_v, src, dst

if "--no-updates" in sys.argv:
    sys.exit(0)


class L:
    def log(self, *a, **k):
        pass


for (H, W, C, B) in GEOMETRIES:
    for graphs in (False, True):
        for name in ("identity", "random_shift", "cutout_color"):
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
