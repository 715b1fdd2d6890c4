#!/usr/bin/env python3
"""Host-side enqueue time of update() vs GPU time (is the Python host ahead of the GPU?).
python tools/host_overhead.py [--graphs] [--setup crop|dedup|color_jiggle|noisy_cover] [--no-profile]
  --graphs   CurlSacAgent.enable_update_graphs, updates replayed from hipGraphs
  --setup    crop (default): RandomCrop 84 -> 76, 9 channels, B = 512 (BASELINE.json configs[1]);
             dedup: the same on the de-duplicated frame store;
             color_jiggle / noisy_cover: the reference's default geometry (train.py: 90 x 160 x 9, B = 512) on a
             ReplayBuffer(..., staged_aug=True) -- without --graphs AND with --default-buffer: the default buffer
The last line reports the GPU time per update: 60 updates back to back, one synchronize at the end."""
import os, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import curla_amd
dev = torch.device("cuda")
curla_amd.set_seed_everywhere(1)
setup = sys.argv[sys.argv.index("--setup") + 1] if "--setup" in sys.argv else "crop"
B = 512
if setup in ("crop", "dedup"):
    in_hw = (84, 84)
    aug = curla_amd.RandomCrop(in_hw, (76, 76))
else:
    in_hw = (90, 160)
    aug = curla_amd.make_augmentor(setup, in_hw)
agent = curla_amd.CurlSacAgent((9,) + tuple(aug.output_shape), (2,), dev, aug, hidden_dim=1024, log_interval=10 ** 9)
kw = dict(staged_aug=True) if setup in ("color_jiggle", "noisy_cover") and "--default-buffer" not in sys.argv else {}
cap = 4000 if setup == "dedup" else 20000
rb = curla_amd.ReplayBuffer((9,) + in_hw, (2,), cap, B, dev, aug, dedup_frames=setup == "dedup", **kw)
if setup == "dedup":  # one long frame-stacked run: every step adds one new frame
    rs = np.random.RandomState(0)
    stack = [rs.randint(0, 256, (3,) + in_hw, dtype=np.uint8) for _ in range(3)]
    for t in range(cap):
        new = stack[1:] + [rs.randint(0, 256, (3,) + in_hw, dtype=np.uint8)]
        rb.add(np.concatenate(stack), rs.uniform(-1, 1, 2), 0.1, np.concatenate(new), False)
        stack = new
else:
    rb._obs_store.random_(0, 256); rb._next_store.random_(0, 256)
    rb.actions.uniform_(-1, 1); rb.rewards.normal_(); rb.not_dones.fill_(1.0); rb.idx, rb.full = 0, True
class L:
    def log(self, *a, **k): pass
if "--graphs" in sys.argv:
    agent.enable_update_graphs(rb)
step = 1  # (never a logging step: log_interval is 1e9 and step 0 is skipped)
for _ in range(20):
    agent.update(rb, L(), step); step += 1
torch.cuda.synchronize()
for n in (3, 3, 3, 3):  # (short bursts: with 2 graphs per kind the host may run 3 updates ahead without waiting)
    t0, c0 = time.perf_counter(), time.process_time()
    for _ in range(n):
        agent.update(rb, L(), step); step += 1
    t1, c1 = time.perf_counter(), time.process_time()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    print(f"{n} updates: host enqueue {(t1 - t0) / n * 1e3:.3f} ms/update wall, {(c1 - c0) / n * 1e3:.3f} ms/update CPU; "
          f"total {(t2 - t0) / n * 1e3:.3f} ms/update", flush=True)
if "--no-profile" not in sys.argv:
    import cProfile, pstats
    pr = cProfile.Profile(); pr.enable()
    for _ in range(20):
        agent.update(rb, L(), step); step += 1
    pr.disable(); torch.cuda.synchronize()
    pstats.Stats(pr).sort_stats("tottime").print_stats(12)
for rep in range(3):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(60):
        agent.update(rb, L(), step); step += 1
    torch.cuda.synchronize()
    print(f"setup {setup} graphs {'--graphs' in sys.argv}: 60 updates back to back, {(time.perf_counter() - t0) / 60 * 1e3:.3f} "
          "ms/update (GPU-bound when the host enqueue above is shorter)", flush=True)
