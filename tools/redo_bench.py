"""What one ``CurlSacAgent.redo_pass()`` costs at BASELINE configs[1] (B = 512, 84x84x9 -> random_crop 76x76, hidden
1024), beside the time of one ``update()``.

python tools/redo_bench.py [--passes N] [--updates N] [--capacity N]

For ``redo_recycle`` in {False, True} it prints one line:

    host ms   : wall time of the call, from an idle device to its return (median of ``--passes`` calls) -- with recycling
                that is the drawing of a fresh Actor and Critic on the CPU (reset_networks()'s)
    device ms : the time between two device events around what the call enqueues, with the device idle in front (median
                of ``--passes`` calls).  With recycling the events would bracket the host's draw as well, so this figure
                is taken with the staged values sent again without a new draw: the forward, the four column sums, the
                mask launch, two host-to-device copies and the two recycle launches

and, once, the wall time per eager ``update()``.  One GPU."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.reset_bench import B, C, CROP, HIDDEN, HW, NullLogger, build  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--updates", type=int, default=100)
    ap.add_argument("--capacity", type=int, default=20_000)
    args = ap.parse_args()
    np.random.seed(0)
    agent, rb = build(args.capacity)
    L = NullLogger()
    step = 0
    for _ in range(6):  # (first use: workspaces, Adam states)
        step += 1
        agent.update(rb, L, step)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.updates):
        step += 1
        agent.update(rb, L, step)
    torch.cuda.synchronize()
    t_update = (time.perf_counter() - t0) / args.updates
    print(f"# B = {B}, {HW[0]}x{HW[1]}x{C} -> {CROP[0]}x{CROP[1]}, hidden {HIDDEN}; {args.passes} passes per row")
    print(f"{'redo_recycle':>12s} {'host ms':>9s} {'device ms':>10s} {'update() ms':>12s}  dormant fractions")
    batch = lambda: rb.sample_cpc_refs()[:2]  # noqa: E731  (a handle is valid until the ring has drawn a few more)
    agent.redo_pass(*batch())  # (first use: the pass's buffers, the staging buffers)
    torch.cuda.synchronize()
    for recycle in (False, True):
        agent.redo_recycle = recycle
        host = []
        for _ in range(args.passes):
            step += 1
            agent.update(rb, L, step)  # (a pass over a trained state)
            obs, action = batch()
            torch.cuda.synchronize()
            h0 = time.perf_counter()
            agent.redo_pass(obs, action)
            host.append(time.perf_counter() - h0)
        torch.cuda.synchronize()
        dev_ms = []  # (draw=False: the draw taken out of the bracket, the staged values re-sent)
        for _ in range(args.passes):
            obs, action = batch()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            agent._redo_pass(obs, action, draw=False)
            e1.record()
            e1.synchronize()
            dev_ms.append(e0.elapsed_time(e1))
        fr = " ".join("%.3f" % x for x in agent.dormant_report().values())
        print(f"{str(recycle):>12s} {1e3 * statistics.median(host):9.3f} {statistics.median(dev_ms):10.3f} "
              f"{1e3 * t_update:12.3f}  {fr}", flush=True)


if __name__ == "__main__":
    main()
