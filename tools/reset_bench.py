"""What one ``CurlSacAgent.reset_networks()`` costs at BASELINE configs[1] (B = 512, 84x84x9 -> random_crop 76x76,
hidden 1024), beside the time of one ``update()``.

python tools/reset_bench.py [--resets N] [--updates N] [--capacity N]

For ``encoder_keep`` in {1.0, 0.8} it prints one line:

    host ms : wall time of the call, from an idle device to its return (median of ``--resets`` calls) -- drawing and
              orthogonalising a fresh Actor and Critic on the CPU and laying them out in the pinned staging buffers
    device ms : the time between two device events around what the call enqueues -- two host-to-device copies, three
              shrink-and-perturb launches and the fills -- with the device idle in front (median of ``--resets`` calls).
              Events bracket the host's work between them as well, so this figure is taken in a second pass in which the
              staged values are sent again without a new draw: what remains is the device's work and the gaps the host
              leaves between 19 small enqueues

and, once, the wall time per eager ``update()`` (two device synchronisations around ``--updates`` calls).  One GPU."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C, HW, CROP, B, HIDDEN = 9, (84, 84), (76, 76), 512, 1024


class NullLogger:
    def log(self, *a, **k):
        pass

    log_histogram = log_param = log_image = log


def build(capacity):
    import curla_amd
    from curla_amd import augmentations as A
    dev = torch.device("cuda")
    curla_amd.set_seed_everywhere(1)
    aug = A.RandomCrop(HW, CROP)
    agent = curla_amd.CurlSacAgent(
        (C,) + CROP, (2,), dev, aug, hidden_dim=HIDDEN, discount=0.99, init_temperature=0.1, alpha_lr=1e-4,
        alpha_beta=0.5, actor_lr=1e-3, actor_beta=0.9, critic_lr=1e-3, critic_beta=0.9, critic_tau=0.01,
        encoder_feature_dim=50, encoder_lr=1e-3, encoder_tau=0.05, num_layers=4, num_filters=32, log_interval=10 ** 9)
    rb = curla_amd.ReplayBuffer((C,) + HW, (2,), capacity, B, dev, aug)
    g = torch.Generator(device=dev).manual_seed(0)
    for ring in (rb._obs_store, rb._next_store):
        ring[:] = torch.randint(0, 256, (ring.numel(),), dtype=torch.uint8, device=dev, generator=g)
    rb.actions.uniform_(-1, 1, generator=g)
    rb.rewards.normal_(generator=g)
    rb.not_dones.fill_(1.0)
    rb.not_dones[49::50] = 0.0
    rb.idx, rb.full = 0, True
    return agent, rb


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--resets", type=int, default=20)
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
    n = agent._critic_flat.numel() + agent._target_flat.numel() + agent._actor_flat.numel()
    print(f"# B = {B}, {HW[0]}x{HW[1]}x{C} -> {CROP[0]}x{CROP[1]}, hidden {HIDDEN}: {n} parameters in the three flat "
          f"buffers; {args.resets} resets per row")
    print(f"{'encoder_keep':>12s} {'host ms':>9s} {'device ms':>10s} {'update() ms':>12s}")
    agent.reset_networks()  # (first use: the staging buffers)
    torch.cuda.synchronize()
    for keep in (1.0, 0.8):
        host = []
        for _ in range(args.resets):
            step += 1
            agent.update(rb, L, step)  # (a reset of a trained state, not of a fresh one)
            torch.cuda.synchronize()
            h0 = time.perf_counter()
            agent.reset_networks(encoder_keep=keep)
            host.append(time.perf_counter() - h0)
        torch.cuda.synchronize()
        # the device's share: the same enqueued work with the draw taken out of the bracket (the staged values re-sent)
        real = agent._stage_fresh
        agent._stage_fresh = agent._reset_staging
        dev_ms = []
        for _ in range(args.resets):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            agent.reset_networks(encoder_keep=keep)
            e1.record()
            e1.synchronize()
            dev_ms.append(e0.elapsed_time(e1))
        del agent._stage_fresh
        assert agent._stage_fresh.__func__ is real.__func__
        print(f"{keep:12.1f} {1e3 * statistics.median(host):9.3f} {statistics.median(dev_ms):10.3f} {1e3 * t_update:12.3f}",
              flush=True)


if __name__ == "__main__":
    main()
