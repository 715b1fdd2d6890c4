"""What ``CurlSacAgent(utd_ratio=G)`` costs and saves at BASELINE configs[1] (B = 512, 84x84x9 -> random_crop 76x76,
hidden 1024), with the DroQ / RLPD critic it is for: ``critic_layer_norm=True, critic_dropout=0.01,
critic_target_update_freq=1``.

python tools/utd_bench.py [--calls N] [--capacity N] [--ratios 1,2,4,20] [--depth D]

For G in ``--ratios``, eager and with update graphs, and for a hand-written loop of the same work --
G-1 x (``sample_cpc_refs()``, ``update_critic()``, ``soft_update_targets()``) in front of ``update()`` on a
``utd_ratio=1`` agent -- it prints one line each:

    update() calls/s | critic steps/s | ms per call | ms per leading sub-step = (t(G) - t(1)) / (G - 1) |
    host ms per call: the time one call takes to RETURN when it starts on an idle device (synchronised in front of it,
    not behind; mean of 10) -- the host's own work, plus what it waits for: a graphed call waits for the replay that
    last read a pinned block before rewriting it, so with ``--depth`` (``enable_update_graphs(depth=...)``, default 2)
    smaller than G it returns only ``depth`` sub-steps ahead of the device

and then the same three rows at the largest G on a ``ColorJiggle`` ``staged_aug=True`` buffer of the same geometry (no
crop: 84x84), where ``want_pos=False`` leaves the positive's jitter launch out of every leading sub-step and the
hand-written loop cannot.  Timing: wall clock between two device synchronisations around ``--calls`` calls, after a
warm-up that has captured every graph.  One GPU."""
import argparse
import os
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


def build(G, aug_name, capacity):
    import curla_amd
    from curla_amd import augmentations as A
    dev = torch.device("cuda")
    curla_amd.set_seed_everywhere(1)
    aug = A.RandomCrop(HW, CROP) if aug_name == "random_crop" else A.ColorJiggle(HW)
    agent = curla_amd.CurlSacAgent(
        (C,) + tuple(aug.output_shape), (2,), dev, aug, hidden_dim=HIDDEN, discount=0.99, init_temperature=0.1,
        alpha_lr=1e-4, alpha_beta=0.5, actor_lr=1e-3, actor_beta=0.9, critic_lr=1e-3, critic_beta=0.9, critic_tau=0.01,
        encoder_feature_dim=50, encoder_lr=1e-3, encoder_tau=0.05, num_layers=4, num_filters=32, log_interval=10 ** 9,
        critic_target_update_freq=1, critic_layer_norm=True, critic_dropout=0.01, utd_ratio=G)
    rb = curla_amd.ReplayBuffer((C,) + HW, (2,), capacity, B, dev, aug, staged_aug=aug_name != "random_crop")
    g = torch.Generator(device=dev).manual_seed(0)
    for ring in (rb._obs_store, rb._next_store):
        ring[:] = torch.randint(0, 256, (ring.numel(),), dtype=torch.uint8, device=dev, generator=g)
    rb.actions.uniform_(-1, 1, generator=g)
    rb.rewards.normal_(generator=g)
    rb.not_dones.fill_(1.0)
    rb.not_dones[49::50] = 0.0
    rb.idx, rb.full = 0, True
    return agent, rb


def hand_loop(agent, rb, G):
    """What a user of the ``utd_ratio=1`` agent writes: the critic's step on a fresh minibatch and the targets' lerp,
    G-1 times, then the update."""
    L = NullLogger()

    def call(step):
        for _ in range(G - 1):
            obs, action, reward, next_obs, not_done, _ = rb.sample_cpc_refs()
            agent.update_critic(obs, action, reward, next_obs, not_done, L, step)
            agent.soft_update_targets()
        agent.update(rb, L, step)
    return call


def measure(mode, G, aug_name, calls, capacity, depth):
    agent, rb = build(1 if mode == "hand loop" else G, aug_name, capacity)
    L = NullLogger()
    call = hand_loop(agent, rb, G) if mode == "hand loop" else (lambda step: agent.update(rb, L, step))
    step = 1
    call(step)  # (first use: workspaces, Adam states)
    if mode == "graphed":
        agent.enable_update_graphs(rb, depth=depth)
    for _ in range(2 * (1 + depth) + 2):  # warm-up; graphed: one eager use and ``depth`` captures of the even and the odd kind
        step += 1
        call(step)
    if mode == "graphed":
        assert agent._graphs and all(len(r) == depth and all(g["graph"] is not None for g in r)
                                     for r in agent._graphs.values())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        step += 1
        call(step)
    torch.cuda.synchronize()
    t = (time.perf_counter() - t0) / calls
    host = 0.0
    for _ in range(10):
        step += 1
        torch.cuda.synchronize()
        h0 = time.perf_counter()
        call(step)
        host += time.perf_counter() - h0
    torch.cuda.synchronize()
    host /= 10
    del agent, rb
    torch.cuda.empty_cache()
    return t, host


def table(aug_name, ratios, calls, capacity, depth):
    print(f"# {aug_name}, B = {B}, {HW[0]}x{HW[1]}x{C}, hidden {HIDDEN}, critic_layer_norm, critic_dropout = 0.01, "
          f"critic_target_update_freq = 1; {calls} timed calls per row, graph depth {depth}")
    print(f"{'mode':10s} {'G':>3s} {'calls/s':>9s} {'critic steps/s':>15s} {'ms/call':>9s} {'ms/leading':>11s} {'host ms/call':>13s}")
    for mode in ("eager", "graphed", "hand loop"):
        t1 = None
        for G in ratios:
            n = calls if G <= 4 else max(10, 4 * calls // G)  # (about as many critic steps per row)
            t, host = measure(mode, G, aug_name, n, capacity, depth)
            if G == 1:
                t1 = t
            lead = "" if G == 1 or t1 is None else "%.3f" % (1e3 * (t - t1) / (G - 1))
            print(f"{mode:10s} {G:3d} {1 / t:9.1f} {G / t:15.1f} {1e3 * t:9.3f} {lead:>11s} {1e3 * host:13.3f}", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--capacity", type=int, default=20_000)
    ap.add_argument("--ratios", default="1,2,4,20")
    ap.add_argument("--depth", type=int, default=2, help="enable_update_graphs(depth=...) of the graphed rows")
    args = ap.parse_args()
    ratios = sorted({int(g) for g in args.ratios.split(",")})
    np.random.seed(0)
    table("random_crop", ratios, args.calls, args.capacity, args.depth)
    print()
    table("color_jiggle staged_aug", sorted({1, ratios[-1]}), args.calls, min(args.capacity, 8_000), args.depth)


if __name__ == "__main__":
    main()
