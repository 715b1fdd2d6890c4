"""What truncated quantile critics cost: the two loss kernels alone, and ``update()`` with the feature off and on.

python tools/tqc_bench.py [--quantiles 25] [--drop 2] [--steps 200] [--warmup 20] [--rounds 3] [--out FILE]

One process, one GPU, bench.py's configs[1] (its CONFIGS["c2"]: B = 512, 84x84x9 ring -> random_crop 76x76, hidden 1024,
the ring prefilled as bench.py's device prefill does).  Four agents are built -- plain, ``critic_quantiles=M,
critic_drop_quantiles=d``, ``critic_layer_norm=True`` and both -- and timed in alternating rounds (plain, quantiles,
LayerNorm, both; again ...), ``--steps`` updates per window between device synchronisations, so that every "on" figure
stands beside an "off" figure of the same run.  The kernels alone: ``curla_tqc_critic_loss`` (with its mean launch)
and ``curla_tqc_actor_loss`` at B = 512 between device events, beside the launches they replace or sit next to
(``curla_critic_td_loss``, ``curla_actor_loss``, the critics' LayerNorm pair).  Prints one JSON line; ``--out`` also
writes a readable table there (profiles/tqc_bench.txt is one)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class NullLogger:
    def log(self, *a, **k):
        pass

    log_histogram = log_param = log_image = log


def build(cfg, capacity, **kw):
    import bench
    import curla_amd
    from curla_amd import augmentations as A
    dev = torch.device("cuda")
    C, (H, W), B = cfg["obs"][0], cfg["obs"][1:], cfg["batch"]
    curla_amd.set_seed_everywhere(1)
    aug = A.RandomCrop((H, W), cfg["crop"])
    agent = curla_amd.CurlSacAgent(
        (C,) + tuple(aug.output_shape), (2,), dev, aug, hidden_dim=bench.HIDDEN, discount=0.99, init_temperature=0.1,
        alpha_lr=1e-4, alpha_beta=0.5, actor_lr=1e-3, actor_beta=0.9, critic_lr=1e-3, critic_beta=0.9, critic_tau=0.01,
        encoder_feature_dim=50, encoder_lr=1e-3, encoder_tau=0.05, num_layers=cfg["layers"], num_filters=32,
        pixel_sac=cfg["pixel_sac"], log_interval=10 ** 9, **kw)
    rb = curla_amd.ReplayBuffer((C, H, W), (2,), capacity, B, dev, aug)
    g = torch.Generator(device=dev).manual_seed(0)
    for ring in (rb._obs_store, rb._next_store):
        for s in range(0, ring.numel(), 1 << 28):
            e = min(ring.numel(), s + (1 << 28))
            ring[s:e] = torch.randint(0, 256, (e - s,), dtype=torch.uint8, device=dev, generator=g)
    rb.actions.uniform_(-1, 1, generator=g)
    rb.rewards.normal_(generator=g)
    rb.not_dones.fill_(1.0)
    rb.not_dones[49::50] = 0.0
    rb.idx, rb.full = 0, True
    return agent, rb


def time_kernel(fn, iters=200, warm=20):
    """Microseconds per call of ``fn`` (which only enqueues), between device events over ``iters`` back-to-back calls."""
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / iters


def kernels_alone(B, M, d, H):
    from curla_amd import ops
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
    q, tq, dq = r(2, B, M), r(2, B, M), torch.empty(2, B, M, device=dev)
    q1, tq1, dq1, tgt = r(2, B, 1), r(2, B, 1), torch.empty(2, B, 1, device=dev), torch.empty(B, 1, device=dev)
    lp, rew, nd, ls = r(B, 1), r(B, 1), torch.ones(B, 1, device=dev), r(B, 2)
    la = torch.tensor(-2.3, device=dev, dtype=torch.float64)
    dla = torch.zeros((), device=dev, dtype=torch.float64)
    row, sc = torch.empty(B, device=dev), torch.zeros(8, device=dev)
    out = {
        "tqc_critic_loss (+ mean)": time_kernel(lambda: ops.tqc_critic_loss(q, B * M, tq, B * M, lp, rew, nd, la, 0.99, B, M,
                                                                            d, dq, B * M, row, sc[0:1])),
        "tqc_critic_loss (no mean)": time_kernel(lambda: ops.tqc_critic_loss(q, B * M, tq, B * M, lp, rew, nd, la, 0.99, B,
                                                                             M, d, dq, B * M, row, None)),
        "tqc_actor_loss": time_kernel(lambda: ops.tqc_actor_loss(q, B * M, lp, ls, 2, la, -2.0, B, M, sc[1:5], dq, B * M,
                                                                 dla)),
        "critic_td_loss (M = 1)": time_kernel(lambda: ops.critic_td_loss(q1, tq1, B, lp, rew, nd, la, 0.99, B, tgt,
                                                                         sc[0:1], dq1)),
        "actor_loss (M = 1)": time_kernel(lambda: ops.actor_loss(q1, B, lp, ls, 2, la, -2.0, B, sc[1:5], dq1, dla)),
    }
    # the critics' LayerNorm pair of one hidden layer (twins, B x H), for scale
    h, gm, bt = r(2, B, H), torch.ones(2, H, device=dev), torch.zeros(2, H, device=dev)
    xhat, rstd = torch.empty(2, B, H, device=dev), torch.empty(2, B, device=dev)
    out["mlp_ln_relu_fwd (twins)"] = time_kernel(lambda: ops.mlp_ln_relu_fwd(h, B * H, gm, bt, H, B, H, 2, xhat=xhat,
                                                                             rstd=rstd))
    dh = r(2, B, H)
    out["mlp_ln_bwd (twins, data gradient)"] = time_kernel(lambda: ops.mlp_ln_bwd(dh, B * H, xhat, rstd, gm, H, B, H, 2))
    return out


def main():
    import bench
    ap = argparse.ArgumentParser()
    ap.add_argument("--quantiles", type=int, default=25)
    ap.add_argument("--drop", type=int, default=2)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--capacity", type=int, default=20_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/tqc_bench.py needs the GPU: nothing is measured without one")
    cfg = bench.CONFIGS["c2"]
    M, d = args.quantiles, args.drop
    tqc = dict(critic_quantiles=M, critic_drop_quantiles=d)
    variants = [("plain", {}), ("quantiles", tqc), ("layer_norm", dict(critic_layer_norm=True)),
                ("layer_norm + quantiles", dict(critic_layer_norm=True, **tqc))]
    built = [(name, *build(cfg, args.capacity, **kw)) for name, kw in variants]
    L = NullLogger()
    step = {name: 1 for name, _ in variants}

    def window(name, agent, rb, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            agent.update(rb, L, step[name])
            step[name] += 1
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t0)
    for name, agent, rb in built:
        window(name, agent, rb, args.warmup)
    rates = {name: [] for name, _ in variants}
    for _ in range(args.rounds):
        for name, agent, rb in built:
            rates[name].append(window(name, agent, rb, args.steps))
    med = {k: statistics.median(v) for k, v in rates.items()}
    kernels = kernels_alone(cfg["batch"], M, d, bench.HIDDEN)
    us = lambda on, off: 1e6 * (1.0 / med[on] - 1.0 / med[off])  # noqa: E731
    result = {"tool": "tqc_bench", "config": "c2", "quantiles": M, "drop": d, "steps": args.steps, "rounds": args.rounds,
              "updates_per_s": {k: [round(x, 1) for x in v] for k, v in rates.items()},
              "median_updates_per_s": {k: round(v, 1) for k, v in med.items()},
              "cost_us_per_update": {"quantiles vs plain": round(us("quantiles", "plain"), 1),
                                     "layer_norm + quantiles vs layer_norm": round(us("layer_norm + quantiles", "layer_norm"), 1)},
              "kernel_us": {k: round(v, 2) for k, v in kernels.items()}}
    if args.out:
        with open(args.out, "w") as f:
            f.write(f"tools/tqc_bench.py --quantiles {M} --drop {d} --steps {args.steps} --rounds {args.rounds}\n")
            f.write("bench.py configs[1] (B = 512, 84x84x9 -> 76x76, hidden 1024), one MI355X, alternating rounds\n\n")
            f.write("update()/s per round, median\n")
            for k, v in rates.items():
                f.write(f"  {k:<26}" + "  ".join(f"{x:8.1f}" for x in v) + f"   median {med[k]:8.1f}\n")
            f.write("\ncost per update (from the medians), microseconds\n")
            for k, v in result["cost_us_per_update"].items():
                f.write(f"  {k:<40}{v:8.1f}\n")
            f.write("\nlaunches alone at B = 512, microseconds per call (device events, 200 back-to-back calls)\n")
            for k, v in kernels.items():
                f.write(f"  {k:<40}{v:8.2f}\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
