"""What the categorical HL-Gauss critic costs at BASELINE.json configs[1] (B = 512, 84x84x9 -> random_crop 76x76,
hidden 1024).

python tools/hlg_bench.py [--bins 0,51,101] [--capacity 100000] [--reps 3] [--updates 200] [--out FILE]

``CurlSacAgent(critic_bins=M, critic_value_range=(-10, 10))`` for every M of ``--bins`` on the same build, alternating:
time per whole ``update()`` (host clock around back-to-back calls that end in a synchronise) and, for M > 0, the time of
each of the two new entry points (HIP events around back-to-back launches on the agent's own workspace).  M = 0 builds
the agent without the keyword, so ``--bins 0`` also runs on a checkout from before it: alternate the two checkouts to
see that nothing else moved.  The spread the figures have to be read against is each row's (min, max) over ``--reps``.
Prints one JSON line; ``--out`` also writes a text table."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

C, H, W, CROP, B, HIDDEN = 9, 84, 84, (76, 76), 512, 1024
RANGE = (-10.0, 10.0)


class _Log:
    def log(self, *a, **k):
        pass

    log_histogram = log_param = log_image = log


def build(capacity, bins):
    import curla_amd
    from curla_amd import augmentations as A
    dev = torch.device("cuda")
    curla_amd.set_seed_everywhere(1)
    aug = A.RandomCrop((H, W), CROP)
    kw = dict(critic_bins=bins, critic_value_range=RANGE) if bins else {}
    agent = curla_amd.CurlSacAgent(
        (C,) + CROP, (2,), dev, aug, hidden_dim=HIDDEN, discount=0.99, init_temperature=0.1, alpha_lr=1e-4,
        alpha_beta=0.5, actor_lr=1e-3, actor_beta=0.9, critic_lr=1e-3, critic_beta=0.9, critic_tau=0.01,
        encoder_feature_dim=50, encoder_lr=1e-3, encoder_tau=0.05, num_layers=4, num_filters=32, log_interval=10 ** 9, **kw)
    rb = curla_amd.ReplayBuffer((C, H, W), (2,), capacity, B, dev, aug)
    g = torch.Generator(device=dev).manual_seed(0)
    for ring in (rb._obs_store, rb._next_store):  # bench.py's device prefill
        for s in range(0, ring.numel(), 1 << 28):
            e = min(ring.numel(), s + (1 << 28))
            ring[s:e] = torch.randint(0, 256, (e - s,), dtype=torch.uint8, device=dev, generator=g)
    rb.actions.uniform_(-1, 1, generator=g)
    rb.rewards.normal_(generator=g)
    rb.not_dones.fill_(1.0)
    rb.not_dones[49::50] = 0.0
    rb.idx, rb.full = 0, True
    return agent, rb


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


def event_us(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(10):
        fn()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def one(capacity, bins, updates):
    agent, rb = build(capacity, bins)
    L, step = _Log(), [1]

    def update():
        agent.update(rb, L, step[0])
        step[0] += 1
    timed(update, 20)  # warm-up: code objects, workspaces
    out = dict(update_us=timed(update, updates))
    if bins:
        from curla_amd import ops
        ws = agent._ws(B)
        rew, nd = rb.rewards[:B].contiguous(), rb.not_dones[:B].contiguous()
        v_min, v_max, sigma = agent._hlg_params()
        n, la, A = B * bins, agent.log_alpha, agent.action_dim
        out["critic_loss_us"] = event_us(lambda: ops.hlg_critic_loss(
            ws.q, n, ws.tq, n, ws.log_pi, rew, nd, la, 0.99, B, bins, v_min, v_max, sigma, ws.dq, n, ws.target_q,
            ws.q_row_loss, ws.scalars[0:1]), 200)
        out["actor_loss_us"] = event_us(lambda: ops.hlg_actor_loss(
            ws.q, n, ws.log_pi, ws.log_std, A, la, float(agent.target_entropy), B, bins, v_min, v_max, ws.q_row_loss,
            ws.scalars[1:5], ws.dq, n, None), 200)
        out["target_clip_fraction"] = agent.target_clip_fraction()
    del agent, rb
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", default="0,51,101")
    ap.add_argument("--capacity", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--updates", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("hlg_bench.py measures on the GPU: no HIP device")
    bins = [int(m) for m in args.bins.split(",")]
    runs = {m: [] for m in bins}
    for _ in range(args.reps):
        for m in bins:
            runs[m].append(one(args.capacity, m, args.updates))
    res = dict(config="BASELINE.json configs[1]: B=512, 84x84x9 -> 76x76, hidden 1024", capacity=args.capacity,
               reps=args.reps, updates=args.updates)
    lines = []
    for m in bins:
        for key in sorted(runs[m][0]):
            vals = [r[key] for r in runs[m]]
            res["critic_bins=%d/%s" % (m, key)] = dict(median=statistics.median(vals), min=min(vals), max=max(vals))
            lines.append("critic_bins=%-3d  %-20s median %9.1f  (min %9.1f, max %9.1f)" %
                         (m, key, statistics.median(vals), min(vals), max(vals)))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write("tools/hlg_bench.py --bins %s --capacity %d --reps %d --updates %d\n%s\n" %
                    (args.bins, args.capacity, args.reps, args.updates, res["config"]))
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
