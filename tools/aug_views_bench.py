"""What two augmented views per transition cost at BASELINE.json configs[1] (B = 512, 84x84x9 -> random_crop 76x76,
hidden 1024).

python tools/aug_views_bench.py [--capacity 100000] [--reps 3] [--updates 200] [--out FILE]

``CurlSacAgent(aug_views=2)`` on a ``ReplayBuffer(aug_views=2)`` against both built without the keyword, on the same
build, alternating: time per whole ``update()`` (host clock around back-to-back calls that end in a synchronise) at the
same B -- B positions either way, so the views run holds B / 2 transitions --, and the time of each of the two new entry
points beside the one it stands in for (HIP events around back-to-back launches on the agent's own workspace).  Prints
one JSON line; ``--out`` also writes a text table."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

C, H, W, CROP, B, HIDDEN = 9, 84, 84, (76, 76), 512, 1024


class _Log:
    def log(self, *a, **k):
        pass

    log_histogram = log_param = log_image = log


def build(capacity, views):
    import curla_amd
    from curla_amd import augmentations as A
    dev = torch.device("cuda")
    curla_amd.set_seed_everywhere(1)
    aug = A.RandomCrop((H, W), CROP)
    kw = dict(aug_views=2) if views == 2 else {}
    agent = curla_amd.CurlSacAgent(
        (C,) + CROP, (2,), dev, aug, hidden_dim=HIDDEN, discount=0.99, init_temperature=0.1, alpha_lr=1e-4,
        alpha_beta=0.5, actor_lr=1e-3, actor_beta=0.9, critic_lr=1e-3, critic_beta=0.9, critic_tau=0.01,
        encoder_feature_dim=50, encoder_lr=1e-3, encoder_tau=0.05, num_layers=4, num_filters=32, log_interval=10 ** 9, **kw)
    rb = curla_amd.ReplayBuffer((C, H, W), (2,), capacity, B, dev, aug, **kw)
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


def one(capacity, views, updates):
    from curla_amd import ops
    agent, rb = build(capacity, views)
    L, step = _Log(), [1]

    def update():
        agent.update(rb, L, step[0])
        step[0] += 1
    timed(update, 20)  # warm-up: code objects, workspaces
    out = dict(update_us=timed(update, updates))
    ws = agent._ws(B)
    rew, nd = rb.rewards[:B].contiguous(), rb.not_dones[:B].contiguous()
    td = ops.critic_td_loss_views if views == 2 else ops.critic_td_loss
    ce = ops.curl_ce_views if views == 2 else ops.curl_ce
    out["td_loss_us"] = event_us(lambda: td(ws.q, ws.tq, B, ws.log_pi, rew, nd, agent.log_alpha, 0.99, B, ws.target_q,
                                            ws.scalars[0:1], ws.dq), 200)
    out["curl_ce_us"] = event_us(lambda: ce(ws.logits, B, B, ws.row_loss, None, ws.dlogits), 200)
    del agent, rb
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--capacity", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--updates", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("aug_views_bench.py measures on the GPU: no HIP device")
    runs = {1: [], 2: []}
    for _ in range(args.reps):
        for v in (1, 2):
            runs[v].append(one(args.capacity, v, args.updates))
    res = dict(config="BASELINE.json configs[1]: B=512, 84x84x9 -> 76x76, hidden 1024", capacity=args.capacity,
               reps=args.reps, updates=args.updates)
    lines = []
    for v in (1, 2):
        for key in sorted(runs[v][0]):
            vals = [r[key] for r in runs[v]]
            res["aug_views=%d/%s" % (v, key)] = dict(median=statistics.median(vals), min=min(vals), max=max(vals))
            lines.append("aug_views=%d  %-12s median %9.1f us  (min %9.1f, max %9.1f)" % (v, key, statistics.median(vals),
                                                                                        min(vals), max(vals)))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write("tools/aug_views_bench.py --capacity %d --reps %d --updates %d\n%s\n" %
                    (args.capacity, args.reps, args.updates, res["config"]))
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
