"""What prioritized replay costs at BASELINE.json configs[1] (B = 512, 84x84x9 -> random_crop 76x76, hidden 1024).

python tools/per_bench.py [--capacity 100000] [--reps 3] [--updates 200] [--samples 300] [--out FILE]

``ReplayBuffer(prioritized=True)`` against ``prioritized=False`` on the same build, alternating: device time per
``sample_cpc_refs()`` and per whole ``update()`` (host clock around back-to-back calls that end in a synchronise), and
the time of each of the three new entry points on its own (HIP events around back-to-back launches on the buffer's own
storage).  Prints one JSON line; ``--out`` also writes a text table."""
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


def build(capacity, prioritized):
    import curla_amd
    from curla_amd import augmentations as A
    dev = torch.device("cuda")
    curla_amd.set_seed_everywhere(1)
    aug = A.RandomCrop((H, W), CROP)
    agent = curla_amd.CurlSacAgent(
        (C,) + CROP, (2,), dev, aug, hidden_dim=HIDDEN, discount=0.99, init_temperature=0.1, alpha_lr=1e-4,
        alpha_beta=0.5, actor_lr=1e-3, actor_beta=0.9, critic_lr=1e-3, critic_beta=0.9, critic_tau=0.01,
        encoder_feature_dim=50, encoder_lr=1e-3, encoder_tau=0.05, num_layers=4, num_filters=32, log_interval=10 ** 9)
    rb = curla_amd.ReplayBuffer((C, H, W), (2,), capacity, B, dev, aug, prioritized=prioritized)
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
    if prioritized:  # a spread of priorities, as a run that has been learning for a while has
        vals = torch.empty(capacity, device=dev).uniform_(0.05, 2.0, generator=g) ** 0.6
        rb.update_priorities(torch.arange(capacity, device=dev), vals)
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


def one(capacity, prioritized, updates, samples):
    from curla_amd import ops
    agent, rb = build(capacity, prioritized)
    L, step = _Log(), [1]

    def update():
        agent.update(rb, L, step[0])
        step[0] += 1
    timed(update, 20)  # warm-up: code objects, workspaces
    out = dict(update_us=timed(update, updates), sample_us=timed(rb.sample_cpc_refs, samples))
    if prioritized:
        obs = rb.sample_cpc_refs()[0]
        ws, per = agent._ws(B), obs.per
        lay = rb.block_layout()
        dev_blk = rb._sample_slots[rb._sample_slot]["dev"]
        out["per_sample_us"] = event_us(lambda: ops.per_sample(rb._per_s, rb._per_sums, dev_blk, lay["u"], lay["prob"], B), 200)
        # (per_td rescales the same dq in place at every repetition: the values drift, the work per launch does not)
        out["per_td_us"] = event_us(lambda: ops.per_td(ws.q, B, ws.target_q, per.prob, 0.4, 1e-6, 0.6, B, ws.dq,
                                                       ws.scalars[0:1], ws.per_w, ws.per_value), 200)
        out["per_set_td_us"] = event_us(lambda: ops.per_set(rb._per_s, rb._per_sums, rb._per_max, B, rows=per.rows,
                                                            values=ws.per_value), 200)
        out["per_set_add_us"] = event_us(lambda: ops.per_set(rb._per_s, rb._per_sums, rb._per_max, 1, first_row=7), 200)
    del agent, rb
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--capacity", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--updates", type=int, default=200)
    ap.add_argument("--samples", type=int, default=300)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("per_bench.py measures on the GPU: no HIP device")
    runs = {False: [], True: []}
    for _ in range(args.reps):
        for p in (False, True):
            runs[p].append(one(args.capacity, p, args.updates, args.samples))
    res = dict(config="BASELINE.json configs[1]: B=512, 84x84x9 -> 76x76, hidden 1024", capacity=args.capacity,
               reps=args.reps, updates=args.updates, samples=args.samples)
    lines = []
    for p in (False, True):
        for key in sorted(runs[p][0]):
            v = [r[key] for r in runs[p]]
            res["%s/%s" % ("prioritized" if p else "plain", key)] = dict(median=statistics.median(v), min=min(v), max=max(v))
            lines.append("%-12s %-16s median %9.1f us  (min %9.1f, max %9.1f)" % ("prioritized" if p else "plain", key,
                                                                                 statistics.median(v), min(v), max(v)))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write("tools/per_bench.py --capacity %d --reps %d --updates %d --samples %d\n%s\n" %
                    (args.capacity, args.reps, args.updates, args.samples, res["config"]))
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
