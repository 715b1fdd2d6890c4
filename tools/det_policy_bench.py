"""What the deterministic DrQ-v2 policy costs at BASELINE.json configs[1] (B = 512, 84x84x9 -> random_crop 76x76,
hidden 1024, eager).

python tools/det_policy_bench.py [--policies gaussian,deterministic] [--capacity 100000] [--reps 3] [--updates 200] [--out FILE]

``CurlSacAgent(policy=...)`` for every policy of ``--policies`` on the same build, alternating: time per whole
``update()`` (host clock around back-to-back calls that end in a synchronise) and the time of the policy's head launches
alone on the agent's own workspace (HIP events around back-to-back launches): the actor's last layer with the head in
it, and the head's backward.  ``none`` builds the agent without the keyword, so ``--policies none`` also runs on a
checkout from before it: alternate the two checkouts to see that nothing else moved.  The spread the figures have to be
read against is each row's (min, max) over ``--reps``.  Prints one JSON line; ``--out`` also writes a text table."""
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


def build(capacity, policy):
    import curla_amd
    from curla_amd import augmentations as A
    dev = torch.device("cuda")
    curla_amd.set_seed_everywhere(1)
    aug = A.RandomCrop((H, W), CROP)
    kw = {} if policy == "none" else dict(policy=policy)
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


def one(capacity, policy, updates):
    agent, rb = build(capacity, policy)
    L, step = _Log(), [1]

    def update():
        agent.update(rb, L, step[0])
        step[0] += 1
    timed(update, 20)  # warm-up: code objects, workspaces
    out = dict(update_us=timed(update, updates))
    from curla_amd import ops
    from curla_amd.mlp import _Mlp
    ws, A = agent._ws(B), agent.action_dim
    P, F = _Mlp(agent.actor.trunk), agent.actor.encoder.feature_dim
    outs = dict(mu=ws.mu, log_pi=ws.log_pi, log_std=ws.log_std, xa=ws.xa)
    if getattr(agent, "policy", "gaussian") == "deterministic":
        out["head_fwd_us"] = event_us(lambda: ops.mlp_out_det_head_fwd(
            ws.a_h2, P.W[2], P.b[2], ws.a_out, ws.noise, B, A, HIDDEN, agent.actor.std, agent.policy_std_clip, **outs), 200)
        out["head_bwd_us"] = event_us(lambda: ops.det_head_bwd(None, ws.mu, B, A, ws.a_dout, twin_dxa=ws.dxa, F=F), 200)
    else:
        lo, hi = agent.actor.log_std_min, agent.actor.log_std_max
        out["head_fwd_us"] = event_us(lambda: ops.mlp_out_head_fwd(
            ws.a_h2, P.W[2], P.b[2], ws.a_out, ws.noise, B, A, HIDDEN, lo, hi, pi=ws.pi, tanh_ls=ws.tanh_ls, **outs), 200)
        out["head_bwd_us"] = event_us(lambda: ops.actor_head_bwd(
            None, agent.log_alpha, 1.0 / B, ws.noise, ws.pi, ws.log_std, ws.tanh_ls, B, A, lo, hi, ws.a_dout,
            twin_dxa=ws.dxa, F=F), 200)
    del agent, rb
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--policies", default="gaussian,deterministic")
    ap.add_argument("--capacity", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--updates", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("det_policy_bench.py measures on the GPU: no HIP device")
    policies = args.policies.split(",")
    runs = {p: [] for p in policies}
    for _ in range(args.reps):
        for p in policies:
            runs[p].append(one(args.capacity, p, args.updates))
    res = dict(config="BASELINE.json configs[1]: B=512, 84x84x9 -> 76x76, hidden 1024", capacity=args.capacity,
               reps=args.reps, updates=args.updates)
    lines = []
    for p in policies:
        for key in sorted(runs[p][0]):
            vals = [r[key] for r in runs[p]]
            res["policy=%s/%s" % (p, key)] = dict(median=statistics.median(vals), min=min(vals), max=max(vals))
            lines.append("policy=%-13s  %-12s median %9.1f  (min %9.1f, max %9.1f)" %
                         (p, key, statistics.median(vals), min(vals), max(vals)))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write("tools/det_policy_bench.py --policies %s --capacity %d --reps %d --updates %d\n%s\n" %
                    (args.policies, args.capacity, args.reps, args.updates, res["config"]))
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
