"""What the self-predictive representation phase costs beside the InfoNCE one at BASELINE.json configs[1] (B = 512,
84x84x9 -> random_crop 76x76, hidden 1024).

python tools/pred_bench.py [--objectives infonce,predictive] [--capacity 100000] [--reps 3] [--updates 200] [--out FILE]

``CurlSacAgent(cpc_objective=...)`` for every objective of ``--objectives`` on the same build and the same
``ReplayBuffer(pos_offset=1)``, alternating: time per whole ``update()`` (host clock around back-to-back calls that end in
a synchronise), time of the representation phase alone (HIP events around back-to-back ``update_cpc`` calls on one drawn
minibatch: both encoders' passes, the head, the encoder's backward, the two optimizer steps) and, for the predictive
objective, of ``curla_pred_loss`` alone with and without its mean launch.  ``infonce`` builds the agent without the
keyword, so ``--objectives infonce`` also runs on a checkout from before it: alternate the two checkouts to see that
nothing else moved.  The spread the figures have to be read against is each row's (min, max) over ``--reps``.  Single
runs, nothing is retried.  Prints one JSON line; ``--out`` also writes a text table."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.hlg_bench import B, C, CROP, H, HIDDEN, W, _Log, event_us, timed  # noqa: E402


def build(capacity, objective):
    import curla_amd
    from curla_amd import augmentations as A
    dev = torch.device("cuda")
    curla_amd.set_seed_everywhere(1)
    aug = A.RandomCrop((H, W), CROP)
    kw = dict(cpc_objective=objective) if objective != "infonce" else {}
    agent = curla_amd.CurlSacAgent(
        (C,) + CROP, (2,), dev, aug, hidden_dim=HIDDEN, discount=0.99, init_temperature=0.1, alpha_lr=1e-4,
        alpha_beta=0.5, actor_lr=1e-3, actor_beta=0.9, critic_lr=1e-3, critic_beta=0.9, critic_tau=0.01,
        encoder_feature_dim=50, encoder_lr=1e-3, encoder_tau=0.05, num_layers=4, num_filters=32, log_interval=10 ** 9, **kw)
    rb = curla_amd.ReplayBuffer((C, H, W), (2,), capacity, B, dev, aug, pos_offset=1)
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


def one(capacity, objective, updates):
    agent, rb = build(capacity, objective)
    L, step = _Log(), [1]

    def update():
        agent.update(rb, L, step[0])
        step[0] += 1
    timed(update, 20)  # warm-up: code objects, workspaces
    out = dict(update_us=timed(update, updates))
    obs, action, _, _, _, kw = rb.sample_cpc_refs()
    extra = dict(action=action) if objective == "predictive" else {}
    out["cpc_phase_us"] = event_us(lambda: agent.update_cpc(kw["obs_anchor"], kw["obs_pos"], kw, L, 1, **extra), 200)
    if objective == "predictive":
        from curla_amd import ops
        ws, F = agent._ws(B), agent.critic.encoder.feature_dim
        out["pred_loss_us"] = event_us(lambda: ops.pred_loss(ws.p_out, ws.z_pos, B, F, ws.row_loss, None, ws.p_dout), 200)
        out["pred_loss_with_mean_us"] = event_us(
            lambda: ops.pred_loss(ws.p_out, ws.z_pos, B, F, ws.row_loss, ws.scalars[5:6], ws.p_dout), 200)
    del agent, rb
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objectives", default="infonce,predictive")
    ap.add_argument("--capacity", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--updates", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pred_bench.py measures on the GPU: no HIP device")
    objectives = args.objectives.split(",")
    runs = {o: [] for o in objectives}
    for _ in range(args.reps):
        for o in objectives:
            runs[o].append(one(args.capacity, o, args.updates))
    res = dict(config="BASELINE.json configs[1]: B=512, 84x84x9 -> 76x76, hidden 1024, pos_offset=1", capacity=args.capacity,
               reps=args.reps, updates=args.updates)
    lines = []
    for o in objectives:
        for key in sorted(runs[o][0]):
            vals = [r[key] for r in runs[o]]
            res["cpc_objective=%s/%s" % (o, key)] = dict(median=statistics.median(vals), min=min(vals), max=max(vals))
            lines.append("cpc_objective=%-10s  %-24s median %9.1f  (min %9.1f, max %9.1f)" %
                         (o, key, statistics.median(vals), min(vals), max(vals)))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write("tools/pred_bench.py --objectives %s --capacity %d --reps %d --updates %d\n%s\n" %
                    (args.objectives, args.capacity, args.reps, args.updates, res["config"]))
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
