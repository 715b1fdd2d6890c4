#!/usr/bin/env python3
"""Cost of storing one vector step: ``ReplayBuffer.add_vec`` on an ``n_envs=N`` buffer against N ``add`` calls on an
``n_envs=1`` buffer.  84x84x9 uint8 observations, A = 2, both buffers with ``--n-step`` (default 3, so
the continuity flags are kept and compared).  Two clocks per form, over ``--calls`` vector steps: the host's (wall time
of the enqueueing loop; nothing in it waits for the GPU unless the four pinned add slots are all in flight) and the
device's (stream events around the same loop).  The two forms alternate ``--reps`` times after a warm-up; the median and
the spread (min .. max) of the per-step times are printed, one JSON line per N."""
import argparse, json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import curla_amd

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, nargs="+", default=[4, 16], metavar="N")
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--n-step", type=int, default=3)
args = ap.parse_args()
dev = torch.device("cuda")
aug = curla_amd.RandomCrop((84, 84), (76, 76))
C, HW, A, CAP = 9, (84, 84), 2, 4096
kw = dict(n_step=args.n_step, discount=0.99) if args.n_step > 1 else {}


def timed(step, calls):
    """(host us, device us) per call of ``step`` over ``calls`` calls."""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    for _ in range(calls):
        step()
    t1 = time.perf_counter()
    e1.record()
    torch.cuda.synchronize()
    return (t1 - t0) / calls * 1e6, e0.elapsed_time(e1) / calls * 1e3


for N in args.envs:
    rs = np.random.RandomState(N)
    obs = rs.randint(0, 256, (N, C) + HW, dtype=np.uint8)
    nxt = rs.randint(0, 256, (N, C) + HW, dtype=np.uint8)
    act, rew, done = rs.uniform(-1, 1, (N, A)).astype(np.float32), rs.randn(N).astype(np.float32), np.zeros(N, dtype=bool)
    vec = curla_amd.ReplayBuffer((C,) + HW, (A,), CAP // N * N, 512, dev, aug, n_envs=N, **kw)
    one = curla_amd.ReplayBuffer((C,) + HW, (A,), CAP // N * N, 512, dev, aug, **kw)

    def step_vec():
        vec.add_vec(obs, act, rew, nxt, done)

    def step_one():
        for e in range(N):
            one.add(obs[e], act[e], rew[e], nxt[e], done[e])
    for _ in range(20):
        step_vec(), step_one()
    tv, to = [], []
    for _ in range(args.reps):
        tv.append(timed(step_vec, args.calls))
        to.append(timed(step_one, args.calls))
    out = dict(N=N, calls=args.calls, reps=args.reps, n_step=args.n_step)
    for name, t in (("add_vec", np.array(tv)), ("n_adds", np.array(to))):
        for j, clock in enumerate(("host_us", "device_us")):
            out[f"{name}_{clock}"] = dict(median=round(float(np.median(t[:, j])), 1), min=round(float(t[:, j].min()), 1),
                                          max=round(float(t[:, j].max()), 1))
    for clock in ("host_us", "device_us"):
        out[f"ratio_{clock}"] = round(out[f"n_adds_{clock}"]["median"] / out[f"add_vec_{clock}"]["median"], 2)
    # the launch alone, back to back on the block the last step staged (no host staging, no copy): what the stream is
    # busy with per step when the host is not the limit
    from curla_amd import ops
    cont = vec._cont if args.n_step > 1 else None
    tk = [timed(lambda: ops.add_vec(vec._d_add, vec.obses, vec.next_obses, vec._sc, cont, N, cont is not None, N),
                args.calls)[1] for _ in range(args.reps)]
    out["add_vec_kernel_us"] = dict(median=round(float(np.median(tk)), 1), min=round(min(tk), 1), max=round(max(tk), 1))
    print(json.dumps(out), flush=True)
