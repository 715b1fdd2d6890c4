#!/usr/bin/env python3
"""The autograd path's numbers (curla_amd/autograd.py):

1. the observation-gradient kernel (curla_conv1_dgrad) against PyTorch-ROCm's own input gradient
   (torch.nn.grad.conv2d_input, NCHW fp32) at configs[1] (B = 512, 9 x 76 x 76) and at the shipped 76 x 135 geometry:
   us per launch and algorithmic TB/s (g read once, dobs written once);
2. a user-written autograd critic step -- forward, backward, FlatAdam.step -- against the internal update_critic at
   B = 512 (for information: the internal phase shares passes the reference's autograd cannot).

Prints one line per measurement and a JSON summary line."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as Fn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timeit(fn, iters=50, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3  # us


def dgrad(B, C, H, W, F=32, iters=50):
    from curla_amd import ops
    Ho, Wo = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    g = torch.randn((B, Ho, Wo, F), device="cuda")
    w = torch.randn((F, C, 3, 3), device="cuda")
    dobs = torch.empty((B, C, H, W), device="cuda")
    g_nchw = g.permute(0, 3, 1, 2).contiguous()
    bytes_ = 4 * (g.numel() + dobs.numel())
    ours = timeit(lambda: ops.conv1_dgrad(g, w, dobs), iters)
    theirs = timeit(lambda: torch.nn.grad.conv2d_input((B, C, H, W), w, g_nchw, stride=2), iters)
    ref = torch.nn.grad.conv2d_input((B, C, H, W), w.double(), g_nchw.double(), stride=2) / 255.0
    err = float((dobs.double() - ref).abs().max() / ref.abs().max())
    r = dict(shape=[B, C, H, W], filters=F, us=round(ours, 1), TBps=round(bytes_ / ours / 1e6, 2),
             torch_conv2d_input_us=round(theirs, 1), torch_TBps=round(bytes_ / theirs / 1e6, 2), MB=round(bytes_ / 1e6, 1),
             rel_err=err)
    print(f"conv1_dgrad {B}x{C}x{H}x{W} F={F}: {ours:7.1f} us ({r['TBps']:.2f} TB/s of {r['MB']} MB)   "
          f"torch conv2d_input {theirs:7.1f} us ({r['torch_TBps']:.2f} TB/s)   rel err {err:.1e}")
    return r


def critic_step(B=512, shape=(9, 84, 84), out_hw=(76, 76), iters=20):
    import curla_amd
    aug = curla_amd.RandomCrop(shape[1:], out_hw)
    torch.manual_seed(0)
    agent = curla_amd.CurlSacAgent((shape[0],) + out_hw, (6,), torch.device("cuda"), aug, hidden_dim=1024,
                                   encoder_feature_dim=50, log_interval=10 ** 9)
    rb = curla_amd.ReplayBuffer(shape, (6,), 2 * B, B, torch.device("cuda"), aug)
    rs = np.random.RandomState(0)
    n = 2 * B
    rb.add_batch(rs.randint(0, 256, (n,) + shape, dtype=np.uint8), rs.uniform(-1, 1, (n, 6)).astype(np.float32),
                 rs.randn(n).astype(np.float32), rs.randint(0, 256, (n,) + shape, dtype=np.uint8), np.zeros(n, bool))

    class Log:
        def log(self, *a, **k):
            pass
    obs, act, rew, nxt, nd, _ = rb.sample_cpc()  # float NCHW minibatch, as the reference's sample_cpc hands over
    refs = rb.sample_cpc_refs()

    def internal():
        o, a, r, no, d, _ = refs
        agent.update_critic(o, a, r, no, d, Log(), 1)

    def user():
        with torch.no_grad():
            _, pi_n, logpi_n, _ = agent.actor(nxt)
            tq1, tq2 = agent.critic_target(nxt, pi_n)
            target = rew + nd * agent.discount * (torch.min(tq1, tq2) - agent.alpha.detach() * logpi_n)
        q1, q2 = agent.critic(obs, act)
        loss = Fn.mse_loss(q1, target) + Fn.mse_loss(q2, target)
        agent.critic_optimizer.zero_grad()
        loss.backward()
        agent.critic_optimizer.step()
    t_int = timeit(internal, iters)
    t_user = timeit(user, iters)
    print(f"critic step B={B}: update_critic {t_int / 1e3:7.3f} ms   user autograd (forward, backward, FlatAdam.step) "
          f"{t_user / 1e3:7.3f} ms  ({t_user / t_int:.2f}x)")
    return dict(B=B, update_critic_ms=round(t_int / 1e3, 3), user_autograd_ms=round(t_user / 1e3, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--skip-critic", action="store_true")
    args = ap.parse_args()
    out = dict(dgrad=[dgrad(512, 9, 76, 76, iters=args.iters), dgrad(512, 9, 76, 135, iters=args.iters)])
    if not args.skip_critic:
        out["critic_step"] = critic_step()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
