"""The deterministic DrQ-v2 policy (CurlSacAgent(policy="deterministic")) restated in float64 from its
definition, not from the kernels: the head per element -- vectorised and as plain loops --, its gradient, the std
schedule, the head's Philox normals (on tests/_dropout_ref.philox4x32_10) and the pieces of the critic / actor phases
on explicit parameters (the oracle's encoder and MLPs produce the trunk output, this file the policy and the TD target).

Per row b and action a, with o the actor trunk's output [B, A], n a standard-normal draw, s the standard deviation (a
float32), c the noise clip (None: none) and lim = float32(1 - 1e-6):

    m      = tanh(o)                          (mu)
    e      = clamp(s n, -c, c)
    pi     = clamp(m + e, -lim, lim)
    log_pi = 0,  log_std = log(s)
    d pi / d o = 1 - m^2                      (straight through the outer clamp; e depends on no parameter)

Value and gradient are continuous in every input: a float64 evaluation on the same float32 inputs is a fair arbiter
everywhere, the clamps' kinks included."""
import math

import numpy as np
import torch

from tests._dropout_ref import philox4x32_10

LIM = float(np.float32(1.0 - 1e-6))


def _f64(x):
    return x.detach().double().cpu() if torch.is_tensor(x) else torch.as_tensor(np.asarray(x), dtype=torch.float64)


def forward(o, noise, std, clip):
    """dict(mu, pi, log_pi, log_std) in float64; ``noise`` None: no pi.  ``std`` a float (the float32's value)."""
    o = _f64(o)
    s = float(np.float32(std))
    m = torch.tanh(o)
    out = dict(mu=m, log_pi=torch.zeros(o.shape[0], 1, dtype=torch.float64),
               log_std=torch.full_like(o, math.log(s)), pi=None)
    if noise is not None:
        e = s * _f64(noise)
        if clip is not None:
            e = e.clamp(-float(clip), float(clip))
        out["pi"] = (m + e).clamp(-LIM, LIM)
    return out


def forward_loops(o, noise, std, clip):
    """``forward``'s mu and pi as plain Python loops over rows and actions (lists of lists of floats)."""
    s = float(np.float32(std))
    o, noise = np.asarray(o, dtype=np.float64), np.asarray(noise, dtype=np.float64)
    mu, pi = [], []
    for b in range(o.shape[0]):
        mu.append([]), pi.append([])
        for a in range(o.shape[1]):
            m = math.tanh(o[b, a])
            e = s * noise[b, a]
            if clip is not None:
                e = max(-float(clip), min(float(clip), e))
            mu[-1].append(m)
            pi[-1].append(max(-LIM, min(LIM, m + e)))
    return mu, pi


def grad_o(o, dpi=None, dmu=None):
    """d o = (dmu + dpi)(1 - tanh(o)^2) in float64 (None = zero)."""
    o = _f64(o)
    g = torch.zeros_like(o)
    for d in (dpi, dmu):
        if d is not None:
            g = g + _f64(d)
    return g * (1.0 - torch.tanh(o) ** 2)


def policy(o, noise, std, clip):
    """(mu, pi) as differentiable float64 tensors of a float64 ``o`` that may require grad: the outer clamp is straight
    through, as DrQ-v2's ``_clamp`` (x + (clamp(x) - x).detach())."""
    s = float(np.float32(std))
    m = torch.tanh(o)
    e = s * noise.double()
    if clip is not None:
        e = e.clamp(-float(clip), float(clip))
    x = m + e
    return m, x + (x.clamp(-LIM, LIM) - x).detach()


def linear(schedule, step):
    """DrQ-v2's linear(init, final, duration) at ``step``."""
    init, final, duration = schedule
    return init + (final - init) * min(step / duration, 1.0)


def philox_normals(seed, offset, n):
    """The head's in-kernel draw (include/curla_hip.h): element i = Box-Muller, in float32, on outputs (i % 4) & 2, + 1 of
    Philox4x32-10 with key ``seed`` and counter ``offset + i // 4``; cos for even i, sin for odd.  float32 [n]."""
    m = (n + 3) // 4
    ctr = np.uint64(int(offset) & (2 ** 64 - 1)) + np.arange(m, dtype=np.uint64)
    zero = np.zeros(m, dtype=np.uint64)
    seed = int(seed) & (2 ** 64 - 1)
    r = np.stack(philox4x32_10((ctr & np.uint64(0xFFFFFFFF), ctr >> np.uint64(32), zero, zero),
                               (seed & 0xFFFFFFFF, seed >> 32)), axis=1)
    out = np.empty((m, 4), np.float32)
    for h in range(2):
        a, b = r[:, 2 * h] >> np.uint64(8), r[:, 2 * h + 1] >> np.uint64(8)
        u1 = (a.astype(np.float32) + np.float32(1)) * np.float32(1.0 / 16777216.0)
        u2 = b.astype(np.float32) * np.float32(1.0 / 16777216.0)
        rad = np.sqrt(np.float32(-2) * np.log(u1))
        ang = np.float32(6.283185307179586) * u2
        out[:, 2 * h], out[:, 2 * h + 1] = rad * np.cos(ang), rad * np.sin(ang)
    return out.reshape(-1)[:n]


# ------------------------------------------------------------------ pieces of the phases, on explicit float64 parameters
def _trunk_out(O, actor, critic, obs, layers, detach_encoder=False, plan=None):
    """The deterministic actor's trunk output o [B, A]: the critic's (tied) convs, the actor's fc / ln / trunk."""
    merged = dict(actor)
    merged.update({k: v for k, v in critic.items() if k.startswith("encoder.convs.")})
    z = O.encoder_forward(merged, "encoder.", obs, layers, detach=detach_encoder)
    return O.mlp3(merged, "trunk.", z, plan)


def next_action(O, actor, critic, next_obs, noise, std, clip, layers):
    """a' = pi(next_obs) of the online actor, no gradient."""
    with torch.no_grad():
        return policy(_trunk_out(O, actor, critic, next_obs, layers), noise, std, clip)[1]


def td_target(tq1, tq2, reward, not_done, discount):
    """The entropy-free TD target r + not_done * discount * min Q' ([B, 1] each); n-step: ``reward`` and ``discount`` are
    the composed ones."""
    return reward + not_done * discount * torch.minimum(tq1, tq2)
