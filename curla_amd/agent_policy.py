"""CurlSacAgent's policy head: the reference's squashed Gaussian or DrQ-v2's deterministic policy."""
import numpy as np
import torch

from . import ops
from .mlp import _Mlp, _mlp_fwd
from .networks import _check_policy_std, _check_policy_std_clip


def _check_policy(policy):
    if policy not in ("gaussian", "deterministic"):
        raise ValueError("policy: %r is not 'gaussian' or 'deterministic'" % (policy,))
    return policy


def _check_policy_std_schedule(sched):
    """DrQ-v2's ``linear(init, final, duration)`` as a tuple of three floats: init and final finite and > 0, duration
    finite and > 0; or None."""
    if sched is None:
        return None
    try:
        init, final, duration = (float(v) for v in sched)
    except (TypeError, ValueError):
        raise ValueError("policy_std_schedule: %r is not None or (init, final, duration)" % (sched,)) from None
    if not (np.isfinite(init) and np.isfinite(final) and np.isfinite(duration) and init > 0 and final > 0 and duration > 0):
        raise ValueError("policy_std_schedule: (%r, %r, %r) is not (init > 0, final > 0, duration > 0), all finite"
                         % (init, final, duration))
    return init, final, duration


def _linear_schedule(sched, step):
    """DrQ-v2's linear(init, final, duration) at ``step``: init + (final - init) * min(step / duration, 1)."""
    init, final, duration = sched
    return init + (final - init) * min(step / duration, 1.0)


def _policy_keywords(agent, policy, policy_std, policy_std_clip, policy_std_schedule):
    """The class call's policy keywords, checked, onto the agent under construction (gaussian: the instance is the one
    without the keyword, and the three ``policy_std*`` keywords raise)."""
    if _check_policy(policy) == "deterministic":
        agent.policy = "deterministic"
        agent.policy_std_schedule = _check_policy_std_schedule(policy_std_schedule)
        agent._policy_std = _check_policy_std(policy_std)
        if agent.policy_std_schedule is not None:  # (the schedule's value at step 0 until the first update)
            agent._policy_std = _check_policy_std(_linear_schedule(agent.policy_std_schedule, 0))
        agent.policy_std_clip = _check_policy_std_clip(policy_std_clip)
        return
    for name, value, default in (("policy_std", policy_std, 0.2), ("policy_std_clip", policy_std_clip, 0.3),
                                 ("policy_std_schedule", policy_std_schedule, None)):
        if value is not default and value != default:
            raise ValueError("%s = %r needs policy='deterministic' (the Gaussian policy learns its own standard "
                             "deviation)" % (name, value))


class _PolicyMixin:
    """CurlSacAgent's policy methods; the settings come from the class call (_policy_keywords)."""

    policy = "gaussian"
    policy_std_clip = None
    policy_std_schedule = None
    _policy_std = None

    def _actor_kw(self):
        """The keyword that shapes the actor, for every place that builds one."""
        return dict(deterministic=True) if self.policy == "deterministic" else {}

    def _actor_out_dim(self):
        """The width of the actor trunk's last layer: [mu | raw log_std], or the deterministic policy's A means."""
        return self.action_dim if self.policy == "deterministic" else 2 * self.action_dim

    def _place_policy_scalars(self):
        """__init__, once the parameters lie in their flat buffers: the standard deviation the deterministic head
        kernels read on the device, and where the actor loss launches leave their d(alpha loss)/d(log_alpha) --
        log_alpha.grad stays all zeros, so its Adam step leaves it bit for bit alone."""
        if self.policy == "deterministic":
            self.actor.std = torch.full((1,), self._policy_std, device=self.device, dtype=torch.float32)
            self.actor.std_clip = self.policy_std_clip
            self._dla_scratch = torch.zeros((), device=self.device, dtype=torch.float64)

    def _policy_clip(self):
        """``policy_std_clip`` as it stands now (it may have been edited), checked; the actor's follows the agent's."""
        clip = self.actor.std_clip = _check_policy_std_clip(self.policy_std_clip)
        return clip

    @property
    def policy_std(self):
        """The deterministic policy's current standard deviation (None: the Gaussian policy); ``set_policy_std``."""
        return self._policy_std

    def set_policy_std(self, value):
        """Set the deterministic policy's standard deviation: one fill of the device scalar the head kernels read,
        enqueued on the current stream and only when the value changes; the host is never synchronised and no captured
        graph holds the value."""
        if self.policy != "deterministic":
            raise ValueError("set_policy_std needs policy='deterministic'")
        value = _check_policy_std(value)
        if value != self._policy_std:
            self._policy_std = value
            self.actor.std.fill_(value)

    def _policy_schedule_step(self, step):
        """The top of ``update()``, before the eager / graph route is chosen (std is data): the schedule's value."""
        if self.policy_std_schedule is not None:
            self.set_policy_std(_linear_schedule(_check_policy_std_schedule(self.policy_std_schedule), step))

    def _actor_fwd(self, ws, noise=None, **outs):
        """The actor trunk over ws.z_a into ws.a_out; with ``noise``, the policy head behind it, which writes ``outs``
        (ops.actor_head_fwd's: mu, pi, log_pi, log_std, tanh_ls, xa, rng; the deterministic head has no tanh_ls and
        clips its scaled noise to ``policy_std_clip``)."""
        B, F = ws.z_a.shape
        if self.policy == "deterministic":
            outs.pop("tanh_ls", None)
            head = None if noise is None else (noise, self.actor.std, self._policy_clip(), outs, "det")
        else:
            head = None if noise is None else (noise, self.actor.log_std_min, self.actor.log_std_max, outs)
        _mlp_fwd(ws.z_a, 0, _Mlp(self.actor.trunk), 1, B, F, self.hidden_dim, self._actor_out_dim(), ws.a_h1, ws.a_h2,
                 ws.a_out, head=head)

    # -- the actor phase's three policy-dependent places (update_actor_and_alpha)
    def _actor_phase_outs(self, ws):
        """What the actor phase asks the head for (the deterministic head leaves its action in xa alone)."""
        return dict(mu=ws.mu, pi=None if self.policy == "deterministic" else ws.pi, log_pi=ws.log_pi,
                    log_std=ws.log_std, tanh_ls=ws.tanh_ls, xa=ws.xa)

    def _dlog_alpha(self):
        """Where the actor loss launches leave d(alpha loss)/d(log_alpha) (the deterministic policy: log_pi = 0 and the
        temperature takes no part -- a scratch word)."""
        return self._dla_scratch if self.policy == "deterministic" else self.log_alpha.grad

    def _actor_head_bwd(self, ws, nz, B, A, F):
        """d(loss)/d(trunk output) into ws.a_dout from d(loss)/d(pi) = the action columns of ws.dxa summed over the
        twin, read in place."""
        if self.policy == "deterministic":
            ops.det_head_bwd(None, ws.mu, B, A, ws.a_dout, twin_dxa=ws.dxa, F=F)
        else:
            ops.actor_head_bwd(None, self.log_alpha, 1.0 / B, nz, ws.pi, ws.log_std, ws.tanh_ls, B, A,
                               self.actor.log_std_min, self.actor.log_std_max, ws.a_dout, twin_dxa=ws.dxa, F=F)

    def _log_actor(self, ws, L, step, alpha=False):
        """The actor phase's lines on a logging step: behind its loss, and (``alpha``) behind its optimizer steps; the
        deterministic policy has no entropy term and no temperature."""
        det = self.policy == "deterministic"
        if alpha:
            if not det:
                L.log('train_alpha/loss', ws.scalars[2], step)
                L.log('train_alpha/value', ws.scalars[4], step)
            return
        L.log('train_actor/loss', ws.scalars[1], step)
        if det:
            L.log('train_actor/std', self._policy_std, step)
        else:
            L.log('train_actor/target_entropy', self.target_entropy, step)
            L.log('train_actor/entropy', ws.scalars[3], step)

    # ------------------------------------------------------------------ graphs, checkpoints
    def _policy_graph_key(self):
        """The policy's part of _graph_key (gaussian: none; the deterministic policy's std is data the head kernels read
        on the device and is not here, its clip is a kernel argument)."""
        return (("policy", "deterministic", self._policy_clip()),) if self.policy == "deterministic" else ()

    def _policy_checkpoint(self):
        if self.policy != "deterministic":
            return {}  # (gaussian: the file of an agent without the keyword)
        return {"policy": "deterministic", "policy_std": float(self._policy_std),
                "policy_std_clip": self.policy_std_clip, "policy_std_schedule": self.policy_std_schedule}

    def _load_policy_checkpoint(self, ck):
        """(A checkpoint of the other policy has failed before, on the size of actor.trunk.4.)"""
        if self.policy == "deterministic" and ck.get("policy") == "deterministic":
            self.policy_std_clip = _check_policy_std_clip(ck["policy_std_clip"])
            self.policy_std_schedule = _check_policy_std_schedule(ck["policy_std_schedule"])
            self.set_policy_std(ck["policy_std"])
