"""CurlSacAgent's dormant-neuron scores and ReDo recycling (Sokar et al., ICML 2023) for the hidden layers of the twin Q
functions and the actor trunk: a no-grad pass over a minibatch, the scores and masks on the device, the masked units'
incoming weights re-initialised from the reset stream, their outgoing weights and Adam moments zeroed."""
import math
import numbers

import numpy as np
import torch
import torch.nn as nn

from . import _lib, ops
from .encoder import CNNEncoder
from .mlp import _linears
from .networks import _check_int
from .ops import ObsRef
from .optim import FlatAdam

# the scored layers, in the order of every per-layer tensor: the post-ReLU outputs of the two hidden layers of a trunk
# (with critic_layer_norm: behind the LayerNorm)
LAYERS = ("Q1.h1", "Q1.h2", "Q2.h1", "Q2.h2", "actor.h1", "actor.h2")


def _check_redo_interval(v):
    """Updates between two redo passes: an ``int >= 0`` (0: never; a bool, a float or a string is not one)."""
    return _check_int(v, 0, None, "redo_interval: %r is not an int >= 0" % (v,))


def _check_redo_tau(v):
    """The dormancy threshold: a real number >= 0 as a float (0: exactly dead units; a bool or a NaN is not one)."""
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or math.isnan(v) or not v >= 0:
        raise ValueError("redo_tau: %r is not a number >= 0" % (v,))
    return float(v)


def _check_redo_recycle(v):
    """Whether a pass recycles what it finds: a bool (an int or a string is not one)."""
    if not isinstance(v, (bool, np.bool_)):
        raise ValueError("redo_recycle: %r is not a bool" % (v,))
    return bool(v)


def _redo_keywords(agent, redo_interval, redo_tau, redo_recycle):
    """The class call's redo keywords, checked, onto the agent under construction."""
    agent.redo_interval = _check_redo_interval(redo_interval)
    agent.redo_tau = _check_redo_tau(redo_tau)
    agent.redo_recycle = _check_redo_recycle(redo_recycle)


def _trunk_segments(seq, base, l1, l2):
    """The segments of ops.redo_recycle for a trunk Linear [- LayerNorm] - ReLU - Linear [- LayerNorm] - ReLU - Linear
    whose parameters lie in one flat buffer, offsets counted in floats from the address ``base``; ``l1`` / ``l2``: the
    mask rows of its two hidden layers.  The last Linear's bias belongs to no hidden unit and is not in the list."""
    lin = _linears(seq)
    lns = [m for m in seq if isinstance(m, nn.LayerNorm)]
    H = lin[0].out_features

    def off(p):
        return (p.data_ptr() - base) // 4
    segs = [(off(lin[0].weight), H, lin[0].in_features, l1, -1), (off(lin[0].bias), H, 1, l1, -1),
            (off(lin[1].weight), H, H, l2, l1), (off(lin[1].bias), H, 1, l2, -1),
            (off(lin[2].weight), lin[2].out_features, H, -1, l2)]
    for ln, layer in zip(lns, (l1, l2)):
        segs += [(off(ln.weight), H, 1, layer, -1), (off(ln.bias), H, 1, layer, -1)]
    return segs


class _RedoMixin:
    """CurlSacAgent's redo methods; the settings (``redo_interval``, ``redo_tau``, ``redo_recycle``) come from the class
    call (_AgentType), the fresh values from _ResetMixin's reset stream."""

    redo_interval = 0     # a redo pass at the end of every update whose step is a multiple of this (0: never)
    redo_tau = 0.1        # a unit is dormant when its score is <= this
    redo_recycle = True   # False: a pass scores and counts only
    redo_count = 0        # passes made so far
    _redo_buf = None      # the device buffers of a pass, made on first use

    # ------------------------------------------------------------------ public surface
    @property
    def dormant_counts(self):
        """int32 device tensor [6]: the dormant units per layer (``agent_redo.LAYERS``) of the last pass; None before
        the first."""
        return None if self._redo_buf is None else self._redo_buf["count"]

    @property
    def dormant_fractions(self):
        """float32 device tensor [6]: ``dormant_counts / hidden_dim`` of the last pass; None before the first."""
        return None if self._redo_buf is None else self._redo_buf["fraction"]

    def dormant_report(self):
        """{layer: dormant fraction} of the last pass as Python floats -- this one waits for the device: for user code,
        not for the update loop.  Empty before the first pass."""
        if self._redo_buf is None:
            return {}
        return dict(zip(LAYERS, (float(x) for x in self._redo_buf["fraction"].tolist())))

    # ------------------------------------------------------------------ schedule
    def _redo_due(self, step, only_cpc=False):
        """Whether the update at ``step`` ends with a redo pass."""
        if self.redo_interval == 0 and type(self.redo_interval) is int:
            return False
        interval = _check_redo_interval(self.redo_interval)  # (the attribute may have been edited)
        return interval > 0 and step > 0 and step % interval == 0 and not only_cpc

    def _redo_scheduled(self, obs, action, L, step):
        """The pass at the end of a redo step's ``update()``, on the minibatch of its final sub-step, and its two log
        entries (device scalars, as the losses are logged)."""
        self.redo_pass(obs, action)
        fr = self._redo_buf["fraction"]
        L.log('train_critic/dormant_fraction', fr[:4].mean(), step)
        L.log('train_actor/dormant_fraction', fr[4:].mean(), step)

    # ------------------------------------------------------------------ buffers
    def _redo_buffers(self):
        if self._redo_buf is None:
            n, H, dev = len(LAYERS), self.hidden_dim, self.device
            f = lambda *shape: torch.zeros(shape, device=dev, dtype=torch.float32)  # noqa: E731
            i = lambda *shape: torch.zeros(shape, device=dev, dtype=torch.int32)    # noqa: E731
            self._redo_buf = dict(sums=f(n, H), score=f(n, H), mask=i(n, H), count=i(n), fraction=f(n))
        return self._redo_buf

    def _redo_moments(self, opt, off, n):
        """The addresses of Adam's two moments of the flat elements [off, off + n) of ``opt``'s buffer.  torch's own
        Adam (CURLA_TORCH_ADAM=1) keeps one tensor per parameter, not a mirror of the flat layout: no recycling there.
        (Under the launch-trace hook a CPU agent has torch's Adams too: the launches are traced with NULL moments.)"""
        if isinstance(opt, FlatAdam):
            return opt.moment_addresses(off, n)
        if _lib._trace_hook is not None:
            return None, None
        raise RuntimeError("CurlSacAgent.redo_pass(redo_recycle=True) needs the flat optimizers (FlatAdam): their "
                           "moments mirror the flat parameter layout the recycling kernel walks")

    # ------------------------------------------------------------------ the pass
    @torch.no_grad()
    def redo_pass(self, obs, action):
        """Score the six hidden layers on the minibatch (``obs``: an ObsRef or a float tensor [B, C, H, W]; ``action``
        [B, A]) with the parameters as they are, no dropout, and -- ``redo_recycle`` -- recycle the units whose score is
        <= ``redo_tau``:
          score   : a unit's mean |activation| over the minibatch, divided by its layer's mean; data parallel, the sums
                    are added over the ranks first, so every replica takes the same masks
          recycle : a dormant unit's incoming weights, bias and (critic_layer_norm) LayerNorm weight / bias become
                    freshly initialised ones from the reset stream (``reset_seed``), its outgoing weights 0, Adam's
                    moments 0 at every element written; everything else is not written.  The target critic is not
                    touched (it follows through the soft update), the optimizers' step counts neither
        ``dormant_counts`` / ``dormant_fractions`` hold the result on the device; nothing waits for it here.  A layer
        that holds a NaN counts and recycles nothing: ``reset_networks()`` remains the way back from NaN."""
        self._redo_pass(obs, action)

    @torch.no_grad()
    def _redo_pass(self, obs, action, draw=True):
        """``redo_pass``; ``draw=False`` (tools/redo_bench.py: the device's share of a recycling pass) recycles with
        the values staged last instead of drawing new ones (_upload_fresh)."""
        tau = _check_redo_tau(self.redo_tau)            # (the attributes may have been edited)
        recycle = _check_redo_recycle(self.redo_recycle)
        if self.device.type != "cuda" and _lib._trace_hook is None:
            raise RuntimeError("CurlSacAgent.redo_pass needs a CUDA/HIP device: the learner path has no CPU fallback")
        cf, af, lay = self._critic_flat, self._actor_flat, self._lay
        q0 = (self.critic.Q1.trunk[0].weight.data_ptr() - cf.data_ptr()) // 4
        a0 = (self.actor.trunk[0].weight.data_ptr() - af.data_ptr()) // 4
        qs = self.critic.twin_stride
        assert q0 == lay["q"][0] and qs == lay["qblock"]
        if recycle:  # (before any launch: an agent that cannot recycle has scored nothing either)
            seg_q = _trunk_segments(self.critic.Q1.trunk, cf.data_ptr() + 4 * q0, 0, 1)
            seg_a = _trunk_segments(self.actor.trunk, af.data_ptr() + 4 * a0, 4, 5)
            end = lambda segs: max(s[0] + s[1] * s[2] for s in segs)  # noqa: E731
            mq = self._redo_moments(self.critic_optimizer, q0, qs + end(seg_q))
            ma = self._redo_moments(self.actor_optimizer, a0, end(seg_a))
        self._finish_actor_step()
        o = obs if isinstance(obs, ObsRef) else ObsRef.from_tensor(obs.contiguous().float())
        action = action.contiguous()
        B, A, H = o.B, self.action_dim, self.hidden_dim
        enc, aenc = self.critic.encoder, self.actor.encoder
        ws, buf = self._ws(B), self._redo_buffers()

        # the forward: the tied convs once, the critic's and the actor's fc / ln on their output, the twins over
        # [z, action] and the actor trunk over its z -- the no-grad buffers of the workspace, no saves, no dropout
        h = enc.conv_forward(o, ws.acts_tmp)
        CNNEncoder.fc_partial_multi([(aenc, h), (enc, h)])
        CNNEncoder.ln_from_partial_multi(B, [(aenc, ws.z_a, {}), (enc, ws.z_c, dict(xa=ws.xa, act=action))], A)
        self._twin_fwd(ws, self.critic, self.critic.twin_ln(), ws.q)
        self._actor_fwd(ws)

        # sums [6][H]: the twins' layers interleave (Q1.h1, Q1.h2, Q2.h1, Q2.h2), so a twin launch writes every other row
        sums, n = buf["sums"], len(LAYERS)
        ops.dormant_colsum(ws.q_h1, B * H, 2, B, H, sums[0], 2 * H)
        ops.dormant_colsum(ws.q_h2, B * H, 2, B, H, sums[1], 2 * H)
        ops.dormant_colsum(ws.a_h1, B * H, 1, B, H, sums[4], H)
        ops.dormant_colsum(ws.a_h2, B * H, 1, B, H, sums[5], H)
        self._redo_allreduce(sums)
        ops.dormant_mask(sums, n, H, tau, buf["score"], buf["mask"], buf["count"], buf["fraction"])

        if recycle:
            stage = self._upload_fresh(draw)
            # one launch per flat buffer: the twins (Q2 a block behind Q1, its mask rows two further on), the actor trunk
            ops.redo_recycle(cf[q0:], mq[0], mq[1], stage["critic"]["dev"][q0:], qs, 2, seg_q, buf["mask"], n, H, 2)
            ops.redo_recycle(af[a0:], ma[0], ma[1], stage["actor"]["dev"][a0:], af.numel() - a0, 1, seg_a, buf["mask"],
                             n, H, 0)
        self._drop_encoder_caches()
        self.redo_count += 1

    def _redo_allreduce(self, sums):
        """Data parallel: the ranks' column sums added up (SUM, not the gradients' average: |h| summed over the global
        batch), in place -- one collective."""
        if not self._dp_active:
            return
        import torch.distributed as dist
        if self._dp_staged:  # (a backend staged through the host, as _allreduce stages it)
            host = sums.detach().cpu()
            dist.all_reduce(host, op=dist.ReduceOp.SUM, group=self._dp_group)
            sums.copy_(host)
        else:
            dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=self._dp_group)

    # ------------------------------------------------------------------ checkpoints
    def _redo_checkpoint(self):
        """The three settings and the count -- of an agent that has the feature on or has made a pass: a file of an
        agent that never used it has the keys it always had."""
        if not self.redo_interval and not self.redo_count:
            return {}
        return {"redo_interval": int(self.redo_interval), "redo_tau": float(self.redo_tau),
                "redo_recycle": bool(self.redo_recycle), "redo_count": int(self.redo_count)}

    def _load_redo_checkpoint(self, ck):
        """The count comes from the file (a file without the keys: 0 passes); the settings stay the agent's own."""
        self.redo_count = int(ck.get("redo_count", 0))
