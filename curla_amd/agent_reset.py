"""CurlSacAgent's periodic network resets: heads re-initialised, encoder shrunk and perturbed, optimizers started over."""
import math
import numbers

import numpy as np
import torch

from . import _lib, ops
from .networks import Actor, Critic, _check_int
from .optim import FlatAdam


def _check_reset_interval(v):
    """Updates between two scheduled resets: an ``int >= 0`` (0: never; a bool, a float or a string is not one)."""
    return _check_int(v, 0, None, "reset_interval: %r is not an int >= 0" % (v,))


def _check_reset_keep(v):
    """The share of the old encoder a reset keeps: a real number in [0, 1] as a float (a bool or a NaN is not one)."""
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or math.isnan(v) or not 0 <= v <= 1:
        raise ValueError("reset_encoder_keep: %r is not a number in [0, 1]" % (v,))
    return float(v)


def _check_reset_seed(v):
    """The seed of the reset stream: an ``int`` a torch generator takes (a bool, a float or a string is not one)."""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not -2 ** 63 <= v < 2 ** 64:
        raise ValueError("reset_seed: %r is not an int (-2**63 .. 2**64 - 1)" % (v,))
    return int(v)


def _reset_keywords(agent, reset_interval, reset_encoder_keep, reset_seed):
    """The class call's reset keywords, checked, onto the agent under construction."""
    agent.reset_interval = _check_reset_interval(reset_interval)
    agent.reset_encoder_keep = _check_reset_keep(reset_encoder_keep)
    agent.reset_seed = _check_reset_seed(reset_seed)


def _zero_torch_adam(opt):
    """A torch.optim.Adam's state back to step 0 with zero moments, every tensor filled in place."""
    for st in opt.state.values():
        for k in ("exp_avg", "exp_avg_sq", "step"):
            if torch.is_tensor(st.get(k)):
                st[k].zero_()


class _ResetMixin:
    """CurlSacAgent's reset methods; the settings (``reset_interval``, ``reset_encoder_keep``, ``reset_seed``) come from
    the class call (_AgentType), the constructor's arguments a fresh network needs from ``__init__`` (``_net_args``,
    ``_init_log_alpha``)."""

    reset_interval = 0         # a scheduled reset every this many steps (0: never); may be edited between calls
    reset_encoder_keep = 1.0   # the share of the old encoder a reset keeps (1: heads only); may be edited between calls
    reset_seed = 0             # the seed of the reset stream
    reset_count = 0            # resets made so far
    _reset_epoch = 0           # step // reset_interval of the last scheduled reset
    _reset_rng = None          # the reset stream: a CPU generator state (ByteTensor), made from reset_seed on first use
    _reset_stage = None        # the staging buffers of the fresh values, made on first use

    # ------------------------------------------------------------------ the reset stream
    def _reset_stream(self):
        if self._reset_rng is None:
            self._reset_rng = torch.Generator().manual_seed(_check_reset_seed(self.reset_seed)).get_state()
        return self._reset_rng

    def _draw_fresh(self):
        """(Actor, Critic, W) on the CPU, constructed as ``__init__`` constructs them and in its order, with torch's CPU
        generator standing at the reset stream's state; the state behind the draws is the stream's new one.  The
        global generator is put back (fork_rng); the device generator and NumPy's state are not involved."""
        obs_shape, action_shape, hidden, feat, ls_min, ls_max, layers, filters = self._net_args
        q_kw = self._critic_width_kw()
        with torch.random.fork_rng(devices=[]):
            torch.set_rng_state(self._reset_stream())
            actor = Actor(obs_shape, action_shape, hidden, feat, ls_min, ls_max, layers, filters, **self._actor_kw())
            critic = Critic(obs_shape, action_shape, hidden, feat, layers, filters, layer_norm=self.critic_layer_norm,
                            dropout=self.critic_dropout, **q_kw)
            W = torch.rand(feat, feat)
            self._reset_rng = torch.get_rng_state()
        return actor, critic, W

    # ------------------------------------------------------------------ staging
    def _reset_staging(self):
        """One staging buffer per flat buffer -- {"critic", "actor"} -> dict(host, dev, event) --, the host side pinned
        beside a HIP device: allocated on first use, reused from then on.  The target flat shares the critic's."""
        if self._reset_stage is None:
            cuda = self.device.type == "cuda"
            self._reset_stage = {
                k: dict(host=torch.zeros(flat.numel(), dtype=torch.float32, pin_memory=cuda), dev=torch.zeros_like(flat),
                        event=None)
                for k, flat in (("critic", self._critic_flat), ("actor", self._actor_flat))}
        return self._reset_stage

    @staticmethod
    def _stage_params(host, flat, live, fresh, fc=None):
        """Write ``fresh``'s tensors into ``host`` where ``live``'s namesakes lie in ``flat`` ([(name, Parameter)] both);
        an encoder's fc.weight goes through ``fc.from_reference_layout``, as _to_flat_device_layout stores it."""
        fresh = dict(fresh)
        base = flat.data_ptr()
        for name, p in live:
            src = fresh[name].detach()
            if name == "encoder.fc.weight":
                src = fc.from_reference_layout(src)
            off = (p.data_ptr() - base) // 4
            assert 0 <= off and off + p.numel() <= host.numel() and src.shape == p.shape, name
            host[off:off + p.numel()].view(p.shape).copy_(src)

    def _stage_fresh(self):
        """Draw the fresh networks and lay them out, as the live ones lie in their flat buffers, in the staging buffers'
        host sides; returns the staging buffers."""
        stage = self._reset_staging()
        for st in stage.values():  # (the copy of the previous reset still reading the host side: wait for it)
            if st["event"] is not None:
                st["event"].synchronize()
        actor, critic, W = self._draw_fresh()
        c, a = stage["critic"]["host"], stage["actor"]["host"]
        self._stage_params(c, self._critic_flat, [("W", self.CURL.W)], [("W", W)])
        self._stage_fresh_cpc(c)  # (cpc_objective="predictive": a fresh predictor behind W, from the same stream)
        self._stage_params(c, self._critic_flat, list(self.critic.named_parameters()), critic.named_parameters(),
                           fc=self.critic.encoder.fc)
        own = [(n, p) for n, p in self.actor.named_parameters() if ".convs." not in n]  # (the convs are the critic's)
        self._stage_params(a, self._actor_flat, own, actor.named_parameters(), fc=self.actor.encoder.fc)
        return stage

    def _upload_fresh(self, draw=True):
        """``_stage_fresh()`` and its two host-to-device copies, enqueued on the current stream (the events let the
        next staging wait for them); returns the staging buffers.  ``draw=False`` (measurements: the device's share
        without the host's draw) sends the values staged last again and leaves the reset stream where it is."""
        stage = self._stage_fresh() if draw else self._reset_staging()
        for st in stage.values():
            st["dev"].copy_(st["host"], non_blocking=True)
            if st["dev"].is_cuda:
                if st["event"] is None:
                    st["event"] = torch.cuda.Event()
                st["event"].record()
        return stage

    # ------------------------------------------------------------------ the reset
    @torch.no_grad()
    def reset_networks(self, encoder_keep=None, alpha=True):
        """Re-initialise the networks in place (Nikishin et al. 2022; D'Oro et al. 2023).
          heads   : actor.trunk, critic.Q1 / Q2 and the target's Q functions become freshly initialised ones (the
                    target's equal the critic's)
          encoder : the critic encoder (the actor's tied convs with it), the target encoder -- same fresh values --, the
                    actor encoder's fc / ln -- their own -- and CURL.W (CURL.predictor with it: DESIGN.md 7n) become
                    ``keep * old + (1 - keep) * fresh`` with keep = ``encoder_keep`` (None: the attribute
                    ``reset_encoder_keep``); 1 leaves them untouched
          state   : the four network optimizers start over -- moments zero, every step count 0; whole optimizers, also
                    where the encoder is kept: their fused launches have one step count each --, the gradient buffers
                    are zero; ``alpha=True``: log_alpha is the constructor's log(init_temperature) again and its
                    optimizer starts over too
        The fresh values come from the agent's reset stream (``reset_seed``), not from torch's or NumPy's global streams,
        which a reset leaves bit for bit where they were.  Nothing is re-allocated: captured update graphs stay valid.
        A prioritized replay buffer keeps its priorities; they re-form from the next TD errors."""
        keep = _check_reset_keep(self.reset_encoder_keep if encoder_keep is None else encoder_keep)
        if self.device.type != "cuda" and _lib._trace_hook is None:
            raise RuntimeError("CurlSacAgent.reset_networks needs a CUDA/HIP device: the learner path has no CPU fallback")
        self._finish_actor_step()
        stage = self._upload_fresh()
        lay = self._lay
        (w0, w1), (e0, e1), (_, q1) = lay["w"], lay["enc"], lay["q"]
        cf, tf, sc = self._critic_flat, self._target_flat, stage["critic"]["dev"]
        af, sa = self._actor_flat, stage["actor"]["dev"]
        trunk0 = (self.actor.trunk[0].weight.data_ptr() - af.data_ptr()) // 4
        # critic flat [ W | encoder | Q1 | Q2 ]: the target has no W, so W takes a launch of its own
        ops.shrink_perturb2(cf[w0:w1], None, sc[w0:w1], w1 - w0, keep, keep)
        ops.shrink_perturb2(cf[e0:q1], tf[e0:q1], sc[e0:q1], e1 - e0, keep, 0.0)
        ops.shrink_perturb2(af, None, sa, trunk0, keep, 0.0)  # actor flat [ fc, ln | trunk ]

        for opt in (self.actor_optimizer, self.critic_optimizer, self.encoder_optimizer, self.cpc_optimizer):
            if isinstance(opt, FlatAdam):
                opt.reset_state()
            else:
                _zero_torch_adam(opt)
        self._critic_gflat.zero_()
        self._actor_gbucket.zero_()
        self.log_alpha.grad.zero_()
        if alpha:
            self.log_alpha.fill_(self._init_log_alpha)
            _zero_torch_adam(self.log_alpha_optimizer)
        self._drop_encoder_caches()
        self.reset_count += 1

    def _maybe_reset(self, step):
        """The schedule, at the top of ``update()``: at most one reset per epoch of ``reset_interval`` steps, none in
        epoch 0."""
        if self.reset_interval == 0 and type(self.reset_interval) is int:
            return
        interval = _check_reset_interval(self.reset_interval)  # (the attribute may have been edited)
        if interval > 0 and step // interval > self._reset_epoch:
            self.reset_networks()
            self._reset_epoch = step // interval

    # ------------------------------------------------------------------ checkpoints
    def _reset_checkpoint(self):
        return {"reset_rng": self._reset_stream().clone(), "reset_epoch": int(self._reset_epoch),
                "reset_count": int(self.reset_count), "reset_interval": int(self.reset_interval),
                "reset_encoder_keep": float(self.reset_encoder_keep), "reset_seed": int(self.reset_seed)}

    def _load_reset_checkpoint(self, ck):
        """The stream, the epoch and the count come from the file; the settings stay the agent's own.  A file from
        before the keywords: the epoch of its step, so that the first update does not catch up on a reset."""
        if "reset_rng" in ck:
            self._reset_rng = ck["reset_rng"].clone()
            self._reset_epoch = int(ck["reset_epoch"])
            self.reset_count = int(ck["reset_count"])
        else:
            interval = _check_reset_interval(self.reset_interval)
            self._reset_epoch = int(ck["step"]) // interval if interval > 0 else 0
