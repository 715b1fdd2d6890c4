"""CurlSacAgent's five optimizers: their construction, each phase's step, clipping by the global gradient norm,
decoupled weight decay, the target soft update and the checkpoint layout of their state."""
import os

import torch

from . import ops
from .optim import FlatAdam, check_max_grad_norm, check_weight_decay


class _OptimMixin:
    """CurlSacAgent's optimizer methods; the hints the step methods read (``_soft_update_hint``, ``_defer_actor_step``,
    ...) are the agent's hand-over attributes."""

    def _build_optimizers(self, actor_lr, actor_beta, critic_lr, critic_beta, alpha_lr, alpha_beta, encoder_lr):
        """Optimizers (curl_sac.py:299-313).  The reference hands Adam the tied convs (actor) and the target
        encoder (cpc) as well; their .grad is always None at step time there, so Adam never touches them.
        FlatAdam is torch.optim.Adam with its step() as one HIP launch over the flat buffer (optim.py);
        CURLA_TORCH_ADAM=1 keeps torch's own fused multi-tensor step (same state_dict either way)."""
        actor_own = [p for n, p in self.actor.named_parameters() if ".convs." not in n]
        enc_params = list(self.critic.encoder.parameters())
        if self.device.type == "cuda" and os.environ.get("CURLA_TORCH_ADAM", "0") == "1":
            def adam(params, flat, gflat, **kw):
                return torch.optim.Adam(params, fused=True, **kw)
        elif self.device.type == "cuda":
            def adam(params, flat, gflat, **kw):
                return FlatAdam(params, flat, gflat, **kw)
        else:
            def adam(params, flat, gflat, **kw):
                return torch.optim.Adam(params, **kw)
        cf, cg = self._critic_flat, self._critic_gflat
        self.actor_optimizer = adam(actor_own, self._actor_flat, self._actor_gflat, lr=actor_lr, betas=(actor_beta, 0.999))
        self.critic_optimizer = adam(list(self.critic.parameters()), cf, cg, lr=critic_lr, betas=(critic_beta, 0.999))
        # (beside a FlatAdam actor, log_alpha's step rides in the actor's launch: FlatAdam.step_with_scalar)
        flat_actor = isinstance(self.actor_optimizer, FlatAdam)
        self.log_alpha_optimizer = torch.optim.Adam(
            [self.log_alpha], lr=alpha_lr, betas=(alpha_beta, 0.999),
            **(dict(foreach=False) if flat_actor else dict(fused=True) if self.device.type == "cuda" else {}))
        self.encoder_optimizer = adam(enc_params, cf, cg, lr=encoder_lr)
        # (the head's parameters: CURL.W, or the predictor's with cpc_objective="predictive" -- agent_cpc.py)
        self.cpc_optimizer = adam(self._cpc_head_params() + enc_params, cf, cg, lr=encoder_lr)

    def _optimizers(self):
        return {"actor": self.actor_optimizer, "critic": self.critic_optimizer, "log_alpha": self.log_alpha_optimizer,
                "encoder": self.encoder_optimizer, "cpc": self.cpc_optimizer}

    # ------------------------------------------------------------------ the phases' steps
    def _critic_step(self):
        """critic_optimizer.step() (curl_sac.py:367) -- with the target soft update update() has announced right behind
        it (:442-445) in the same launch where the optimizer is the flat one: the update reads what the step writes, so
        both share one pass over the critic's flat parameters."""
        opt, hidden, fused = self.critic_optimizer, [], False
        if self.detach_encoder:  # convs received no gradient: Adam must skip them (grad None in the reference)
            hidden = [(p, p.grad) for m in self.critic.encoder.convs for p in (m.weight, m.bias)]
            for p, _ in hidden:
                p.grad = None
        elif self._soft_update_hint:
            (e0, e1), (_, q1) = self._lay["enc"], self._lay["q"]
            fused = self._soft_update_done = FlatAdam.step_with_lerp(opt, self._target_flat, e0, q1, e1 - e0,
                                                                     self.encoder_tau, self.critic_tau)
        if not fused:
            self._clip_torch(0, opt)
            opt.step()
        for p, g in hidden:
            p.grad = g

    def _actor_reduce_and_step(self, L, step):
        """The actor phase's reduction and optimizer steps.  Data parallel: ONE collective for the phase -- the bucket
        [fc, ln | trunk | words], log_alpha's float64 gradient riding in the words.  Overlapped schedule: the collective
        is asynchronous and, when update() has announced that the CURL phase follows, the two optimizer steps are taken
        only after that phase has been enqueued (_finish_actor_step): the CURL phase reads nothing they write (the
        actor's own fc / ln / trunk and log_alpha), so the numbers are the reference order's (curl_sac.py:393-404
        before :418-423) and the all-reduce runs underneath the CURL phase's convolutions."""
        overlap = self._dp_active and self._dp_overlap
        self._allreduce(self._actor_gbucket, async_op=overlap, f64_rider=(self.log_alpha.grad, self._la_words))
        self._actor_step_pending = bool(overlap and self._defer_actor_step and not self.log_param_hist_imgs)
        # (the norm is logged once the step that takes it has been enqueued: a deferred step is not, yet)
        self._actor_norm_log = (L, step) if self._max_grad_norm is not None and step % self.log_interval == 0 else None
        if not self._actor_step_pending:
            if overlap:
                self._allreduce_wait()
            self._actor_steps()

    def _actor_steps(self):
        # actor_optimizer.step() ... log_alpha_optimizer.step() (curl_sac.py:393-404): nothing in between reads
        # log_alpha (the logged alpha is the loss kernel's), so the two steps share a launch
        # (clipping: the actor's own parameters; log_alpha has its own optimizer and loss scale and is not clipped)
        if isinstance(self.actor_optimizer, FlatAdam):
            FlatAdam.step_with_scalar(self.actor_optimizer, self.log_alpha_optimizer)
        else:
            self._clip_torch(1, self.actor_optimizer)
            self.actor_optimizer.step()
            self.log_alpha_optimizer.step()
        if self._actor_norm_log is not None:
            (L, step), self._actor_norm_log = self._actor_norm_log, None
            L.log('train_actor/grad_norm', self.grad_clip_stats[1, 0], step)

    def _finish_actor_step(self):
        if self._actor_step_pending:
            self._actor_step_pending = False
            self._allreduce_wait()
            self._actor_steps()

    def _cpc_steps(self):
        # encoder_optimizer.step() ... cpc_optimizer.step() (curl_sac.py:418-423)
        if isinstance(self.encoder_optimizer, FlatAdam):
            FlatAdam.step_pair(self.encoder_optimizer, self.cpc_optimizer)  # both steps in one pass over the encoder
        else:
            self._clip_torch(2, self.cpc_optimizer)  # [W | encoder], once: both steps consume the clipped gradient
            self.encoder_optimizer.step()
            self.cpc_optimizer.step()

    def soft_update_targets(self):
        """utils.soft_update_params x3 (curl_sac.py:442-445) as one flat lerp with two rates."""
        lay = self._lay
        (e0, e1), (q0, q1) = lay["enc"], lay["q"]
        assert e1 == q0  # [encoder | Q1 | Q2] are adjacent: one launch, two rates
        ops.soft_update2(self._critic_flat[e0:q1], self._target_flat[e0:q1], e1 - e0, self.encoder_tau, self.critic_tau)

    # ---------------------------------------------------------------- clipping by the global gradient norm
    _max_grad_norm = None
    grad_clip_stats = None

    @property
    def max_grad_norm(self):
        """The threshold set by ``set_max_grad_norm`` (None: no clipping)."""
        return self._max_grad_norm

    def set_max_grad_norm(self, value):
        """Clip every phase's gradient by its global norm right in front of the phase's optimizer steps:
        ``torch.nn.utils.clip_grad_norm_(parameters with a gradient, value)`` where one would put it in the reference
        -- in front of curl_sac.py:367 over ``critic.parameters()`` (without the convs under ``detach_encoder``), in
        front of :393-404 over the actor's own parameters (``log_alpha`` is not clipped), in front of :418-423 over
        [CURL.W | encoder], once for both optimizers; data parallel: after the gradient's all-reduce.  ``value``: None
        (off, the default: the launches are the unclipped ones) or a positive number shared by the three phases.
        With the flat optimizers the norm never leaves the device: one square-sum launch per phase, the coefficient
        applied inside the Adam launch (optim.py).  ``grad_clip_stats`` (float32 device tensor [3, 2]; rows critic /
        actor / cpc, columns norm before clipping / coefficient applied) holds each phase's last figures.
        A hyper-parameter, not state: checkpoints do not carry it, a resumed run calls this again."""
        value = check_max_grad_norm(value)
        if value is not None and self.grad_clip_stats is None:
            self.grad_clip_stats = torch.zeros(3, 2, device=self.device, dtype=torch.float32)
        rows = ((self.critic_optimizer, 0), (self.actor_optimizer, 1), (self.encoder_optimizer, 2), (self.cpc_optimizer, 2))
        for opt, row in rows:
            if isinstance(opt, FlatAdam):
                if value is not None:
                    opt.clip_stats = self.grad_clip_stats[row]
                opt.max_grad_norm = value
        self._max_grad_norm = value  # (captured update graphs hold it by value: _graph_key)

    def _clip_torch(self, row, opt):
        """The clipping step of a phase whose optimizer is torch's own (CURLA_TORCH_ADAM=1, a CPU agent): FlatAdam
        clips inside its launches."""
        if self._max_grad_norm is None or isinstance(opt, FlatAdam):
            return
        params = [p for g in opt.param_groups for p in g["params"] if p.grad is not None]
        norm = torch.nn.utils.clip_grad_norm_(params, self._max_grad_norm)
        self.grad_clip_stats[row, 0] = norm
        self.grad_clip_stats[row, 1] = torch.clamp(self._max_grad_norm / (norm + 1e-6), max=1.0)

    # ---------------------------------------------------------------- decoupled weight decay (AdamW)
    @property
    def weight_decay(self):
        """The decoupled weight decay of the network optimizers, read from the critic optimizer's param group (the four
        carry the same value unless their groups were edited one by one); set by ``set_weight_decay``."""
        return float(self.critic_optimizer.param_groups[0].get("weight_decay", 0))

    def set_weight_decay(self, value):
        """Decoupled weight decay on the four network optimizers: actor, critic, encoder and cpc become what
        ``torch.optim.AdamW(..., weight_decay=value)`` is in the reference's place (curl_sac.py:299-313) -- every step
        multiplies the parameters it steps by ``1 - lr * value`` in front of the Adam update.  log_alpha's optimizer
        stays plain Adam.  The encoder is decayed by each optimizer that steps it (critic, encoder and cpc), as it would
        be there; parameters without a gradient at step time (the convs under ``detach_encoder`` in the critic's step)
        are not, as torch skips them.  ``value``: a finite number >= 0; 0 switches it off (the launches are the plain
        ones again).  Written into the optimizers' param groups (``weight_decay``, ``decoupled_weight_decay = value !=
        0``) as torch keeps them: it is part of their ``state_dict()`` and a checkpoint restores it.  With the flat
        optimizers the multiply is inside the Adam launches (``curla_adamw_*``, optim.py): an update launches as many
        optimizer kernels as without it."""
        value = check_weight_decay(value)
        for opt in (self.critic_optimizer, self.actor_optimizer, self.encoder_optimizer, self.cpc_optimizer):
            for g in opt.param_groups:
                g["weight_decay"] = value
                g["decoupled_weight_decay"] = value != 0

    # ---------------------------------------------------------------- checkpoints
    def _convert_opt_state(self, opt, sd, to_reference):
        """Adam moments of an encoder fc.weight follow the weight's column order: (c,y,x) on disk like the
        reference's Parameter, (y,x,c) in HBM."""
        fc_of = {id(e.fc.weight): e.fc for e in (self.actor.encoder, self.critic.encoder, self.critic_target.encoder)}
        params = [q for g in opt.param_groups for q in g["params"]]
        state = {}
        for i, st in sd["state"].items():
            st = dict(st)
            fc = fc_of.get(id(params[i]))
            for k, v in st.items():
                if torch.is_tensor(v):
                    if fc is not None and v.dim() == 2:
                        v = (fc.to_reference_layout(v) if to_reference else fc.from_reference_layout(v)).contiguous()
                    st[k] = v.detach().cpu() if to_reference else v
            state[i] = st
        return {"state": state, "param_groups": sd["param_groups"]}
