"""CurlSacAgent's representation objective: what depends on the head of the cpc phase -- CURL's bilinear InfoNCE (the
reference's, the default) or the self-predictive latent loss (``cpc_objective="predictive"``)."""
import numpy as np
import torch
import torch.nn as nn

from . import ops
from .networks import weight_init

OBJECTIVES = ("infonce", "predictive")


def _check_cpc_objective(v):
    """The representation objective: one of the two strings."""
    if not isinstance(v, str) or v not in OBJECTIVES:
        raise ValueError("cpc_objective: %r is not one of %s" % (v, " / ".join(repr(o) for o in OBJECTIVES)))
    return v


def _check_predictor_hidden(v):
    """The predictor's hidden width: None (the agent's hidden_dim) or an ``int >= 1`` (a bool, a float or a string is
    not one)."""
    if v is None:
        return None
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
        raise ValueError("predictor_hidden: %r is not a positive int (or None: hidden_dim)" % (v,))
    return int(v)


def _cpc_keywords(agent, cpc_objective, predictor_hidden):
    """The class call's objective keywords, checked, onto the agent under construction (``"infonce"``: the instance is
    the one without the keyword, down to its __dict__)."""
    hidden = _check_predictor_hidden(predictor_hidden)
    if _check_cpc_objective(cpc_objective) == "predictive":
        agent.cpc_objective = "predictive"
        agent.predictor_hidden = hidden  # (None until __init__ knows hidden_dim: _build_predictor)
    elif hidden is not None:
        raise ValueError("predictor_hidden needs cpc_objective='predictive'")


class _CpcMixin:
    """CurlSacAgent's objective-dependent methods; the settings come from the class call (_cpc_keywords)."""

    cpc_objective = "infonce"
    predictor_hidden = None

    @property
    def _predictive(self):
        return self.cpc_objective == "predictive"

    # ------------------------------------------------------------------ construction
    def _check_cpc_init(self, pixel_sac):
        """At the top of ``__init__``, before a network is built."""
        if self._predictive and pixel_sac:
            raise ValueError("cpc_objective='predictive' is not combined with pixel_sac=True: pixel SAC has no "
                             "representation phase for the objective to run in")

    def _new_predictor(self, feature_dim):
        """predictor([z, a]) -> the target encoder's latent of the next observation, initialised like every other
        Linear; its draws come from torch's generator where it stands."""
        net = nn.Sequential(nn.Linear(feature_dim + self.action_dim, self.predictor_hidden), nn.ReLU(),
                            nn.Linear(self.predictor_hidden, feature_dim))
        net.apply(weight_init)
        return net

    def _build_predictor(self, feature_dim):
        """Behind everything the reference constructs (CURL.W is the last): a seeded agent's networks are the default
        agent's.  A submodule of CURL, so its state dict carries it."""
        if self._predictive:
            if self.predictor_hidden is None:
                self.predictor_hidden = int(self.hidden_dim)
            self.CURL.predictor = self._new_predictor(feature_dim)

    def _cpc_flat_params(self):
        """What joins CURL.W in the flat layout's W group, in order: [(name, Parameter)] (none by default)."""
        if not self._predictive:
            return []
        return [("predictor." + n, p) for n, p in self.CURL.predictor.named_parameters()]

    def _cpc_head_params(self):
        """The head's parameters cpc_optimizer steps in front of the encoder's.  Predictive: the predictor's -- CURL.W
        keeps its slot and a zero gradient and belongs to no optimizer, so it is never stepped, nor decayed."""
        return [p for _, p in self._cpc_flat_params()] if self._predictive else [self.CURL.W]

    def _cpc_workspace(self, ws, f, B, F, A):
        """The predictive head's buffers of one batch size (none by default), onto the workspace: [z | a], the hidden
        layer, the prediction and the gradients of the latter two."""
        if self._predictive:
            H = self.predictor_hidden
            ws.p_xa, ws.p_h, ws.p_out, ws.p_dh, ws.p_dout = f(B, F + A), f(B, H), f(B, F), f(B, H), f(B, F)

    # ------------------------------------------------------------------ update(): checks, the head's launches
    def _check_cpc_buffer(self, replay_buffer):
        """The positive of the predictive objective is the observation one step after obs[t], the step action[t]
        caused: the buffer must say so (``pos_offset == 1``; an n-step buffer's stored row still has its own next_obs
        there).  A buffer without the attribute delivers an augmentation of obs[t] itself."""
        if self._predictive and getattr(replay_buffer, "pos_offset", None) != 1:
            raise ValueError("cpc_objective='predictive' needs a replay buffer with pos_offset = 1 (the positive is the "
                             "observation one step after obs[t], the step action[t] caused); this one has pos_offset = %r"
                             % (getattr(replay_buffer, "pos_offset", None),))

    def _cpc_call_kw(self, action):
        """What ``_phases`` hands update_cpc behind the reference's five arguments."""
        return dict(action=action) if self._predictive else {}

    def _check_cpc_action(self, action, B):
        """At the top of update_cpc, before anything is written."""
        if not self._predictive:
            return None
        if action is None:
            raise ValueError("update_cpc: cpc_objective='predictive' needs action= (the minibatch's actions, [B, A])")
        if tuple(action.shape) != (B, self.action_dim):
            raise ValueError("update_cpc: action has shape %r, not (%d, %d)" % (tuple(action.shape), B, self.action_dim))
        return action.contiguous()

    def _predictive_head(self, ws, obs_ref, action, logged):
        """Behind ws.z_c / ws.z_pos: p = predictor([z_c | action]), the loss against z_pos and its gradient in one
        kernel, the predictor's backward into its .grad views and d(loss)/d(z_c) into ws.dz, the encoder's backward
        as the unfused CURL route calls it.  No host synchronisation: capturable."""
        B, F, A, H = obs_ref.B, self.critic.encoder.feature_dim, self.action_dim, self.predictor_hidden
        l1, l2 = self.CURL.predictor[0], self.CURL.predictor[2]
        ops.concat(ws.z_c, action, B, F, A, ws.p_xa)
        ops.linear_fwd(ws.p_xa, 0, l1.weight, 0, l1.bias, 0, ws.p_h, 0, B, H, F + A, relu=1)
        ops.linear_fwd(ws.p_h, 0, l2.weight, 0, l2.bias, 0, ws.p_out, 0, B, F, H)
        ops.pred_loss(ws.p_out, ws.z_pos, B, F, ws.row_loss, ws.scalars[5:6] if logged else None, ws.p_dout)
        ops.linear_dw(ws.p_dout, 0, ws.p_h, 0, l2.weight.grad, 0, B, F, H)
        ops.colsum(ws.p_dout, B, F, F, 0, l2.bias.grad, 0)
        ops.linear_dx(ws.p_dout, 0, l2.weight, 0, ws.p_dh, 0, B, F, H, mask=ws.p_h)  # (the ReLU's mask)
        ops.linear_dw(ws.p_dh, 0, ws.p_xa, 0, l1.weight.grad, 0, B, H, F + A)
        ops.colsum(ws.p_dh, B, H, H, 0, l1.bias.grad, 0)
        # d(loss)/d(z_c): the first F columns of the first layer's input gradient, W's rows read by their leading
        # dimension; the action's columns are not formed
        ops.linear_dx(ws.p_dh, 0, l1.weight, 0, ws.dz, 0, B, H, F, ldw=F + A)
        self._encoder_backward_reduced(ws, obs_ref, ws.dz, 0, self._lay["enc"][1])

    def _cpc_loss_key(self):
        return 'train/pred_loss' if self._predictive else 'train/curl_loss'

    # ------------------------------------------------------------------ resets
    def _stage_fresh_cpc(self, host):
        """reset_networks(): a fresh predictor, drawn from the reset stream behind the fresh (Actor, Critic, W), into the
        critic staging buffer where the live one lies -- the shrink-and-perturb launch over the W group then treats it as
        it treats CURL.W."""
        if not self._predictive:
            return
        with torch.random.fork_rng(devices=[]):
            torch.set_rng_state(self._reset_stream())
            fresh = self._new_predictor(self.critic.encoder.feature_dim)
            self._reset_rng = torch.get_rng_state()
        self._stage_params(host, self._critic_flat, self._cpc_flat_params(),
                           [("predictor." + n, p) for n, p in fresh.named_parameters()])

    # ------------------------------------------------------------------ graphs, checkpoints
    def _cpc_graph_key(self):
        """The objective's part of _graph_key: none for InfoNCE -- the key of an agent without the keyword."""
        return (("cpc", "predictive", int(self.predictor_hidden)),) if self._predictive else ()

    def _cpc_checkpoint(self):
        if not self._predictive:  # (the file of an agent without the keyword)
            return {}
        return {"cpc_objective": "predictive", "predictor_hidden": int(self.predictor_hidden)}

    def _check_cpc_checkpoint(self, ck):
        """At the top of load_checkpoint, before anything is written: the file's objective is the agent's."""
        theirs = ck.get("cpc_objective", "infonce")
        if theirs != self.cpc_objective:
            raise ValueError("the checkpoint was written with cpc_objective = %r; this agent has cpc_objective = %r: the "
                             "two heads have different parameters and optimizer state" % (theirs, self.cpc_objective))
        if self._predictive and int(ck.get("predictor_hidden", self.predictor_hidden)) != self.predictor_hidden:
            raise ValueError("the checkpoint was written with predictor_hidden = %r; this agent has predictor_hidden = %r"
                             % (ck.get("predictor_hidden"), self.predictor_hidden))

    def _check_curl_state_dict(self, sd):
        """``load()``'s CURL file against the agent's objective, before anything is written."""
        theirs = any(k.startswith("predictor.") for k in sd)
        if theirs != self._predictive:
            raise ValueError("the CURL state dict %s a predictor; this agent has cpc_objective = %r"
                             % ("holds" if theirs else "holds no", self.cpc_objective))
