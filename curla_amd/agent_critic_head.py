"""CurlSacAgent's critic head: what depends on a Q function's last layer -- the reference's one Q value, truncated
quantile atoms (``critic_quantiles``) or the logits of an HL-Gauss histogram (``critic_bins``, 7l)."""
import numpy as np
import torch

from . import ops
from .networks import _check_bin_sigma, _check_bins, _check_drop_quantiles, _check_quantiles, _check_value_range


def _critic_head_keywords(agent, critic_quantiles, critic_drop_quantiles, critic_bins, critic_value_range,
                          critic_bin_sigma):
    """The class call's critic-head keywords, checked, onto the agent under construction (``critic_bins=0``: the
    instance is the one without the keyword, down to its __dict__)."""
    agent.critic_quantiles = _check_quantiles(critic_quantiles)
    agent.critic_drop_quantiles = _check_drop_quantiles(critic_drop_quantiles, agent.critic_quantiles)
    bin_sigma = _check_bin_sigma(critic_bin_sigma)
    if _check_bins(critic_bins):
        if critic_value_range is None:
            raise ValueError("critic_bins = %d needs critic_value_range=(v_min, v_max), the range of the returns the "
                             "bins cover" % critic_bins)
        agent.critic_bins = int(critic_bins)
        agent.critic_value_range = _check_value_range(critic_value_range)
        agent.critic_bin_sigma = bin_sigma
    elif critic_value_range is not None:
        raise ValueError("critic_value_range needs critic_bins > 0")


class _CriticHeadMixin:
    """CurlSacAgent's critic-head methods; the settings come from the class call (_critic_head_keywords)."""

    critic_quantiles = 0
    critic_drop_quantiles = 0
    critic_bins = 0
    critic_value_range = None
    critic_bin_sigma = 0.75
    _hlg_last_B = None  # critic_bins: the batch size of the last critic phase (target_clip_fraction's workspace)

    def _critic_width_kw(self):
        """The keywords that widen the Q functions' last layers, for every place that builds a Critic."""
        if self.critic_bins:
            return dict(bins=self.critic_bins, value_range=self.critic_value_range)
        return dict(quantiles=self.critic_quantiles) if self.critic_quantiles else {}

    def _has_row_loss(self):
        """Whether the loss kernels leave a value per row (the workspace's q_row_loss): the quantile loss
        (ops.tqc_critic_loss); the cross-entropies (ops.hlg_critic_loss) in the critic phase and min(Q1, Q2)
        (ops.hlg_actor_loss) in the actor phase."""
        return bool(self.critic_quantiles or self.critic_bins)

    def _hlg_params(self):
        """(v_min, v_max, sigma) of the HL-Gauss critic as they stand now -- the range and the smoothing may have been
        edited --, checked; the critics' own ``value_range`` (bin_centres, expected) follows the agent's."""
        v_min, v_max = rng = _check_value_range(self.critic_value_range)
        self.critic.value_range = self.critic_target.value_range = rng
        return v_min, v_max, _check_bin_sigma(self.critic_bin_sigma) * (v_max - v_min) / self.critic_bins

    def target_clip_fraction(self):
        """The share of the last critic phase's TD targets that the clamp moved onto ``v_min`` or ``v_max``: near 0 with
        a value range that fits, towards 1 with one the returns have left -- the HL-Gauss critic's own failure mode.  A
        host read of the workspace (it waits for the device); not part of ``update()``."""
        if not self.critic_bins:
            raise RuntimeError("target_clip_fraction: this agent has no categorical critic (critic_bins=M)")
        ws = self._workspaces.get(self._hlg_last_B)
        if ws is None:
            raise RuntimeError("target_clip_fraction: no critic phase has run yet")
        v_min, v_max = (np.float32(v) for v in _check_value_range(self.critic_value_range))
        t = ws.target_q.detach().reshape(-1).cpu().numpy()
        return float(((t == v_min) | (t == v_max)).mean())

    def _critic_loss_settings(self, per):
        """(dropped atoms, (v_min, v_max, sigma) or None): the loss settings as they stand now -- they may have been
        edited --, checked at the top of update_critic, before anything is written; and the one place that refuses
        ``per``, a prioritized minibatch, where the loss has no scalar TD error per Q function or row."""
        drop_q, hlg = 0, None
        if self.critic_quantiles:
            drop_q = _check_drop_quantiles(self.critic_drop_quantiles, self.critic.out_dim)
            if per is not None:
                raise ValueError("critic_quantiles: a prioritized minibatch is not supported (its priorities are built "
                                 "on one scalar TD error per Q function): use ReplayBuffer(prioritized=False)")
        if self.critic_bins:
            hlg = self._hlg_params()
            if per is not None:
                raise ValueError("critic_bins: a prioritized minibatch is not supported (its priorities are built on one "
                                 "scalar TD error per Q function): use ReplayBuffer(prioritized=False)")
        if self.aug_views == 2 and per is not None:
            raise ValueError("aug_views = 2: a prioritized minibatch is not supported (its rows are drawn per "
                             "position): use ReplayBuffer(prioritized=False)")
        return drop_q, hlg

    def _note_critic_batch(self, B):
        if self.critic_bins:
            self._hlg_last_B = B

    # -- the loss descriptors of _twin_bwd: (fields, launch) -- ``fields`` for the form computed inside the backward
    #    launch of the Q functions' last layer, ``launch()`` the loss kernel on its own where that form does not apply
    def _critic_loss(self, ws, reward, not_done, per, settings):
        """target_Q = r + not_done * gamma * (min Q' - alpha log pi'), the two MSE terms and their gradient dq
        (curl_sac.py:353-361).  ``critic_quantiles``: the quantile Huber loss of the critic's atoms against
        the kept target atoms, always a launch of its own.  ``aug_views = 2``: both views' estimates against
        the mean of the two views' targets, a launch of its own as well.  ``critic_bins``: the two
        cross-entropies of the critic's logits against the Gaussian histogram of the clamped TD target, with or without
        views, always a launch of its own.  ``settings``: _critic_loss_settings', which has refused ``per`` for the three.
        ``per``, a prioritized minibatch: the loss is launched here, the importance weights scale dq and the loss in
        place and the drawn rows get their new priorities -- all on the device --, and the backward runs on the weighted
        dq it finds: no descriptor, None."""
        B, Mq = ws.log_pi.shape[0], self.critic.out_dim
        la, gamma, total = self.log_alpha, self.discount, ws.scalars[0:1]
        drop_q, hlg = settings
        if self.critic_quantiles:
            return None, lambda: ops.tqc_critic_loss(ws.q, B * Mq, ws.tq, B * Mq, ws.log_pi, reward, not_done, la, gamma,
                                                     B, Mq, drop_q, ws.dq, B * Mq, ws.q_row_loss, total)
        if self.critic_bins:
            v_min, v_max, sigma = hlg
            return None, lambda: ops.hlg_critic_loss(ws.q, B * Mq, ws.tq, B * Mq, ws.log_pi, reward, not_done, la, gamma, B,
                                                     Mq, v_min, v_max, sigma, ws.dq, B * Mq, ws.target_q, ws.q_row_loss,
                                                     total, views=self.aug_views == 2)
        if self.aug_views == 2:
            return None, lambda: ops.critic_td_loss_views(ws.q, ws.tq, B, ws.log_pi, reward, not_done, la, gamma, B,
                                                          ws.target_q, total, ws.dq)
        def launch():
            ops.critic_td_loss(ws.q, ws.tq, B, ws.log_pi, reward, not_done, la, gamma, B, ws.target_q, total, ws.dq)
        if per is None:
            return dict(kind=1, twin_stride=B, q=ws.q, target_q_twin=ws.tq, log_pi=ws.log_pi, reward=reward,
                        not_done=not_done, log_alpha=la, discount=gamma, target_q=ws.target_q, scalars=total,
                        dq=ws.dq), launch
        if ws.per_w is None:
            ws.per_w, ws.per_value = (torch.empty(B, device=ws.dq.device, dtype=torch.float32) for _ in range(2))
        launch()
        per.td_update(ws.q, B, ws.target_q, ws.dq, total, ws.per_w, ws.per_value)
        return None

    def _actor_loss(self, ws):
        """The actor / alpha losses and d(loss)/dQ (curl_sac.py:377-401); ``critic_quantiles``: over the mean of all
        atoms in place of min(Q1, Q2), a launch of its own; ``critic_bins``: min(Q1, Q2) through the softmax, likewise."""
        B, A, Mq = ws.log_pi.shape[0], self.action_dim, self.critic.out_dim
        la, te, out, dla = self.log_alpha, float(self.target_entropy), ws.scalars[1:5], self._dlog_alpha()
        if self.critic_quantiles:
            return None, lambda: ops.tqc_actor_loss(ws.q, B * Mq, ws.log_pi, ws.log_std, A, la, te, B, Mq, out, ws.dq,
                                                    B * Mq, dla)
        if self.critic_bins:
            v_min, v_max, _ = self._hlg_params()
            return None, lambda: ops.hlg_actor_loss(ws.q, B * Mq, ws.log_pi, ws.log_std, A, la, te, B, Mq, v_min, v_max,
                                                    ws.q_row_loss, out, ws.dq, B * Mq, dla)
        return (dict(kind=2, A=A, twin_stride=B, q=ws.q, log_pi=ws.log_pi, log_std=ws.log_std, log_alpha=la,
                     target_entropy=te, scalars=out, dq=ws.dq, dlog_alpha=dla),
                lambda: ops.actor_loss(ws.q, B, ws.log_pi, ws.log_std, A, la, te, B, out, ws.dq, dla))

    # ------------------------------------------------------------------ graphs, checkpoints
    def _critic_head_graph_key(self):
        """The critic head's part of _graph_key: the quantiles' entry or the bins' (never both), none for the scalar
        head -- the key of an agent without the keywords."""
        if self.critic_quantiles:
            return (("quantiles", self.critic_quantiles, self.critic_drop_quantiles),)
        if self.critic_bins:
            return (("bins", self.critic_bins) + tuple(float(v) for v in self.critic_value_range) +
                    (float(self.critic_bin_sigma),),)
        return ()

    def _critic_head_checkpoint(self):
        ck = {"critic_quantiles": int(self.critic_quantiles), "critic_drop_quantiles": int(self.critic_drop_quantiles)}
        if self.critic_bins:  # (0: the file of an agent without the keyword)
            ck.update(critic_bins=int(self.critic_bins), critic_value_range=tuple(float(v) for v in self.critic_value_range),
                      critic_bin_sigma=float(self.critic_bin_sigma))
        return ck

    def _load_critic_head_checkpoint(self, ck):
        """(Another ``critic_quantiles`` or ``critic_bins`` has failed before, on the last layers' shapes.)  The dropped
        atoms, the range and the smoothing are numbers of the loss alone and come from the file."""
        if self.critic_quantiles and "critic_drop_quantiles" in ck:
            self.critic_drop_quantiles = _check_drop_quantiles(ck["critic_drop_quantiles"], self.critic_quantiles)
        if self.critic_bins and "critic_value_range" in ck:
            self.critic_value_range = _check_value_range(ck["critic_value_range"])
            self.critic_bin_sigma = _check_bin_sigma(ck.get("critic_bin_sigma", self.critic_bin_sigma))
            self._hlg_params()
