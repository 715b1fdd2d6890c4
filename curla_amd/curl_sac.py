"""CURL + SAC learner on MI355X: Actor / QFunction / Critic / CURL /
CurlSacAgent with the reference's API (curl_sac.py:57-465).

Host code is Python on PyTorch-ROCm: parameters are ``nn.Parameter`` views into
flat HBM buffers, the five optimizers are ``torch.optim.Adam`` objects (four of
them ``FlatAdam``: the same optimizer with its step as one flat HIP launch) --
the reference's division of labour.  Everything between "minibatch indices" and
".grad is filled in" runs as hand-written HIP kernels through the C ABI
(include/curla_hip.h); there is no autograd graph and no PyTorch fallback.

Schedule of one ``update()`` (reference curl_sac.py:426-451), with the sharing
the reference's autograd cannot do:
  critic phase : conv(next_obs; theta) -> actor head;  conv(next_obs; xi) -> target Q;
                 conv(obs; theta) -> twin Q -> loss -> explicit backward -> Adam
  actor phase  : conv(obs; theta') ONCE, reused by actor.fc, critic.fc and (below) CURL;
                 only live gradients are computed (actor fc/ln/trunk, log_alpha)
  soft update  : two flat lerps (Q block with critic_tau, encoder block with encoder_tau)
  cpc phase    : anchor features reused from the actor phase on even steps;
                 conv(pos; xi') -> bilinear logits (MFMA) -> CE -> backward -> 2x Adam
=> 5 conv-stack forwards + 2 backwards per update instead of the reference's 7 + 2.
"""
import inspect
import os
import warnings

import numpy as np
import torch

from . import ops
from .agent_acting import _ActingMixin
from .agent_checkpoint import _CheckpointMixin
from .agent_cpc import _cpc_keywords, _CpcMixin
from .agent_critic_head import _critic_head_keywords, _CriticHeadMixin
from .agent_dp import _DataParallelMixin
from .agent_graphs import _NullLog, _UpdateGraphsMixin
from .agent_optim import _OptimMixin
from .agent_policy import _policy_keywords, _PolicyMixin
from .agent_redo import _redo_keywords, _RedoMixin
from .agent_reset import _reset_keywords, _ResetMixin
from .encoder import CNNEncoder
from .mlp import _Mlp, _mlp_bwd, _mlp_fwd
from .networks import (CURL, LOG_FREQ, Actor, Critic, _check_dropout, _check_int, _check_layer_norm_width,
                       _device_generator, _reserve_dropout_counter)
from .ops import ObsRef
from .optim import check_weight_decay

# the other names this module defined before its splits, from their homes (tests/test_module_layout_host.py)
from .agent_policy import _check_policy, _check_policy_std_schedule, _linear_schedule  # noqa: F401
from .agent_redo import _check_redo_interval, _check_redo_recycle, _check_redo_tau  # noqa: F401
from .agent_reset import _check_reset_interval, _check_reset_keep, _check_reset_seed  # noqa: F401
from .mlp import _MlpLn, _linears  # noqa: F401
from .networks import (QFunction, _check_bin_sigma, _check_bins, _check_drop_quantiles,  # noqa: F401
                       _check_policy_std, _check_policy_std_clip, _check_quantiles, _check_value_range, _CriticType,
                       _QFunctionType, _widen_last_layers, weight_init)
from .optim import FlatAdam, check_max_grad_norm  # noqa: F401


def _as_ref(obs):
    if isinstance(obs, ObsRef):
        return obs
    return ObsRef.from_tensor(obs.contiguous().float())


def _no_drop(tag):
    return None


def _check_views(v):
    """The augmented views per transition: the ``int`` 1 or 2 (a bool, a float or a string is not one)."""
    return _check_int(v, 1, 2, "aug_views: %r is not the int 1 or 2" % (v,))


def _check_utd_ratio(g):
    """The update-to-data ratio: an ``int >= 1`` (a bool, a float or a string is not one)."""
    return _check_int(g, 1, None, "utd_ratio: %r is not an int >= 1" % (g,))


class _Workspace:
    """Every per-update buffer for one batch size, allocated once (static
    addresses: the kernel sequence is hipGraph-capturable)."""

    def __init__(self, agent, B):
        enc = agent.critic.encoder
        dev = agent.device
        F, A, H, L = enc.feature_dim, agent.action_dim, agent.hidden_dim, enc.num_layers
        f = lambda *shape: torch.empty(shape, device=dev, dtype=torch.float32)  # noqa: E731
        shapes = [(B, h, w, enc.num_filters) for (h, w) in enc.layer_hw[1:]]
        # [obs | next_obs] activations of the critic phase's pass through the online convs (one launch per layer for
        # both); the obs half doubles as the activations kept for a backward pass
        self.acts_pair = [f(2 * s[0], *s[1:]) for s in shapes]
        self.acts_main = [a[:B] for a in self.acts_pair]
        self.acts_tmp = [f(*s) for s in shapes]   # no-grad passes
        gmax = max(int(np.prod(s)) for s in shapes)
        self.gbuf = [f(gmax), f(gmax)]
        self.gviews = [[g[:int(np.prod(s))].view(s) for s in shapes] for g in self.gbuf]
        # one slab workspace per conv layer: the layers' weight-gradient reductions run as ONE launch at the end of a
        # backward pass (ops.wgrad_reduce_multi)
        self.wg_ws = [f(ops.wgrad_workspace_floats(enc.obs_shape[0] if i == 0 else enc.num_filters)) for i in range(L)]
        # features
        self.z_a, self.z_t, self.z_c, self.z_pos = f(B, F), f(B, F), f(B, F), f(B, F)
        self.xhat_c, self.rstd_c, self.xhat_a, self.rstd_a = f(B, F), f(B), f(B, F), f(B)
        self.dz, self.dfc = f(B, F), f(B, F)
        self.ln_partial = f(ops.ln_partial_floats(B, F))  # LayerNorm parameter-gradient partial sums (ops.ln_bwd defer=)
        # CURL.W gradient partial sums (ops.curl_head: feature widths it is built for only)
        self.w_partial = f(max(1, B // 16) * F * F) if ops.curl_head_supported(B, F) else None
        self.fc_out = f(B, F)  # pre-LayerNorm features, only written on histogram-logging steps
        # actor trunk
        AO = agent._actor_out_dim()  # ([mu | raw log_std]; the deterministic policy: the A means alone)
        self.a_h1, self.a_h2, self.a_out = f(B, H), f(B, H), f(B, AO)
        self.a_dh1, self.a_dh2, self.a_dout = f(B, H), f(B, H), f(B, AO)
        self.noise = f(B, A)
        self.mu, self.pi, self.log_std, self.tanh_ls, self.gpi = f(B, A), f(B, A), f(B, A), f(B, A), f(B, A)
        self.log_pi = f(B, 1)
        # twin Q
        # [0] = the target critic's pass over next_obs, [1] = the critic's over obs: one launch per layer for the four
        # Q functions (update_critic); the names without a 2 are the critic's halves, what the backward reads
        M = agent.critic.out_dim  # (a wider critic head: M atoms or logits per Q function in place of the one Q value)
        self.xa2, self.q_h1_2, self.q_h2_2, self.q2 = f(2, B, F + A), f(2, 2, B, H), f(2, 2, B, H), f(2, 2, B, M)
        self.xa, self.q_h1, self.q_h2 = self.xa2[1], self.q_h1_2[1], self.q_h2_2[1]
        self.tq, self.q = self.q2[0], self.q2[1]
        self.dxa = f(2, B, F + A)
        self.q_dh1, self.q_dh2 = f(2, B, H), f(2, B, H)
        # critic_layer_norm: what the critic's LayerNorms save for their backward, per hidden layer (the critic and the
        # actor phase share them; the target critic's passes save nothing) and the workspace of their parameter
        # gradients' partial sums -- as Critic.twin_ln takes them
        self.q_ln_saves, self.q_ln_partial = (None, None), None
        if agent.critic_layer_norm:
            self.q_xhat1, self.q_xhat2, self.q_rstd1, self.q_rstd2 = f(2, B, H), f(2, B, H), f(2, B), f(2, B)
            self.q_ln_saves = ([self.q_xhat1, self.q_xhat2], [self.q_rstd1, self.q_rstd2])
            self.q_ln_partial = f(ops.mlp_ln_partial_floats(B, H, 2))
        self.dq, self.target_q = f(2, B, M), f(B, 1)
        self.q_row_loss = f(B) if agent._has_row_loss() else None  # the quantile and HL-Gauss losses' value per row
        self.per_w = self.per_value = None  # importance weights / new stored values [B]: a prioritized buffer's updates only
        # scalars: [0] critic loss, [1..4] actor_loss/alpha_loss/entropy/alpha, [5] curl loss, [6] batch reward
        self.scalars = torch.zeros(8, device=dev, dtype=torch.float32)
        # CURL
        self.WzT, self.dWzT = f(B, F), f(B, F)
        self.logits, self.dlogits, self.row_loss = f(B, B), f(B, B), f(B)
        agent._cpc_workspace(self, f, B, F, A)  # (the predictive objective's head; nothing by default)


class _AgentType(type):
    """``CurlSacAgent(...)`` takes the reference's arguments and, behind them, this package's own keywords.
    ``CurlSacAgent.__init__`` keeps the reference's parameter list name for name (curl_sac.py:226-256: the drop-in
    contract, tests/test_dropin_contract.py); a keyword that shapes the networks has to be known before ``__init__``
    builds them, so the class call takes it off the arguments and leaves it on the instance."""

    def __call__(cls, *args, cpc_objective="infonce", predictor_hidden=None, policy="gaussian", policy_std=0.2,
                 policy_std_clip=0.3, policy_std_schedule=None, aug_views=1, redo_interval=0, redo_tau=0.1, redo_recycle=True, reset_interval=0,
                 reset_encoder_keep=1.0, reset_seed=0, critic_quantiles=0, critic_drop_quantiles=0, critic_bins=0,
                 critic_value_range=None, critic_bin_sigma=0.75, weight_decay=0.0, utd_ratio=1, critic_dropout=0.0,
                 critic_layer_norm=False, **kwargs):
        agent = cls.__new__(cls)
        _cpc_keywords(agent, cpc_objective, predictor_hidden)
        _policy_keywords(agent, policy, policy_std, policy_std_clip, policy_std_schedule)
        _redo_keywords(agent, redo_interval, redo_tau, redo_recycle)
        _reset_keywords(agent, reset_interval, reset_encoder_keep, reset_seed)
        _critic_head_keywords(agent, critic_quantiles, critic_drop_quantiles, critic_bins, critic_value_range,
                              critic_bin_sigma)
        agent.critic_layer_norm = bool(critic_layer_norm)
        agent.critic_dropout = _check_dropout(critic_dropout, agent.critic_layer_norm)
        agent.utd_ratio = _check_utd_ratio(utd_ratio)
        if agent.critic_bins and agent.critic_quantiles:
            raise ValueError("critic_bins > 0 is not combined with critic_quantiles > 0: a Q function's last layer is "
                             "the logits of one categorical distribution or a set of quantile atoms")
        if _check_views(aug_views) == 2:  # (1: the instance is the one without the keyword, down to its __dict__)
            if agent.critic_quantiles:
                raise ValueError("aug_views = 2 is not combined with critic_quantiles > 0: the mean of two views' "
                                 "targets would have to be one of their pooled, truncated atom sets, which is out of scope")
            agent.aug_views = 2
        weight_decay = check_weight_decay(weight_decay)
        agent.__init__(*args, **kwargs)
        if weight_decay != 0:  # (0: the optimizers are built exactly as without the keyword)
            agent.set_weight_decay(weight_decay)
        return agent


class CurlSacAgent(_ActingMixin, _DataParallelMixin, _UpdateGraphsMixin, _ResetMixin, _RedoMixin, _CriticHeadMixin,
                   _CpcMixin, _PolicyMixin, _OptimMixin, _CheckpointMixin, metaclass=_AgentType):
    """CURL representation learning with SAC (curl_sac.py:224-465).
    ``CurlSacAgent(..., critic_layer_norm=True)`` (a keyword of the class call, not in the reference; default off:
    nothing changes): an ``nn.LayerNorm(hidden_dim)`` between each hidden Linear of the Q functions and its ReLU, critic
    and target critic alike -- the critic regulariser of DroQ / RLPD.  ``hidden_dim`` up to 1024 then.
    ``critic_dropout=p`` (with ``critic_layer_norm=True`` only; default 0: nothing changes): DroQ's dropout in front of
    each of those LayerNorms, in every critic pass of ``update()`` -- the target's, the critic's and the actor phase's.
    No module and no mask buffer: ``p`` is this attribute, the masks are a counter-based stream.
    ``utd_ratio=G`` (default 1: nothing changes): the update-to-data ratio of DroQ / RLPD -- one ``update()`` call makes
    G critic steps on G freshly drawn minibatches before the actor steps once (``update``).  An attribute
    that may be edited between calls.
    ``weight_decay=wd`` (default 0: nothing changes): decoupled weight decay -- the actor, critic, encoder and cpc
    optimizers are ``torch.optim.AdamW(..., weight_decay=wd)``, log_alpha's stays plain Adam (``set_weight_decay``;
    DESIGN.md 7g).
    ``critic_quantiles=M`` (default 0: nothing changes; 1 .. 32): truncated quantile critics -- each Q function outputs
    M quantile atoms, the two target networks' atoms are pooled and sorted, the ``critic_drop_quantiles=d`` largest per
    network dropped (0 <= d < M) and every online atom regressed on the kept ones with the quantile Huber loss; the
    actor ascends the mean of all atoms.  M shapes the networks; d is an attribute that may be edited
    between calls.  Not with a prioritized replay buffer.
    ``reset_interval=N`` (default 0: nothing changes): every N steps ``update()`` first calls ``reset_networks()`` -- the
    heads re-initialised, the encoder shrunk and perturbed with ``reset_encoder_keep`` (default 1.0: kept as it is), the
    optimizers started over --, the fresh values drawn from a stream of the agent's own seeded by ``reset_seed``
    (agent_reset.py).  The first two are attributes that may be edited between calls.
    ``redo_interval=N`` (default 0: nothing changes): every update whose step is a multiple of N ends with a redo pass
    (``redo_pass``) on its minibatch -- the dormant-neuron scores of the six hidden layers of Q1, Q2 and the actor trunk
    (``dormant_counts``, ``dormant_fractions``, ``dormant_report()``) and, unless ``redo_recycle=False``, ReDo's recycling
    of the units whose score is <= ``redo_tau`` (default 0.1) with fresh values from the reset stream (agent_redo.py;
    DESIGN.md 7j).  All three are attributes that may be edited between calls.
    ``aug_views=2`` (default 1: nothing changes; with a ``ReplayBuffer(aug_views=2)``, and ``update`` checks that the two
    agree): DrQ's K = 2, M = 2 -- a minibatch of B positions is B / 2 transitions, each under two independent
    augmentations at positions b and b + B / 2.  The critic phase regresses both views' Q estimates on the mean of the two
    views' TD targets, the CURL phase does not count a position's partner among its negatives; the actor phase sees all B
    positions.  Fixed at construction.  Not with ``critic_quantiles``.
    ``critic_bins=M`` (default 0: nothing changes; 2 .. 256) with ``critic_value_range=(v_min, v_max)`` (required then;
    finite, v_min < v_max) and ``critic_bin_sigma=s`` (default 0.75; finite, > 0): the categorical HL-Gauss critic -- each
    Q function outputs M logits over M equal bins of the value range, Q is the softmax's expectation of the bin centres,
    and the critic is trained by cross-entropy on the histogram of a Gaussian of standard deviation s bin widths around
    the clamped scalar TD target; the actor ascends min(Q1, Q2) through the softmax.  M shapes the
    networks; the range and s are attributes that may be edited between calls.  ``target_clip_fraction()`` tells whether
    the range fits.  With ``aug_views=2``; not with ``critic_quantiles``, not with a prioritized replay buffer.
    ``policy="deterministic"`` (default "gaussian": nothing changes) with ``policy_std=0.2`` (finite, > 0),
    ``policy_std_clip=0.3`` (finite, >= 0, or None: no clip) and ``policy_std_schedule=None`` (or ``(init, final,
    duration)``: DrQ-v2's linear schedule in ``update``'s ``step``): DrQ-v2's policy -- the actor outputs A pre-squash
    means, ``select_action`` returns tanh(mu), ``sample_action`` clamp(tanh(mu) + std * noise, -lim, lim), and the update
    phases clip the scaled noise to ``policy_std_clip`` before they add it (TD3's target smoothing); log_pi is 0, so the
    critic losses compute the entropy-free target, the actor loss is -mean Q, and log_alpha never moves.
    The policy shapes the actor; ``policy_std`` is read through ``agent.policy_std`` and set by ``set_policy_std`` (a
    device scalar: data to captured graphs), clip and schedule are attributes that may be edited between calls.  The
    three ``policy_std*`` keywords raise beside the Gaussian policy.
    ``cpc_objective="predictive"`` (default "infonce": nothing changes) with ``predictor_hidden=H`` (None: hidden_dim; a
    positive int): the self-predictive latent objective of SPR / BBF in one step -- the representation phase trains the
    encoder, and ``CURL.predictor`` = Linear(F + A, H) - ReLU - Linear(H, F), to predict from the online latent of obs[t]
    and action[t] the target encoder's latent of the next observation, by the squared distance of the two normalised
    vectors (``curla_pred_loss``; agent_cpc.py).  No negatives: per row, whatever the batch size.  With a
    ``ReplayBuffer(pos_offset=1)``, and ``update`` checks it; CURL.W keeps its slot and is never stepped; logged as
    ``train/pred_loss``.  Fixed at construction.  Not with ``pixel_sac``."""

    critic_layer_norm = False
    critic_dropout = 0.0
    utd_ratio = 1
    aug_views = 1

    def __init__(
        self,
        obs_shape,
        action_shape,
        device,
        augmentor,
        hidden_dim=256,
        discount=0.99,
        init_temperature=0.01,
        alpha_lr=1e-3,
        alpha_beta=0.9,
        actor_lr=1e-3,
        actor_beta=0.9,
        actor_log_std_min=-10,
        actor_log_std_max=2,
        actor_update_freq=2,
        critic_lr=1e-3,
        critic_beta=0.9,
        critic_tau=0.005,
        critic_target_update_freq=2,
        encoder_feature_dim=50,
        encoder_lr=1e-3,
        encoder_tau=0.005,
        num_layers=4,
        num_filters=32,
        cpc_update_freq=1,
        log_interval=100,
        log_param_hist_imgs=False,
        detach_encoder=False,
        pixel_sac=False
    ):
        _check_layer_norm_width(self.critic_layer_norm, hidden_dim)
        self._check_cpc_init(pixel_sac)
        self.augmentor = augmentor
        self.device = torch.device(device)
        if self.critic_dropout > 0 and self.device.type == "cuda" and \
                not hasattr(_device_generator(self.device), "get_offset"):
            raise RuntimeError("critic_dropout: this torch build's device generator exposes no Philox offset "
                               "(get_offset / set_offset), which the dropout masks' stream positions are taken from")
        self.discount = discount
        self.critic_tau = critic_tau
        self.encoder_tau = encoder_tau
        self.actor_update_freq = actor_update_freq
        self.critic_target_update_freq = critic_target_update_freq
        self.cpc_update_freq = cpc_update_freq
        self.log_interval = log_interval
        self.log_param_hist_imgs = log_param_hist_imgs
        self.image_shape = tuple(obs_shape[-2:])
        self._act_stage = {}
        self._act_batch_stage = {}  # (C, H, W) -> staging blocks and ring of select_actions / sample_actions
        self.detach_encoder = detach_encoder
        self.pixel_sac = pixel_sac
        self.action_dim = action_shape[0]
        self.hidden_dim = hidden_dim
        # what reset_networks() builds fresh networks from, and puts log_alpha back to
        self._net_args = (tuple(obs_shape), tuple(action_shape), hidden_dim, encoder_feature_dim, actor_log_std_min,
                          actor_log_std_max, num_layers, num_filters)
        self._init_log_alpha = float(np.log(init_temperature))

        # same construction order as the reference => same RNG stream => same init for a given seed
        self.actor = Actor(obs_shape, action_shape, hidden_dim, encoder_feature_dim, actor_log_std_min,
                           actor_log_std_max, num_layers, num_filters, **self._actor_kw())
        q_kw = self._critic_width_kw()
        self.critic = Critic(obs_shape, action_shape, hidden_dim, encoder_feature_dim, num_layers, num_filters,
                             layer_norm=self.critic_layer_norm, dropout=self.critic_dropout, **q_kw)
        self.critic_target = Critic(obs_shape, action_shape, hidden_dim, encoder_feature_dim, num_layers, num_filters,
                                    layer_norm=self.critic_layer_norm, dropout=self.critic_dropout, **q_kw)
        self.critic_target.load_state_dict(self.critic.state_dict())

        # tie encoders between actor and critic, and CURL and critic
        self.actor.encoder.copy_conv_weights_from(self.critic.encoder)

        self.log_alpha = torch.tensor(np.log(init_temperature)).to(self.device)  # float64, like the reference
        self.log_alpha.requires_grad = True
        self.target_entropy = -np.prod(action_shape)

        self.CURL = CURL(obs_shape, encoder_feature_dim, self.critic, self.critic_target, output_type='continuous')
        self._build_predictor(encoder_feature_dim)  # (cpc_objective="predictive": behind everything the reference draws)

        self._to_flat_device_layout()
        self._place_policy_scalars()
        self._build_optimizers(actor_lr, actor_beta, critic_lr, critic_beta, alpha_lr, alpha_beta, encoder_lr)
        self._install_grad_views()

        self._workspaces = {}
        self._dp_group = None
        self._dp_world = 1
        self._dp_active = False
        self._dp_avg = False
        self._dp_staged = False
        self._dp_overlap = False
        self._dp_check_every = 0
        self._dp_pending = []
        self._graphs = None      # captured update graphs: None (off) or {kind: state} (enable_update_graphs)
        self._graph_cap = None   # while a graph is being captured: the device addresses its kernels read their
        #                          per-update values from
        self.train()
        self.critic_target.train()

    # ------------------------------------------------------------------ layout
    def _to_flat_device_layout(self):
        """Move every parameter into flat fp32 device buffers (16-byte aligned
        slots), Q1/Q2 as two identically laid-out blocks, and give each a
        persistent .grad view into a mirror buffer.
          critic flat : [ CURL.W (+ CURL.predictor: cpc_objective="predictive") | encoder (convs, fc, ln) | Q1 | Q2 ]
          target flat : same layout (W group's slot unused)
          actor flat  : [ encoder.fc, encoder.ln | trunk ]"""
        dev = self.device
        for m in (self.actor, self.critic, self.critic_target):
            m.encoder.to_kernel_layout()

        def place(named, flat_size_only=False, flat=None, gflat=None, off0=0):
            off = off0
            for _, p in named:
                n = p.numel()
                if not flat_size_only:
                    dst = flat[off:off + n].view(p.shape)
                    dst.copy_(p.data)
                    p.data = dst
                    if gflat is not None:
                        p.grad = gflat[off:off + n].view(p.shape)
                off += (n + 3) & ~3
            return off

        def critic_groups(critic, W):
            enc = [("encoder." + n, p) for n, p in critic.encoder.named_parameters()]
            q1 = [("Q1." + n, p) for n, p in critic.Q1.named_parameters()]
            q2 = [("Q2." + n, p) for n, p in critic.Q2.named_parameters()]
            return [("W", W)] + self._cpc_flat_params() if W is not None else [], enc, q1, q2

        wl, enc, q1, q2 = critic_groups(self.critic, self.CURL.W)
        w_sz = place(wl, True)
        enc_sz = place(enc, True)
        q_sz = place(q1, True)
        total = w_sz + enc_sz + 2 * q_sz
        self._lay = dict(w=(0, w_sz), enc=(w_sz, w_sz + enc_sz), q=(w_sz + enc_sz, total), total=total, qblock=q_sz)

        # target and critic parameters in one allocation, [target | critic]: a fixed distance apart, so the four Q
        # functions are one two-level batch (update_critic)
        both = torch.zeros(2 * total, device=dev, dtype=torch.float32)
        self._twin_outer = total if os.environ.get("CURLA_FOUR_Q", "1") != "0" else None
        # (read per agent, like the other Python-level switches: tests/test_gpu_switches.py builds one agent per value)
        self._curl_unfused = os.environ.get("CURLA_CURL_HEAD") == "unfused"

        def build(critic, W, with_grad):
            flat = both[total:] if with_grad else both[:total]
            gflat = torch.zeros(total, device=dev, dtype=torch.float32) if with_grad else None
            wl_, enc_, q1_, q2_ = critic_groups(critic, W)
            place(wl_, False, flat, gflat, 0)
            place(enc_, False, flat, gflat, w_sz)
            place(q1_, False, flat, gflat, w_sz + enc_sz)
            place(q2_, False, flat, gflat, w_sz + enc_sz + q_sz)
            critic.twin_stride = q_sz
            return flat, gflat

        self._critic_flat, self._critic_gflat = build(self.critic, self.CURL.W, True)
        self._target_flat, _ = build(self.critic_target, None, False)
        for p in self.critic_target.parameters():
            p.requires_grad_(False)

        actor_own = [(n, p) for n, p in self.actor.named_parameters() if ".convs." not in n]
        a_sz = place(actor_own, True)
        self._actor_flat = torch.zeros(a_sz, device=dev, dtype=torch.float32)
        # the actor's data-parallel bucket: [fc, ln | trunk | ops.F64_WORDS words]; the words carry log_alpha's float64
        # gradient through the bucket's all-reduce (ops.f64_pack) -- unused without data parallelism
        self._actor_gbucket = torch.zeros(a_sz + ops.F64_WORDS, device=dev, dtype=torch.float32)
        self._actor_gflat = self._actor_gbucket[:a_sz]
        self._la_words = self._actor_gbucket[a_sz:]
        place(actor_own, False, self._actor_flat, self._actor_gflat, 0)
        self.log_alpha.grad = torch.zeros((), device=dev, dtype=torch.float64)

    def _install_grad_views(self):
        """User autograd (autograd.py) against the flat gradient buffers.  A backward that finds a parameter's .grad
        unset (``zero_grad()`` sets it to None) makes a fresh tensor; the hook registered here copies it into the
        parameter's flat-buffer view and points .grad back at the view, which FlatAdam.step() requires.  Accumulation
        into an existing view is in place anyway.  Parameters that receive no gradient keep None, so the optimizers
        skip them as torch's Adam does.  ``zero_grad`` of the five optimizers marks the views as possibly dropped;
        update() restores them first (_restore_grad_views) -- a flag test, not a walk, while nothing has changed."""
        views, seen = [], set()
        for p in [self.CURL.W, *(p for _, p in self._cpc_flat_params()), self.log_alpha, *self.critic.parameters(),
                  *self.actor.parameters()]:
            if id(p) not in seen and p.grad is not None:
                seen.add(id(p))
                views.append((p, p.grad))
        self._grad_views = views
        state = self._grad_state = {"dirty": False}

        def make_hook(view):
            def hook(p):
                if p.grad is not None and p.grad is not view:
                    if p.grad.data_ptr() != view.data_ptr():
                        view.copy_(p.grad)
                    p.grad = view
            return hook
        for p, v in views:
            p.register_post_accumulate_grad_hook(make_hook(v))

        def watch(opt):
            inner = opt.zero_grad

            def zero_grad(set_to_none=True):
                state["dirty"] = True
                return inner(set_to_none)
            opt.zero_grad = zero_grad
        for opt in self._optimizers().values():
            watch(opt)

    def _restore_grad_views(self):
        if self._grad_state["dirty"]:
            self._grad_state["dirty"] = False
            for p, v in self._grad_views:
                if p.grad is not v:
                    p.grad = v

    _curl_unfused = False       # the CURL head as separate launches (set per agent from CURLA_CURL_HEAD=unfused)

    # ------------------------------------------------------------------ what the phases hand to each other
    # Ten attributes, here at their idle values.  update() sets the hints around the phase they are for and clears them
    # again, so a phase called by hand sees idle values; a call that raises goes through _reset_handover().
    _soft_update_hint = False    # hint to update_critic(): a target soft update follows the critic's step
    _soft_update_done = False    # ... and the critic's Adam launch has made it
    _pos_hint = None             # hint to the actor phase: the positives it may encode along the way
    _defer_actor_step = False    # hint to the actor phase: the CURL phase follows (overlapped data parallel)
    _actor_step_pending = False  # the actor phase has left its optimizer steps to _finish_actor_step()
    _actor_norm_log = None       # (logger, step) of a logging step while clipping is on, until the actor's step is taken
    _utd_leading = False         # set by _leading_phases around a leading sub-step (utd_ratio > 1): it records nothing
    _anchor_cache = None         # the encoder caches: the obs whose critic features (ws.z_c) the actor phase left,
    _pos_cache = None            # the obs_pos handle whose target-encoder activations sit in the workspace
    _pos_fc_done = False         # ... and whose features the actor phase has finished as well (ws.z_pos)

    def _drop_encoder_caches(self):
        """The workspace no longer holds what one phase left for the next (the critic phase's start, a reset, a redo
        pass, a loaded checkpoint)."""
        self._anchor_cache = self._pos_cache = None
        self._pos_fc_done = False

    def _reset_handover(self):
        """Back to the state a fresh ``update()`` call finds, after a call that raised: pending data-parallel work is
        waited for (not while a graph capture is open, which must not wait on a collective) and dropped, a deferred
        actor step with it, every hint and cache idle."""
        if self._dp_pending and self._graph_cap is None:
            self._allreduce_wait()
        self._dp_pending = []
        self._soft_update_hint = self._soft_update_done = self._defer_actor_step = self._actor_step_pending = False
        self._utd_leading = False
        self._pos_hint = self._actor_norm_log = None
        self._drop_encoder_caches()

    def _ws(self, B):
        if B not in self._workspaces:
            from . import _lib
            if self.device.type != "cuda" and _lib._trace_hook is None:
                raise RuntimeError("CurlSacAgent.update needs a CUDA/HIP device: the learner path has no CPU fallback")
            self._workspaces[B] = _Workspace(self, B)
        return self._workspaces[B]

    # ------------------------------------------------------------------ reference API
    def train(self, training=True):
        self.training = training
        self.actor.train(training)
        self.critic.train(training)
        self.CURL.train(training)

    @property
    def alpha(self):
        return self.log_alpha.exp()

    # ------------------------------------------------------------------ building blocks
    def _encoder_backward(self, ws, obs_ref, dz, xhat, rstd, enc, conv_grads=True, dense_done=None, twin_ld=None,
                          ln_token=None):
        """Backward of fc+LN and (optionally) the conv stack from d(loss)/d(z);
        writes .grad of enc.{ln,fc,convs}.  ``dense_done()`` is called once the fc / LayerNorm gradients are
        final, i.e. before the conv backward is enqueued (data parallel: their all-reduce starts there).
        ``twin_ld``: ``dz`` is the twin-Q input gradient [2, B, twin_ld]; d(loss)/d(z) is the sum over the twin of
        its first F columns, read in place by the LayerNorm backward."""
        B, F, K, L = obs_ref.B, enc.feature_dim, enc.flat_dim, enc.num_layers
        acts = ws.acts_main
        dy, dy2 = (dz, None) if twin_ld is None else (dz[0], dz[1])
        streams = ops.fc_bwd_streams(F, K)
        # (the LayerNorm's parameter gradients and the fc bias gradient -- column sums over the batch -- are left as
        # partial sums and finished inside the fc backward's launch, when that is one of the streaming kernels)
        # (``ln_token``: the CURL head's launch has already done the LayerNorm backward into ws.dfc and left its
        # partial sums -- and those of CURL.W's gradient -- for the fc backward to finish)
        ln = ln_token if ln_token is not None else ops.ln_bwd(
            dy, xhat, rstd, enc.ln.weight, B, F, ws.dfc, dgamma=enc.ln.weight.grad, dbeta=enc.ln.bias.grad,
            dbias_in=enc.fc.bias.grad, dy2=dy2, ld=twin_ld, defer=ws.ln_partial if streams else None)
        h = acts[-1]
        cur = L % 2
        g = ws.gviews[cur][L - 1]
        if streams and conv_grads:
            # fc weight gradient and the data gradient into the conv stack (ReLU mask of the last conv layer fused)
            # in one launch: both only read dfc
            ops.fc_bwd(ws.dfc, enc.fc.weight, h, g, enc.fc.weight.grad, B, F, K, ln=ln)
        elif streams:
            ops.fc_dw(ws.dfc, h, enc.fc.weight.grad, B, F, K, ln=ln)
        else:
            ops.linear_dw(ws.dfc, 0, h, 0, enc.fc.weight.grad, 0, B, F, K)
        if dense_done is not None:
            dense_done()
        if not conv_grads:
            return
        if not streams:
            ops.linear_dx(ws.dfc, 0, enc.fc.weight, 0, g, 0, B, F, K, mask=h)
        jobs = []
        for layer in range(L, 1, -1):  # layer l: input acts[l-2], output acts[l-1]
            conv = enc.convs[layer - 1]
            cur ^= 1
            gin = ws.gviews[cur][layer - 2]
            # weight gradient (slabs) and data gradient of the layer: both only read g, one launch for both
            n = ops.conv_s1_bwd_slabs(acts[layer - 2], g, conv.weight, gin, ws.wg_ws[layer - 1])
            jobs.append((ws.wg_ws[layer - 1], n, conv.weight.grad, conv.bias.grad))
            g = gin
        n = ops.conv1_wgrad_slabs(obs_ref, g, ws.wg_ws[0], enc.num_filters)
        jobs.append((ws.wg_ws[0], n, enc.convs[0].weight.grad, enc.convs[0].bias.grad))
        for i in range(0, len(jobs), 8):
            ops.wgrad_reduce_multi(jobs[i:i + 8])

    def _records(self, step):
        """True on the steps whose module outputs the optional histogram / image logging reads
        (log_param_hist_imgs, every LOG_FREQ steps: curl_sac.py:17,112-121,171-180)."""
        return self.log_param_hist_imgs and step % LOG_FREQ == 0 and not self._utd_leading

    def _noise(self, ws, noise):
        """(noise buffer, rng): explicit ``noise`` is copied into the buffer (rng None).  Without it
        (``torch.randn_like``, curl_sac.py:97) the policy-head launch draws the numbers itself and writes them into the
        buffer: rng = (seed, Philox counter) taken from the device's default torch generator, whose offset is moved on
        here by the numbers drawn (rounded up to 4) -- consecutive draws use NON-OVERLAPPING counters and
        torch.manual_seed, get_rng_state / set_rng_state (checkpoints) and the per-rank seeds keep their meaning.  The
        offset trajectory is this build's own: it is NOT the one a ``normal_()`` launch would leave behind (torch's
        increment depends on its grid), so a generator state saved by the ``normal_()`` path continues with different
        numbers.  Where the generator does not expose its offset this agent warns once and draws with ``normal_()``."""
        if noise is not None:
            ws.noise.copy_(noise)
            return ws.noise, None
        if self._graph_cap is not None:
            # captured update graph: (seed, counter) are read by the kernel from the update's control block; the host
            # side of the draw (the generator's offset) is advanced by the graph manager once per replay
            cap = self._graph_cap
            addr = cap["rng"][cap["n_noise"]]
            cap["n_noise"] += 1
            return ws.noise, (0, 0, addr)
        if ws.noise.is_cuda and not self._noise_launch:
            try:
                gen = torch.cuda.default_generators[ws.noise.device.index if ws.noise.device.index is not None
                                                    else torch.cuda.current_device()]
                off = gen.get_offset()
                gen.set_offset(off + 4 * ((ws.noise.numel() + 3) // 4))
                return ws.noise, (gen.initial_seed(), off // 4)
            except (AttributeError, RuntimeError) as e:
                self._noise_launch = True  # (this agent only)
                warnings.warn(f"curla_amd: the torch generator exposes no Philox offset ({e!r}); policy noise falls "
                              "back to a separate normal_() launch per phase", RuntimeWarning, stacklevel=2)
        ws.noise.normal_()
        return ws.noise, None

    _noise_launch = False  # True: this torch build's generator has no get_offset / set_offset

    def _dropout(self, rng, dropout_rng):
        """A phase's ``drop(tag)`` -> the ``drop=`` argument of Critic.twin_ln for the pass with that tag base (None
        without dropout).  The masks' stream position: ``dropout_rng`` = (seed, counter) where the caller gives one,
        else the ``rng`` of the phase's in-kernel policy-noise draw (_noise(): by value, or the control block's slot
        under capture -- nothing more is reserved and a replay draws what the eager update draws), else (explicit
        ``noise=``, the ``normal_()`` fallback) one counter reserved from the device generator."""
        if not self.critic_dropout:
            return _no_drop
        p = _check_dropout(self.critic_dropout, self.critic_layer_norm)  # (the attribute may have been edited)
        pos = dropout_rng or rng or _reserve_dropout_counter(self.device)
        return lambda tag: (p, pos, tag)

    def _encoder_backward_reduced(self, ws, obs_ref, dz, lo, hi, **kw):
        """``_encoder_backward`` of the critic's encoder from ``dz`` (``kw``: its further arguments) and the data-parallel
        reduction of the bucket [lo, hi) of the critic's flat gradient -- [convs | fc, ln | Q1 | Q2] in the critic phase,
        [W | convs | fc, ln] in the CURL phase, whose encoder gradients are reduced ONCE for both optimizers.
        Overlapped schedule: the dense piece, from fc.weight's offset to hi, is final before the conv backward starts:
        it goes asynchronously in ``dense_done`` and is reduced underneath it; the front piece goes after the conv
        backward, then the compute stream waits for both.  Blocking schedule: one all-reduce of the whole bucket after
        the backward."""
        enc, g = self.critic.encoder, self._critic_gflat
        if self._dp_active and self._dp_overlap:
            cut = self._grad_offset(enc.fc.weight, g)
            self._encoder_backward(ws, obs_ref, dz, ws.xhat_c, ws.rstd_c, enc,
                                   dense_done=lambda: self._allreduce(g[cut:hi], async_op=True), **kw)
            self._allreduce(g[lo:cut], async_op=True)
            self._allreduce_wait()
        else:
            self._encoder_backward(ws, obs_ref, dz, ws.xhat_c, ws.rstd_c, enc, **kw)
            self._allreduce(g[lo:hi])

    # -- the network passes: shapes and buffers are the workspace's and the agent's, stated here and nowhere else
    def _twin_fwd(self, ws, net, ln, out=None, outer=None):
        """The twin Q functions of ``net`` (the critic or the target) over ws.xa into ``out`` (ws.q / ws.tq), ``ln`` their
        _MlpLn.  ``outer`` = (2, floats from the target's parameters to the critic's): the target's twins over
        ws.xa2[0] and the critic's over ws.xa2[1] as one batch into ws.q2 (``net`` is the target)."""
        _, B, FA = ws.xa2.shape
        x, h1, h2, out = (ws.xa, ws.q_h1, ws.q_h2, out) if outer is None else (ws.xa2, ws.q_h1_2, ws.q_h2_2, ws.q2)
        _mlp_fwd(x, 0, net.twin(), 2, B, FA, self.hidden_dim, net.out_dim, h1, h2, out, outer=outer, ln=ln)

    def _twin_bwd(self, ws, ln, loss, grads):
        """Backward of the critic's twins over ws.xa from ``loss`` (_mlp_bwd's descriptor) into ws.dxa; ``grads``: the
        twins' parameter gradients as well (the critic phase; the actor phase takes the data gradient alone)."""
        (_, B, FA), net = ws.xa2.shape, self.critic
        _mlp_bwd(ws.xa, 0, net.twin(), net.twin(grads=True) if grads else None, 2, B, FA, self.hidden_dim, net.out_dim,
                 ws.q_h1, ws.q_h2, ws.dq, ws.q_dh2, ws.q_dh1, ws.dxa, loss=loss, ln=ln)

    # -- the critic phase's forward: a' ~ pi(. | z'), the target's twins over [z' | a'], the critic's over [z | a]
    #    (curl_sac.py:350-358), by one of three routes; each returns the phase's ``drop`` (_dropout)
    def _critic_forward(self, ws, o, no, online, noise, dropout_rng):
        """``online``: what the critic encoder's LayerNorm launch is given beside z (its saves, xa = [z | a], the
        record's fc_out)."""
        B = o.B
        pair = getattr(o, "pair", None)
        if pair is None or pair[1] is not no or pair[0].B != 2 * B:
            return self._q_unmerged(ws, o, no, online, noise, dropout_rng)
        # obs and next_obs both go through the online convs (the actor's are tied to the critic's): the buffer handed
        # them over as one [obs | next_obs] handle, so they take ONE launch per layer (2B samples), the target encoder's
        # pass over next_obs rides in the same launches (second problem, own weights) and the three fc products --
        # all three activation tensors are there -- take one
        enc, tenc = self.critic.encoder, self.critic_target.encoder
        enc.conv_forward2(pair[0], ws.acts_pair, tenc, no, ws.acts_tmp)
        CNNEncoder.fc_partial_multi([(self.actor.encoder, ws.acts_pair[-1][B:]), (tenc, ws.acts_tmp[-1]),
                                     (enc, ws.acts_main[-1])])
        route = self._q_merged if self._twin_outer is None else self._q_four
        return route(ws, B, online, noise, dropout_rng)

    def _next_policy(self, ws, noise, dropout_rng, **outs):
        """The phase's noise draw and dropout stream, then the actor trunk over ws.z_a and the policy head, which writes
        log_pi and ``outs``."""
        nz, rng = self._noise(ws, noise)
        drop = self._dropout(rng, dropout_rng)
        self._actor_fwd(ws, nz, log_pi=ws.log_pi, rng=rng, **outs)
        return drop

    def _q_four(self, ws, B, online, noise, dropout_rng):
        """Four Q functions in one batch: the target's twins over [z' | a'] and the critic's over [z | a] are four MLPs
        of one shape and share their three launches, the three encoders' features (actor, target, critic) their one
        -- the action columns of [z' | a'] are then written by the policy head.  (Dropout groups: tags 1 / 2, 3 / 4.)"""
        enc, tq = self.critic.encoder, self.critic_target
        CNNEncoder.ln_from_partial_multi(B, [(self.actor.encoder, ws.z_a, {}), (tq.encoder, ws.z_t, dict(xa=ws.xa2[0])),
                                             (enc, ws.z_c, online)], self.action_dim)
        drop = self._next_policy(ws, noise, dropout_rng, pi=None, xa=ws.xa2[0])
        self._twin_fwd(ws, tq, tq.twin_ln(*ws.q_ln_saves, save_first=1, drop=drop(1)), outer=(2, self._twin_outer))
        return drop

    def _q_merged(self, ws, B, online, noise, dropout_rng):
        """Merged convs, separate Q passes (CURLA_FOUR_Q=0)."""
        self.actor.encoder.ln_from_partial(B, ws.z_a)
        drop = self._next_policy(ws, noise, dropout_rng, pi=ws.pi, xa=None)
        self._target_q(ws, B, drop)
        self._online_q(ws, B, online, drop)
        return drop

    def _q_unmerged(self, ws, o, no, online, noise, dropout_rng):
        """Fully separate passes (a buffer without the [obs | next_obs] handle): every conv stack on its own."""
        B = o.B
        enc, aenc, tenc = self.critic.encoder, self.actor.encoder, self.critic_target.encoder
        aenc.fc_partial(enc.conv_forward(no, ws.acts_tmp))  # tied convs, online weights
        aenc.ln_from_partial(B, ws.z_a)
        drop = self._next_policy(ws, noise, dropout_rng, pi=ws.pi, xa=None)
        tenc.fc_partial(tenc.conv_forward(no, ws.acts_tmp))
        self._target_q(ws, B, drop)
        enc.fc_partial(enc.conv_forward(o, ws.acts_main))
        self._online_q(ws, B, online, drop)
        return drop

    def _target_q(self, ws, B, drop):
        tq = self.critic_target
        tq.encoder.ln_from_partial(B, ws.z_t, xa=ws.xa, act=ws.pi)  # xa = cat([z', a'], 1)
        self._twin_fwd(ws, tq, tq.twin_ln(drop=drop(1)), ws.tq)

    def _online_q(self, ws, B, online, drop):
        self.critic.encoder.ln_from_partial(B, ws.z_c, **online)  # xa = cat([z, a], 1)
        self._twin_fwd(ws, self.critic, self.critic.twin_ln(*ws.q_ln_saves, drop=drop(3)), ws.q)

    # ------------------------------------------------------------------ phases
    def update_critic(self, obs, action, reward, next_obs, not_done, L, step, noise=None, dropout_rng=None):
        """curl_sac.py:349-371.  ``dropout_rng`` = (seed, counter): the stream position of a dropout critic's masks
        (the target twins under tags 1 / 2, the critic twins under 3 / 4) instead of the phase's own (_dropout)."""
        per = getattr(obs, "per", None)
        settings = self._critic_loss_settings(per)  # (checked before anything is written)
        self._restore_grad_views()
        o, no = _as_ref(obs), _as_ref(next_obs)
        ws, enc = self._ws(o.B), self.critic.encoder
        self._note_critic_batch(o.B)
        self._drop_encoder_caches()
        action, reward, not_done = action.contiguous(), reward.contiguous(), not_done.contiguous()
        # -- target (no_grad block, curl_sac.py:350-355) and current Q estimates (:357-358)
        rec = self._records(step)
        online = dict(xhat=ws.xhat_c, rstd=ws.rstd_c, fc_out=ws.fc_out if rec else None, xa=ws.xa, act=action)
        drop = self._critic_forward(ws, o, no, online, noise, dropout_rng)
        if rec:  # what critic.log() / encoder.log() histogram: the outputs of THIS forward (curl_sac.py:163-167)
            self.critic.outputs['q1'], self.critic.outputs['q2'] = ws.q[0].clone(), ws.q[1].clone()
            enc.record_from(o, ws.acts_main, ws.fc_out, ws.z_c)
        # -- loss + backward (curl_sac.py:359-367)
        loss = self._critic_loss(ws, reward, not_done, per, settings)
        self._twin_bwd(ws, self.critic.twin_ln(*ws.q_ln_saves, grads=True, partial=ws.q_ln_partial, drop=drop(3)), loss,
                       grads=True)
        if step % self.log_interval == 0:
            L.log('train_critic/loss', ws.scalars[0], step)
        # (d(loss)/d(z) = dxa[0][:, :F] + dxa[1][:, :F], torch.cat's backward: summed inside the LayerNorm backward)
        self._encoder_backward_reduced(ws, o, ws.dxa, self._lay["enc"][0], self._lay["total"],
                                       conv_grads=not self.detach_encoder, twin_ld=ws.xa.shape[1])
        self._critic_step()
        if self._max_grad_norm is not None and step % self.log_interval == 0:
            L.log('train_critic/grad_norm', self.grad_clip_stats[0, 0], step)
        if self.log_param_hist_imgs:
            self.critic.log(L, step)

    def update_actor_and_alpha(self, obs, L, step, noise=None, dropout_rng=None):
        """curl_sac.py:373-404.  Only the live gradients are produced: the
        actor's own fc/ln/trunk and log_alpha (the reference also deposits
        gradients on critic tensors that are zeroed before any step reads them)."""
        self._restore_grad_views()
        o = _as_ref(obs)
        B, A, ws = o.B, self.action_dim, self._ws(o.B)
        enc, aenc, tenc = self.critic.encoder, self.actor.encoder, self.critic_target.encoder
        # one conv pass feeds actor.fc, critic.fc and (even steps) the CURL anchor branch; when update() knows that the
        # CURL phase follows with unchanged target weights, the target encoder's pass over the positives rides in the
        # same launches (second problem) and update_cpc finds its activations ready
        pos, self._pos_hint = self._pos_hint, None
        if pos is not None:
            enc.conv_forward2(o, ws.acts_main, tenc, pos, ws.acts_tmp)
            self._pos_cache = pos
        else:
            enc.conv_forward(o, ws.acts_main)
        # actor.fc and critic.fc read the same conv output, one launch; so are the features: actor's, critic's (kept
        # for the CURL anchor branch; the action columns of xa = cat([z, pi], 1) come from the policy head below) --
        # and, third problem of both launches, the positives' target features
        h = ws.acts_main[-1]
        fcs = [(aenc, h), (enc, h)]
        lns = [(aenc, ws.z_a, dict(xhat=ws.xhat_a, rstd=ws.rstd_a)),
               (enc, ws.z_c, dict(xhat=ws.xhat_c, rstd=ws.rstd_c, xa=ws.xa))]
        if pos is not None:
            fcs.append((tenc, ws.acts_tmp[-1]))
            lns.append((tenc, ws.z_pos, {}))
            self._pos_fc_done = True
        CNNEncoder.fc_partial_multi(fcs)
        CNNEncoder.ln_from_partial_multi(B, lns, A)
        self._anchor_cache = obs

        nz, rng = self._noise(ws, noise)
        self._actor_fwd(ws, nz, rng=rng, **self._actor_phase_outs(ws))
        if self._records(step):  # what actor.log() histograms (curl_sac.py:92-93): pre-squash mean and std
            self.actor.outputs['mu'], self.actor.outputs['std'] = ws.a_out[:, :A].clone(), ws.log_std.exp()
        # (the data gradient through the LayerNorms needs the saves too; dropout: the critic twins under tags 5 / 6)
        q_ln = self.critic.twin_ln(*ws.q_ln_saves, drop=self._dropout(rng, dropout_rng)(5))
        self._twin_fwd(ws, self.critic, q_ln, ws.q)
        # backward: Q -> pi -> trunk -> LN -> fc (encoder detached, curl_sac.py:375-376)
        self._twin_bwd(ws, q_ln, self._actor_loss(ws), grads=False)
        if step % self.log_interval == 0:
            self._log_actor(ws, L, step)
        F, trunk = aenc.feature_dim, self.actor.trunk
        self._actor_head_bwd(ws, nz, B, A, F)
        _mlp_bwd(ws.z_a, 0, _Mlp(trunk), _Mlp(trunk, grads=True), 1, B, F, self.hidden_dim, self._actor_out_dim(), ws.a_h1,
                 ws.a_h2, ws.a_dout, ws.a_dh2, ws.a_dh1, ws.dz)
        self._encoder_backward(ws, o, ws.dz, ws.xhat_a, ws.rstd_a, aenc, conv_grads=False)
        self._actor_reduce_and_step(L, step)
        if self.log_param_hist_imgs:
            self.actor.log(L, step)
        if step % self.log_interval == 0:
            self._log_actor(ws, L, step, alpha=True)

    def update_cpc(self, obs_anchor, obs_pos, cpc_kwargs, L, step, action=None):
        """curl_sac.py:406-423.  ``action`` (``cpc_objective="predictive"`` only, required then: the minibatch's actions):
        the head behind the two encoders is the self-predictive one (agent_cpc.py) in place of CURL's."""
        oa, op_ = _as_ref(obs_anchor), _as_ref(obs_pos)
        action = self._check_cpc_action(action, oa.B)  # (before anything is written)
        self._restore_grad_views()
        B, ws = oa.B, self._ws(oa.B)
        enc, tenc = self.critic.encoder, self.critic_target.encoder
        need_anchor = self._anchor_cache is None or self._anchor_cache is not obs_anchor
        need_pos = self._pos_cache is None or self._pos_cache is not obs_pos
        pos_fc_done = self._pos_fc_done and not need_pos
        self._drop_encoder_caches()
        if need_anchor and need_pos:   # (odd steps) both passes in one launch per layer, own weights each
            enc.conv_forward2(oa, ws.acts_main, tenc, op_, ws.acts_tmp)
        elif need_anchor:
            enc.conv_forward(oa, ws.acts_main)
        elif need_pos:
            tenc.conv_forward(op_, ws.acts_tmp)
        if need_anchor:
            CNNEncoder.fc_partial_multi([(enc, ws.acts_main[-1]), (tenc, ws.acts_tmp[-1])])
            CNNEncoder.ln_from_partial_multi(B, [(enc, ws.z_c, dict(xhat=ws.xhat_c, rstd=ws.rstd_c)),
                                                 (tenc, ws.z_pos, {})])
        elif not pos_fc_done:  # (done: the actor phase left the positives' features in ws.z_pos)
            tenc.fc_partial(ws.acts_tmp[-1])
            tenc.ln_from_partial(B, ws.z_pos)

        logged = step % self.log_interval == 0  # the mean of the row losses is only needed when it is logged
        if action is not None:
            self._predictive_head(ws, oa, action, logged)
        else:
            self._infonce_head(ws, oa, logged)
        self._cpc_steps()
        if logged:
            L.log(self._cpc_loss_key(), ws.scalars[5], step)
            if self._max_grad_norm is not None:
                L.log('train/curl_grad_norm', self.grad_clip_stats[2, 0], step)

    # The drop-in contract pins update_cpc's parameter list to the reference's five names (tests/test_dropin_contract.py),
    # as it pins __init__'s: introspection keeps showing those, and ``action`` is a keyword accepted behind them.
    update_cpc.__signature__ = inspect.Signature(
        [p for p in inspect.signature(update_cpc).parameters.values() if p.name != "action"])

    def _infonce_head(self, ws, oa, logged):
        """CURL's head behind ws.z_c / ws.z_pos (curl_sac.py:211-222, 411-417) and the encoder's backward."""
        B, enc = oa.B, self.critic.encoder
        F, W = enc.feature_dim, self.CURL.W
        ops.linear_fwd(ws.z_pos, 0, W, 0, None, 0, ws.WzT, 0, B, F, F)         # (W z_pos^T)^T
        # logits, cross-entropy, d z_a, the LayerNorm backward and the partial sums of dW in ONE launch where the
        # shapes allow (and the fc backward is a streaming kernel, whose extra workgroup finishes the partial sums)
        token = None
        views = self.aug_views == 2  # (the partner column is no negative: the unfused route, the fused head has no mask)
        if ops.curl_head_supported(B, F) and ops.fc_bwd_streams(F, enc.flat_dim) and not self._curl_unfused and not views:
            token = ops.curl_head(ws.z_c, ws.z_pos, ws.WzT, ws.xhat_c, ws.rstd_c, enc.ln.weight, B, F, ws.row_loss, ws.dfc,
                                  ws.ln_partial, ws.w_partial, enc.ln.weight.grad, enc.ln.bias.grad, enc.fc.bias.grad,
                                  W.grad, loss=ws.scalars[5:6] if logged else None, logits=ws.logits, dz=ws.dz)
        else:
            ops.linear_fwd(ws.z_c, 0, ws.WzT, 0, None, 0, ws.logits, 0, B, B, F)   # z_a (W z_pos^T)
            ce = ops.curl_ce_views if views else ops.curl_ce
            ce(ws.logits, B, B, ws.row_loss, ws.scalars[5:6] if logged else None, ws.dlogits)
            ops.linear_dx(ws.dlogits, 0, ws.WzT, 0, ws.dz, 0, B, B, F)             # d z_a
            ops.linear_dw(ws.dlogits, 0, ws.z_c, 0, ws.dWzT, 0, B, B, F)           # d (W z_pos^T)^T
            ops.linear_dw(ws.dWzT, 0, ws.z_pos, 0, W.grad, 0, B, F, F)             # d W
        self._encoder_backward_reduced(ws, oa, ws.dz, 0, self._lay["enc"][1], ln_token=token)

    def update(self, replay_buffer, L, step, only_cpc=False, noise=None):
        """curl_sac.py:426-451.  A curla_amd ReplayBuffer hands over references
        into its HBM ring (gather + crop fused into the first conv); any other
        buffer is used through the reference's ``sample_cpc()`` tensors.
        ``noise`` (parity tests): (critic-phase, actor-phase) tensors in place of the two ``torch.randn_like`` draws
        (curl_sac.py:97 via :352 and :375).

        ``utd_ratio = G > 1``: the call draws G minibatches, one after the other, each through the
        buffer's ordinary route, so NumPy's and torch's host streams and the device generator move exactly as G
        separate samples and G separate critic phases move them.
          leading sub-steps (minibatches 0 .. G-2): the critic phase, and the target soft update iff
              ``step % critic_target_update_freq == 0`` -- ALL sub-steps of a call share the call's ``step`` (DroQ /
              RLPD users set ``critic_target_update_freq=1``); fused into the critic's Adam launch where a critic-only
              update fuses it.  No actor phase, no CURL phase, nothing logged or recorded; a curla_amd buffer is told
              that the positive is not wanted (``sample_cpc_refs(want_pos=False)``).
          final sub-step (minibatch G-1): the whole update as with ``utd_ratio = 1`` -- every frequency, the logging
              (each ``train_*`` key once per call) and the records.
        ``only_cpc=True`` has no critic phase: one minibatch, no leading sub-steps.  A prioritized buffer's sub-step
        draws from the priorities the previous one left and updates those of its own rows; data parallel, every
        sub-step reduces its critic bucket as a critic-only update does and ``check_replicas()`` runs at most once, in
        front of the first; ``set_max_grad_norm`` clips per sub-step.  A sub-step that raises ends the call.
        The state after the call -- parameters, targets, optimizer state, priorities, generator positions -- is bit
        for bit that of G-1 critic-only ``update()`` calls (a ``step`` without actor and CURL phase, the same soft-update
        decision) followed by the ordinary call with ``utd_ratio = 1``.  ``noise`` is a hook for one minibatch and is
        refused with G > 1."""
        self._restore_grad_views()
        self._policy_schedule_step(step)  # (before the eager / graph route is chosen: the policy's std is data)
        self._check_n_step(replay_buffer)
        self._check_cpc_buffer(replay_buffer)
        self._check_aug_views(replay_buffer)
        self._maybe_reset(step)  # (reset_interval: in front of every sub-step, graphed or not)
        if self.utd_ratio != 1 or type(self.utd_ratio) is not int:  # (the attribute may have been edited)
            if _check_utd_ratio(self.utd_ratio) > 1 and noise is not None and not only_cpc:
                raise ValueError("update(noise=...) stands for the draws of one minibatch: not with utd_ratio = %d"
                                 % self.utd_ratio)
        if noise is None and self._graphs is not None and self._graph_usable(replay_buffer, step, only_cpc):
            return self._update_graphed(replay_buffer, L, step)
        self._update_eager(replay_buffer, L, step, only_cpc, noise)

    def _check_n_step(self, replay_buffer):
        """An n-step buffer composes its rewards with ITS discount and the TD kernels bootstrap with the agent's: the
        two must be one number, or the target is neither's."""
        if getattr(replay_buffer, "n_step", 1) > 1 and replay_buffer.discount != self.discount:
            raise ValueError("replay_buffer.discount = %r (n_step = %d) differs from the agent's discount = %r"
                             % (replay_buffer.discount, replay_buffer.n_step, self.discount))

    def _check_aug_views(self, replay_buffer):
        """The agent's losses pair position b with b + B / 2 exactly when the buffer draws them as one transition: the two
        must say the same (a buffer without the attribute draws one view)."""
        views = getattr(replay_buffer, "aug_views", 1)
        if views != self.aug_views:
            raise ValueError("replay_buffer.aug_views = %r differs from the agent's aug_views = %r"
                             % (views, self.aug_views))

    def _update_eager(self, replay_buffer, L, step, only_cpc=False, noise=None):
        leading = 0 if only_cpc else self.utd_ratio - 1
        for k in range(leading):
            self._substep_eager(replay_buffer, None, step, leading=True, first=k == 0)
        self._substep_eager(replay_buffer, L, step, only_cpc, noise, first=leading == 0)

    def _substep_eager(self, replay_buffer, L, step, only_cpc=False, noise=None, leading=False, first=True):
        """One minibatch of an update: drawn, then its phases.  ``leading``: a sub-step in front of the last one of a
        utd_ratio > 1 call; ``first``: the call's first sub-step, where the replicas are checked."""
        if hasattr(replay_buffer, "sample_cpc_refs"):
            if leading and self._takes_want_pos(replay_buffer):
                sample = replay_buffer.sample_cpc_refs(want_pos=False)
            else:
                sample = replay_buffer.sample_cpc_refs()
        else:
            sample = replay_buffer.sample_cpc()

        if self._replica_check_due(step, first):
            self.check_replicas()
        if leading:
            self._leading_phases(sample, step)
        else:
            self._update_phases(sample, L, step, only_cpc, noise)
            if self._redo_due(step, only_cpc):  # (redo_interval: behind the optimizer steps of the final sub-step)
                self._redo_scheduled(sample[0], sample[1], L, step)

    _want_pos_known = (None, False)

    def _takes_want_pos(self, replay_buffer):
        """Whether the buffer's ``sample_cpc_refs`` takes ``want_pos`` (this package's does; a look-alike need not)."""
        cls, ok = self._want_pos_known
        if cls is not type(replay_buffer):
            try:
                ok = "want_pos" in inspect.signature(replay_buffer.sample_cpc_refs).parameters
            except (TypeError, ValueError):
                ok = False
            self._want_pos_known = (type(replay_buffer), ok)
        return ok

    def _leading_phases(self, sample, step):
        """The phases of a leading sub-step (utd_ratio > 1) on a drawn minibatch: logged to nobody, nothing recorded."""
        self._utd_leading = True
        try:  # (one that raises: no later sub-step runs, _update_phases has reset the hand-over state)
            self._update_phases(sample, _NullLog(), step, leading=True)
        finally:
            self._utd_leading = False

    def _update_phases(self, sample, L, step, only_cpc=False, noise=None, leading=False):
        """The phases of one update on a drawn minibatch (curl_sac.py:431-451).  ``leading`` (_leading_phases): the critic
        phase and, by ``step``, the target soft update -- the update kind (actor=False, soft, cpc=False) whatever the
        other frequencies say.  A phase that raises: the next call starts as a fresh one (_reset_handover) -- the
        collective of a deferred actor step is waited for and dropped with the step, not left to a later update."""
        try:
            self._phases(sample, L, step, only_cpc, noise, leading)
        except BaseException:
            self._reset_handover()
            raise

    def _phases(self, sample, L, step, only_cpc, noise, leading):
        obs, action, reward, next_obs, not_done, cpc_kwargs = sample
        noise_c, noise_a = noise if noise is not None else (None, None)
        if step % self.log_interval == 0 and not leading:
            ws = self._ws(action.shape[0])
            ops.mean(reward.contiguous(), reward.numel(), ws.scalars[6:7])
            L.log('train/batch_reward', ws.scalars[6], step)

        do_cpc = (not self.pixel_sac) and step % self.cpc_update_freq == 0 and not leading
        if not only_cpc:
            soft = step % self.critic_target_update_freq == 0
            # (the hints are set around the phase they are for: a phase called by hand sees idle values)
            self._soft_update_hint, self._soft_update_done = soft, False
            self.update_critic(obs, action, reward, next_obs, not_done, L, step, noise=noise_c)
            self._soft_update_hint = False
            # The target soft update reads the critic's parameters, which the actor phase does not touch (it steps the
            # actor's own tensors and log_alpha): applied BEFORE the actor phase it gives the same numbers as after
            # it (curl_sac.py:437-445), and the target encoder is then final when the actor phase encodes obs -- so
            # the positives' target pass can share those launches.  (Normally it has already happened: inside the
            # critic's Adam launch.)
            if soft and not self._soft_update_done:
                self.soft_update_targets()
            if step % self.actor_update_freq == 0 and not leading:
                if do_cpc and isinstance(cpc_kwargs.get("obs_pos"), ObsRef):
                    self._pos_hint = cpc_kwargs["obs_pos"]
                self._defer_actor_step = do_cpc
                self.update_actor_and_alpha(obs, L, step, noise=noise_a)
                self._pos_hint, self._defer_actor_step = None, False

        if do_cpc:
            obs_anchor, obs_pos = cpc_kwargs["obs_anchor"], cpc_kwargs["obs_pos"]
            self.update_cpc(obs_anchor, obs_pos, cpc_kwargs, L, step, **self._cpc_call_kw(action))
        self._finish_actor_step()
