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
from .agent_dp import _DataParallelMixin
from .agent_graphs import _NullLog, _UpdateGraphsMixin
from .agent_redo import _check_redo_interval, _check_redo_recycle, _check_redo_tau, _RedoMixin
from .agent_reset import _check_reset_interval, _check_reset_keep, _check_reset_seed, _ResetMixin
from .encoder import CNNEncoder
from .mlp import _Mlp, _MlpLn, _linears, _mlp_bwd, _mlp_fwd  # noqa: F401
from .networks import (CURL, LOG_FREQ, Actor, Critic, QFunction, _check_drop_quantiles,  # noqa: F401
                       _check_bin_sigma, _check_bins, _check_dropout, _check_int, _check_layer_norm_width,
                       _check_policy_std, _check_policy_std_clip, _check_quantiles, _check_value_range, _CriticType,
                       _device_generator, _QFunctionType, _reserve_dropout_counter, _widen_last_layers, weight_init)
from .ops import ObsRef
from .optim import FlatAdam, check_max_grad_norm, check_weight_decay


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
        M = agent.critic.out_dim  # (critic_quantiles: M atoms per Q function in place of the one Q value)
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
        # the quantile loss per row (ops.tqc_critic_loss); critic_bins: the cross-entropies per row (ops.hlg_critic_loss)
        # in the critic phase, min(Q1, Q2) per row (ops.hlg_actor_loss) in the actor phase
        self.q_row_loss = f(B) if agent.critic_quantiles or agent.critic_bins else None
        self.per_w = self.per_value = None  # importance weights / new stored values [B]: a prioritized buffer's updates only
        # scalars: [0] critic loss, [1..4] actor_loss/alpha_loss/entropy/alpha, [5] curl loss, [6] batch reward
        self.scalars = torch.zeros(8, device=dev, dtype=torch.float32)
        # CURL
        self.WzT, self.dWzT = f(B, F), f(B, F)
        self.logits, self.dlogits, self.row_loss = f(B, B), f(B, B), f(B)


class _AgentType(type):
    """``CurlSacAgent(...)`` takes the reference's arguments and, behind them, this package's own keywords.
    ``CurlSacAgent.__init__`` keeps the reference's parameter list name for name (curl_sac.py:226-256: the drop-in
    contract, tests/test_dropin_contract.py); a keyword that shapes the networks has to be known before ``__init__``
    builds them, so the class call takes it off the arguments and leaves it on the instance."""

    def __call__(cls, *args, policy="gaussian", policy_std=0.2, policy_std_clip=0.3, policy_std_schedule=None,
                 aug_views=1, redo_interval=0, redo_tau=0.1, redo_recycle=True, reset_interval=0,
                 reset_encoder_keep=1.0, reset_seed=0, critic_quantiles=0, critic_drop_quantiles=0, critic_bins=0,
                 critic_value_range=None, critic_bin_sigma=0.75, weight_decay=0.0, utd_ratio=1, critic_dropout=0.0,
                 critic_layer_norm=False, **kwargs):
        agent = cls.__new__(cls)
        if _check_policy(policy) == "deterministic":  # (gaussian: the instance is the one without the keyword)
            agent.policy = "deterministic"
            agent.policy_std_schedule = _check_policy_std_schedule(policy_std_schedule)
            agent._policy_std = _check_policy_std(policy_std)
            if agent.policy_std_schedule is not None:  # (the schedule's value at step 0 until the first update)
                agent._policy_std = _check_policy_std(_linear_schedule(agent.policy_std_schedule, 0))
            agent.policy_std_clip = _check_policy_std_clip(policy_std_clip)
        else:
            for name, value, default in (("policy_std", policy_std, 0.2), ("policy_std_clip", policy_std_clip, 0.3),
                                         ("policy_std_schedule", policy_std_schedule, None)):
                if value is not default and value != default:
                    raise ValueError("%s = %r needs policy='deterministic' (the Gaussian policy learns its own standard "
                                     "deviation)" % (name, value))
        agent.redo_interval = _check_redo_interval(redo_interval)
        agent.redo_tau = _check_redo_tau(redo_tau)
        agent.redo_recycle = _check_redo_recycle(redo_recycle)
        agent.reset_interval = _check_reset_interval(reset_interval)
        agent.reset_encoder_keep = _check_reset_keep(reset_encoder_keep)
        agent.reset_seed = _check_reset_seed(reset_seed)
        agent.critic_quantiles = _check_quantiles(critic_quantiles)
        agent.critic_drop_quantiles = _check_drop_quantiles(critic_drop_quantiles, agent.critic_quantiles)
        agent.critic_layer_norm = bool(critic_layer_norm)
        agent.critic_dropout = _check_dropout(critic_dropout, agent.critic_layer_norm)
        agent.utd_ratio = _check_utd_ratio(utd_ratio)
        bin_sigma = _check_bin_sigma(critic_bin_sigma)
        if _check_bins(critic_bins):  # (0: the instance is the one without the keyword, down to its __dict__)
            if agent.critic_quantiles:
                raise ValueError("critic_bins > 0 is not combined with critic_quantiles > 0: a Q function's last layer is "
                                 "the logits of one categorical distribution or a set of quantile atoms")
            if critic_value_range is None:
                raise ValueError("critic_bins = %d needs critic_value_range=(v_min, v_max), the range of the returns the "
                                 "bins cover" % critic_bins)
            agent.critic_bins = int(critic_bins)
            agent.critic_value_range = _check_value_range(critic_value_range)
            agent.critic_bin_sigma = bin_sigma
        elif critic_value_range is not None:
            raise ValueError("critic_value_range needs critic_bins > 0")
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


class CurlSacAgent(_ActingMixin, _DataParallelMixin, _UpdateGraphsMixin, _ResetMixin, _RedoMixin, metaclass=_AgentType):
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
    three ``policy_std*`` keywords raise beside the Gaussian policy."""

    policy = "gaussian"
    policy_std_clip = None
    policy_std_schedule = None
    _policy_std = None
    critic_layer_norm = False
    critic_dropout = 0.0
    utd_ratio = 1
    critic_quantiles = 0
    critic_drop_quantiles = 0
    aug_views = 1
    critic_bins = 0
    critic_value_range = None
    critic_bin_sigma = 0.75
    _hlg_last_B = None  # critic_bins: the batch size of the last critic phase (target_clip_fraction's workspace)

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

        self._to_flat_device_layout()
        if self.policy == "deterministic":
            # the standard deviation the head kernels read on the device, and where the actor loss launches leave their
            # d(alpha loss)/d(log_alpha): log_alpha.grad stays all zeros, so its Adam step leaves it bit for bit alone
            self.actor.std = torch.full((1,), self._policy_std, device=self.device, dtype=torch.float32)
            self.actor.std_clip = self.policy_std_clip
            self._dla_scratch = torch.zeros((), device=self.device, dtype=torch.float64)

        actor_own = [p for n, p in self.actor.named_parameters() if ".convs." not in n]
        enc_params = list(self.critic.encoder.parameters())
        # Optimizers (curl_sac.py:299-313).  The reference hands Adam the tied convs (actor) and the target
        # encoder (cpc) as well; their .grad is always None at step time there, so Adam never touches them.
        # FlatAdam is torch.optim.Adam with its step() as one HIP launch over the flat buffer (optim.py);
        # CURLA_TORCH_ADAM=1 keeps torch's own fused multi-tensor step (same state_dict either way).
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
        self.cpc_optimizer = adam([self.CURL.W] + enc_params, cf, cg, lr=encoder_lr)
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
          critic flat : [ CURL.W | encoder (convs, fc, ln) | Q1 | Q2 ]
          target flat : same layout (W slot unused)
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
            return [("W", W)] if W is not None else [], enc, q1, q2

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
        for p in [self.CURL.W, self.log_alpha, *self.critic.parameters(), *self.actor.parameters()]:
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

    # -- the deterministic policy
    def _actor_kw(self):
        """The keyword that shapes the actor, for every place that builds one."""
        return dict(deterministic=True) if self.policy == "deterministic" else {}

    def _actor_out_dim(self):
        """The width of the actor trunk's last layer: [mu | raw log_std], or the deterministic policy's A means."""
        return self.action_dim if self.policy == "deterministic" else 2 * self.action_dim

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

    # -- the network passes: shapes and buffers are the workspace's and the agent's, stated here and nowhere else
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

    def _critic_width_kw(self):
        """The keywords that widen the Q functions' last layers, for every place that builds a Critic."""
        if self.critic_bins:
            return dict(bins=self.critic_bins, value_range=self.critic_value_range)
        return dict(quantiles=self.critic_quantiles) if self.critic_quantiles else {}

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

    # -- the loss descriptors of _twin_bwd: (fields, launch) -- ``fields`` for the form computed inside the backward
    #    launch of the Q functions' last layer, ``launch()`` the loss kernel on its own where that form does not apply
    def _critic_loss(self, ws, reward, not_done, per, drop_q, hlg=None):
        """target_Q = r + not_done * gamma * (min Q' - alpha log pi'), the two MSE terms and their gradient dq
        (curl_sac.py:353-361).  ``critic_quantiles``: the quantile Huber loss of the critic's atoms against
        the kept target atoms, always a launch of its own.  ``aug_views = 2``: both views' estimates against
        the mean of the two views' targets, a launch of its own as well.  ``critic_bins``: the two
        cross-entropies of the critic's logits against the Gaussian histogram of the clamped TD target, with or without
        views, always a launch of its own; ``hlg`` = (v_min, v_max, sigma) as update_critic has checked them.  ``per``, a
        prioritized minibatch: the loss is
        launched here, the importance weights scale dq and the loss in place and the drawn rows get their new priorities
        -- all on the device --, and the backward runs on the weighted dq it finds: no descriptor, None."""
        B, Mq = ws.log_pi.shape[0], self.critic.out_dim
        la, gamma, total = self.log_alpha, self.discount, ws.scalars[0:1]
        if self.critic_quantiles:
            loss = (None, lambda: ops.tqc_critic_loss(ws.q, B * Mq, ws.tq, B * Mq, ws.log_pi, reward, not_done, la, gamma,
                                                      B, Mq, drop_q, ws.dq, B * Mq, ws.q_row_loss, total))
        elif self.critic_bins:  # (a prioritized minibatch has been refused by update_critic)
            v_min, v_max, sigma = hlg
            return None, lambda: ops.hlg_critic_loss(ws.q, B * Mq, ws.tq, B * Mq, ws.log_pi, reward, not_done, la, gamma, B,
                                                     Mq, v_min, v_max, sigma, ws.dq, B * Mq, ws.target_q, ws.q_row_loss,
                                                     total, views=self.aug_views == 2)
        elif self.aug_views == 2:
            if per is not None:
                raise ValueError("aug_views = 2: a prioritized minibatch is not supported (its rows are drawn per "
                                 "position): use ReplayBuffer(prioritized=False)")
            return None, lambda: ops.critic_td_loss_views(ws.q, ws.tq, B, ws.log_pi, reward, not_done, la, gamma, B,
                                                          ws.target_q, total, ws.dq)
        else:
            loss = (dict(kind=1, twin_stride=B, q=ws.q, target_q_twin=ws.tq, log_pi=ws.log_pi, reward=reward,
                         not_done=not_done, log_alpha=la, discount=gamma, target_q=ws.target_q, scalars=total, dq=ws.dq),
                    lambda: ops.critic_td_loss(ws.q, ws.tq, B, ws.log_pi, reward, not_done, la, gamma, B, ws.target_q,
                                               total, ws.dq))
        if per is None:
            return loss
        if ws.per_w is None:
            ws.per_w, ws.per_value = (torch.empty(B, device=ws.dq.device, dtype=torch.float32) for _ in range(2))
        loss[1]()
        per.td_update(ws.q, B, ws.target_q, ws.dq, total, ws.per_w, ws.per_value)
        return None

    def _actor_loss(self, ws):
        """The actor / alpha losses and d(loss)/dQ (curl_sac.py:377-401); ``critic_quantiles``: over the mean of all
        atoms in place of min(Q1, Q2), a launch of its own."""
        B, A, Mq = ws.log_pi.shape[0], self.action_dim, self.critic.out_dim
        la, te, out = self.log_alpha, float(self.target_entropy), ws.scalars[1:5]
        # (the deterministic policy: log_pi = 0 and the temperature takes no part -- its gradient goes to a scratch word)
        dla = self._dla_scratch if self.policy == "deterministic" else la.grad
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

    # ------------------------------------------------------------------ phases
    def update_critic(self, obs, action, reward, next_obs, not_done, L, step, noise=None, dropout_rng=None):
        """curl_sac.py:349-371.  ``dropout_rng`` = (seed, counter): the stream position of a dropout critic's masks
        (the target twins under tags 1 / 2, the critic twins under 3 / 4) instead of the phase's own (_dropout)."""
        per, drop_q = getattr(obs, "per", None), 0
        if self.critic_quantiles:
            drop_q = _check_drop_quantiles(self.critic_drop_quantiles, self.critic.out_dim)  # (it may have been edited)
            if per is not None:
                raise ValueError("critic_quantiles: a prioritized minibatch is not supported (its priorities are built "
                                 "on one scalar TD error per Q function): use ReplayBuffer(prioritized=False)")
        hlg = None
        if self.critic_bins:
            hlg = self._hlg_params()  # (the range or the smoothing may have been edited: checked before anything is written)
            if per is not None:
                raise ValueError("critic_bins: a prioritized minibatch is not supported (its priorities are built on one "
                                 "scalar TD error per Q function): use ReplayBuffer(prioritized=False)")
        self._restore_grad_views()
        o, no = _as_ref(obs), _as_ref(next_obs)
        ws, enc = self._ws(o.B), self.critic.encoder
        if hlg is not None:
            self._hlg_last_B = o.B
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
        loss = self._critic_loss(ws, reward, not_done, per, drop_q, hlg)
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

        det = self.policy == "deterministic"
        nz, rng = self._noise(ws, noise)
        self._actor_fwd(ws, nz, mu=ws.mu, pi=None if det else ws.pi, log_pi=ws.log_pi, log_std=ws.log_std,
                        tanh_ls=ws.tanh_ls, xa=ws.xa, rng=rng)
        if self._records(step):  # what actor.log() histograms (curl_sac.py:92-93): pre-squash mean and std
            self.actor.outputs['mu'], self.actor.outputs['std'] = ws.a_out[:, :A].clone(), ws.log_std.exp()
        # (the data gradient through the LayerNorms needs the saves too; dropout: the critic twins under tags 5 / 6)
        q_ln = self.critic.twin_ln(*ws.q_ln_saves, drop=self._dropout(rng, dropout_rng)(5))
        self._twin_fwd(ws, self.critic, q_ln, ws.q)
        # backward: Q -> pi -> trunk -> LN -> fc (encoder detached, curl_sac.py:375-376)
        self._twin_bwd(ws, q_ln, self._actor_loss(ws), grads=False)
        if step % self.log_interval == 0:
            L.log('train_actor/loss', ws.scalars[1], step)
            if det:  # (no entropy term, no temperature)
                L.log('train_actor/std', self._policy_std, step)
            else:
                L.log('train_actor/target_entropy', self.target_entropy, step)
                L.log('train_actor/entropy', ws.scalars[3], step)
        # d(loss)/d(pi) = the action columns of dxa summed over the twin, read in place
        F, trunk = aenc.feature_dim, self.actor.trunk
        if det:
            ops.det_head_bwd(None, ws.mu, B, A, ws.a_dout, twin_dxa=ws.dxa, F=F)
        else:
            ops.actor_head_bwd(None, self.log_alpha, 1.0 / B, nz, ws.pi, ws.log_std, ws.tanh_ls, B, A,
                               self.actor.log_std_min, self.actor.log_std_max, ws.a_dout, twin_dxa=ws.dxa, F=F)
        _mlp_bwd(ws.z_a, 0, _Mlp(trunk), _Mlp(trunk, grads=True), 1, B, F, self.hidden_dim, self._actor_out_dim(), ws.a_h1,
                 ws.a_h2, ws.a_dout, ws.a_dh2, ws.a_dh1, ws.dz)
        self._encoder_backward(ws, o, ws.dz, ws.xhat_a, ws.rstd_a, aenc, conv_grads=False)
        self._actor_reduce_and_step(L, step)
        if self.log_param_hist_imgs:
            self.actor.log(L, step)
        if step % self.log_interval == 0 and not det:
            L.log('train_alpha/loss', ws.scalars[2], step)
            L.log('train_alpha/value', ws.scalars[4], step)

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

    def update_cpc(self, obs_anchor, obs_pos, cpc_kwargs, L, step):
        """curl_sac.py:406-423."""
        self._restore_grad_views()
        oa, op_ = _as_ref(obs_anchor), _as_ref(obs_pos)
        B, ws = oa.B, self._ws(oa.B)
        enc, tenc, F = self.critic.encoder, self.critic_target.encoder, self.critic.encoder.feature_dim
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

        W = self.CURL.W
        ops.linear_fwd(ws.z_pos, 0, W, 0, None, 0, ws.WzT, 0, B, F, F)         # (W z_pos^T)^T
        logged = step % self.log_interval == 0  # the mean of the row losses is only needed when it is logged
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
        self._cpc_steps()
        if step % self.log_interval == 0:
            L.log('train/curl_loss', ws.scalars[5], step)
            if self._max_grad_norm is not None:
                L.log('train/curl_grad_norm', self.grad_clip_stats[2, 0], step)

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

    def _clip_torch(self, row, opt):
        """The clipping step of a phase whose optimizer is torch's own (CURLA_TORCH_ADAM=1, a CPU agent): FlatAdam
        clips inside its launches."""
        if self._max_grad_norm is None or isinstance(opt, FlatAdam):
            return
        params = [p for g in opt.param_groups for p in g["params"] if p.grad is not None]
        norm = torch.nn.utils.clip_grad_norm_(params, self._max_grad_norm)
        self.grad_clip_stats[row, 0] = norm
        self.grad_clip_stats[row, 1] = torch.clamp(self._max_grad_norm / (norm + 1e-6), max=1.0)

    def soft_update_targets(self):
        """utils.soft_update_params x3 (curl_sac.py:442-445) as one flat lerp with two rates."""
        lay = self._lay
        (e0, e1), (q0, q1) = lay["enc"], lay["q"]
        assert e1 == q0  # [encoder | Q1 | Q2] are adjacent: one launch, two rates
        ops.soft_update2(self._critic_flat[e0:q1], self._target_flat[e0:q1], e1 - e0, self.encoder_tau, self.critic_tau)

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
        if self.policy_std_schedule is not None:  # (evaluated before the eager / graph route is chosen: std is data)
            self.set_policy_std(_linear_schedule(_check_policy_std_schedule(self.policy_std_schedule), step))
        self._check_n_step(replay_buffer)
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
            self.update_cpc(obs_anchor, obs_pos, cpc_kwargs, L, step)
        self._finish_actor_step()

    def save(self, model_dir, augmentation, step):
        """curl_sac.py:453-456 (same three files, reference tensor layouts)."""
        torch.save(self.CURL.state_dict(), '%s/%s_curl_%s.pt' % (model_dir, augmentation, step))
        torch.save(self.actor.state_dict(), '%s/%s_actor_%s.pt' % (model_dir, augmentation, step))
        torch.save(self.critic.state_dict(), '%s/%s_critic_%s.pt' % (model_dir, augmentation, step))

    def load(self, model_dir, augmentation, step):
        """curl_sac.py:458-465 (same files, same three progress lines on stdout)."""
        self.CURL.load_state_dict(torch.load('%s/%s_curl_%s.pt' % (model_dir, augmentation, step)))
        print('Loaded model %s/%s_curl_%s.pt' % (model_dir, augmentation, step))
        self.actor.load_state_dict(torch.load('%s/%s_actor_%s.pt' % (model_dir, augmentation, step)))
        print('Loaded model %s/%s_actor_%s.pt' % (model_dir, augmentation, step))
        self.critic.load_state_dict(torch.load('%s/%s_critic_%s.pt' % (model_dir, augmentation, step)))
        self.critic_target.load_state_dict(self.critic.state_dict())
        print('Loaded model %s/%s_critic_%s.pt' % (model_dir, augmentation, step))

    # -- full training state (the reference only writes the three state_dicts above and
    #    cannot resume; this adds log_alpha, the target critic, the five Adam states, the RNG streams and the step)
    def _optimizers(self):
        return {"actor": self.actor_optimizer, "critic": self.critic_optimizer, "log_alpha": self.log_alpha_optimizer,
                "encoder": self.encoder_optimizer, "cpc": self.cpc_optimizer}

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

    def save_checkpoint(self, path, step):
        rng = {"torch": torch.get_rng_state(), "numpy": np.random.get_state()}
        if self.device.type == "cuda":
            rng["cuda"] = torch.cuda.get_rng_state(self.device)
        torch.save({
            "format": "curla_amd.checkpoint.v1", "step": int(step),
            "actor": self.actor.state_dict(), "critic": self.critic.state_dict(),
            "critic_target": self.critic_target.state_dict(), "curl": self.CURL.state_dict(),
            "log_alpha": self.log_alpha.detach().cpu(),
            "optimizers": {k: self._convert_opt_state(o, o.state_dict(), True) for k, o in self._optimizers().items()},
            "rng": rng, "critic_dropout": float(self.critic_dropout), "utd_ratio": int(self.utd_ratio),
            "critic_quantiles": int(self.critic_quantiles), "critic_drop_quantiles": int(self.critic_drop_quantiles),
            **({"aug_views": 2} if self.aug_views == 2 else {}),  # (1: the file of an agent without the keyword)
            **({"critic_bins": int(self.critic_bins), "critic_value_range": tuple(float(v) for v in self.critic_value_range),
                "critic_bin_sigma": float(self.critic_bin_sigma)} if self.critic_bins else {}),  # (0: likewise)
            **({"policy": "deterministic", "policy_std": float(self._policy_std),
                "policy_std_clip": self.policy_std_clip, "policy_std_schedule": self.policy_std_schedule}
               if self.policy == "deterministic" else {}),  # (gaussian: likewise)
            **self._reset_checkpoint(), **self._redo_checkpoint(),
        }, path)

    def load_checkpoint(self, path, restore_rng=True):
        """Returns the step the checkpoint was written at."""
        ck = torch.load(path, map_location="cpu", weights_only=False)
        if ck.get("format") != "curla_amd.checkpoint.v1":
            raise ValueError("not a curla_amd checkpoint: %r" % (path,))
        if float(ck.get("critic_dropout", 0.0)) != float(self.critic_dropout):
            warnings.warn("curla_amd: the checkpoint was written with critic_dropout = %r; this agent keeps its own, %r"
                          % (ck.get("critic_dropout", 0.0), self.critic_dropout), RuntimeWarning, stacklevel=2)
        if ck.get("utd_ratio", 1) != self.utd_ratio:  # (a file from before the keyword: 1)
            warnings.warn("curla_amd: the checkpoint was written with utd_ratio = %r; this agent keeps its own, %r"
                          % (ck.get("utd_ratio", 1), self.utd_ratio), RuntimeWarning, stacklevel=2)
        if ck.get("aug_views", 1) != self.aug_views:  # (a file from before the keyword: 1)
            warnings.warn("curla_amd: the checkpoint was written with aug_views = %r; this agent keeps its own, %r"
                          % (ck.get("aug_views", 1), self.aug_views), RuntimeWarning, stacklevel=2)
        self.CURL.load_state_dict(ck["curl"])
        self.actor.load_state_dict(ck["actor"])
        self.critic.load_state_dict(ck["critic"])
        self.critic_target.load_state_dict(ck["critic_target"])
        # (another critic_quantiles has failed above, on the last layers' shapes; the dropped atoms are a number of the
        # loss alone and come from the file)
        if self.critic_quantiles and "critic_drop_quantiles" in ck:
            self.critic_drop_quantiles = _check_drop_quantiles(ck["critic_drop_quantiles"], self.critic_quantiles)
        # (another critic_bins has failed above as well; the range and the smoothing are numbers of the loss alone)
        if self.critic_bins and "critic_value_range" in ck:
            self.critic_value_range = _check_value_range(ck["critic_value_range"])
            self.critic_bin_sigma = _check_bin_sigma(ck.get("critic_bin_sigma", self.critic_bin_sigma))
            self._hlg_params()
        # (a checkpoint of the other policy has failed above, on the size of actor.trunk.4)
        if self.policy == "deterministic" and ck.get("policy") == "deterministic":
            self.policy_std_clip = _check_policy_std_clip(ck["policy_std_clip"])
            self.policy_std_schedule = _check_policy_std_schedule(ck["policy_std_schedule"])
            self.set_policy_std(ck["policy_std"])
        with torch.no_grad():
            self.log_alpha.copy_(ck["log_alpha"])
        for k, o in self._optimizers().items():
            o.load_state_dict(self._convert_opt_state(o, ck["optimizers"][k], False))
        if restore_rng:
            torch.set_rng_state(ck["rng"]["torch"])
            np.random.set_state(ck["rng"]["numpy"])
            if self.device.type == "cuda" and "cuda" in ck["rng"]:
                torch.cuda.set_rng_state(ck["rng"]["cuda"], self.device)
        self._load_reset_checkpoint(ck)
        self._load_redo_checkpoint(ck)
        self._drop_encoder_caches()
        # captured graphs hold the addresses of log_alpha's Adam moments, which load_state_dict has just replaced
        self._drop_graphs()
        return ck["step"]

