"""Actor / QFunction / Critic / CURL with the reference's API (curl_sac.py:38-222), and their argument checks."""
import numpy as np
import torch
import torch.nn as nn

from . import autograd, ops
from .encoder import CNNEncoder
from .mlp import _Mlp, _MlpLn, _linears, _mlp_fwd

LOG_FREQ = 25_000


def weight_init(m):
    """The reference's initialisation (curl_sac.py:38-54), applied with ``module.apply``: Linear weights orthogonal
    with zero bias; Conv2d / ConvTranspose2d "delta-orthogonal" (arXiv:1806.05393) -- every tap zero except the
    centre one, which is an orthogonal (out x in) matrix with the ReLU gain -- and zero bias.  The draws come from
    torch's global generator in module order, so a seeded construction reproduces the reference's parameters."""
    if isinstance(m, nn.Linear):
        nn.init.orthogonal_(m.weight.data)
        if m.bias is not None:
            m.bias.data.zero_()
        return
    if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
        kh, kw = m.weight.shape[2:]
        assert kh == kw, "square kernels only"
        m.weight.data.zero_()
        if m.bias is not None:
            m.bias.data.zero_()
        centre = kh // 2
        nn.init.orthogonal_(m.weight.data[:, :, centre, centre], nn.init.calculate_gain('relu'))


def _check_policy_std(v):
    """The deterministic policy's standard deviation: a finite float > 0."""
    if isinstance(v, (bool, str)) or not isinstance(v, (int, float, np.integer, np.floating)) or \
            not np.isfinite(v) or v <= 0:
        raise ValueError("policy_std: %r is not a finite number > 0" % (v,))
    return float(v)


def _check_policy_std_clip(c):
    """The clip of the deterministic policy's scaled noise inside an update: a finite float >= 0, or None (no clip)."""
    if c is None:
        return None
    if isinstance(c, (bool, str)) or not isinstance(c, (int, float, np.integer, np.floating)) or \
            not np.isfinite(c) or c < 0:
        raise ValueError("policy_std_clip: %r is not a finite number >= 0 or None" % (c,))
    return float(c)


class _ActorType(type):
    """``Actor(..., deterministic=True)``: a keyword of the class call, as ``QFunction(..., quantiles=M)`` is;
    ``Actor.__init__`` keeps its parameter list.  The actor is built as without it and its last Linear is then replaced
    in place by a hidden -> A one (the key stays trunk.4), drawn from a fork of torch's generator: every other tensor a
    seed produces, and the generator's state afterwards, are the Gaussian actor's."""

    def __call__(cls, *args, deterministic=False, **kwargs):
        actor = super().__call__(*args, **kwargs)
        if deterministic:
            actor.deterministic = True
            _widen_last_layers([actor.trunk], actor.action_dim, weight_init)
            actor.std = torch.full((1,), 0.2, dtype=torch.float32)  # (no registered buffer: the state-dict keys stay)
            actor.std_clip = 0.3
        return actor


class Actor(nn.Module, metaclass=_ActorType):
    """MLP actor network (curl_sac.py:57-121).  ``Actor(..., deterministic=True)`` (a keyword of the class call; DESIGN.md
    7m): DrQ-v2's deterministic policy -- the trunk outputs the A pre-squash means alone, ``forward`` returns
    ``mu = tanh(o)``, ``pi = clamp(mu + std * noise, -lim, lim)`` (no noise clip, as DrQ-v2 acts), ``log_pi`` zeros and
    ``log_std`` filled with log(std).  ``std`` is a one-element float32 tensor read by the kernels on the device (edit it
    in place, or through CurlSacAgent.set_policy_std); ``std_clip`` is what the agent's update phases clip the scaled noise
    to (None: no clip)."""

    deterministic = False

    def __init__(self, obs_shape, action_shape, hidden_dim, encoder_feature_dim, log_std_min, log_std_max,
                 num_layers, num_filters):
        super().__init__()
        self.encoder = CNNEncoder(obs_shape, encoder_feature_dim, num_layers, num_filters, output_logits=True)
        self.log_std_min = log_std_min
        self.log_std_max = log_std_max
        self.action_dim = action_shape[0]
        self.hidden_dim = hidden_dim
        self.trunk = nn.Sequential(
            nn.Linear(self.encoder.feature_dim, hidden_dim), nn.ReLU(),
            nn.Linear(hidden_dim, hidden_dim), nn.ReLU(),
            nn.Linear(hidden_dim, 2 * action_shape[0])
        )
        self.outputs = dict()
        self.apply(weight_init)

    def forward(self, obs, compute_pi=True, compute_log_pi=True, detach_encoder=False, noise=None):
        """Forward on the HIP kernels; same return tuple as the reference (mu, pi, log_pi, log_std) with pi/log_pi
        None when not asked for.  ``noise`` replaces torch.randn_like (curl_sac.py:97) and is a constant.
        Differentiable (autograd.ActorFn) when grad mode is on and the features or a trunk parameter require grad."""
        z = self.encoder(obs, detach=detach_encoder)
        if autograd.wants_graph(z, *self.trunk.parameters()):
            return autograd.actor_forward(self, z, compute_pi, compute_log_pi, noise)
        B, A, H, F = z.shape[0], self.action_dim, self.hidden_dim, self.encoder.feature_dim
        dev = z.device
        if self.deterministic:
            h1, h2, out = (torch.empty(s, device=dev) for s in ((B, H), (B, H), (B, A)))
            mu, log_std = torch.empty((B, A), device=dev), torch.empty((B, A), device=dev)
            pi = log_pi = None
            if compute_pi:
                if noise is None:
                    noise = torch.randn((B, A), device=dev)
                pi = torch.empty((B, A), device=dev)
                log_pi = torch.empty((B, 1), device=dev) if compute_log_pi else None
            _mlp_fwd(z, 0, _Mlp(self.trunk), 1, B, F, H, A, h1, h2, out,
                     head=(noise if compute_pi else None, self.std_on(dev), None,
                           dict(mu=mu, pi=pi, log_pi=log_pi, log_std=log_std), "det"))
            self.outputs['mu'] = out  # the pre-squash mean
            self.outputs['std'] = log_std.exp()
            return mu, pi, log_pi, log_std
        h1 = torch.empty((B, H), device=dev)
        h2 = torch.empty((B, H), device=dev)
        out = torch.empty((B, 2 * A), device=dev)
        mu = torch.empty((B, A), device=dev)
        log_std = torch.empty((B, A), device=dev)
        pi = log_pi = None
        if compute_pi:
            if noise is None:
                noise = torch.randn((B, A), device=dev)
            pi = torch.empty((B, A), device=dev)
            log_pi = torch.empty((B, 1), device=dev) if compute_log_pi else None
        _mlp_fwd(z, 0, _Mlp(self.trunk), 1, B, F, H, 2 * A, h1, h2, out,
                 head=(noise if compute_pi else None, self.log_std_min, self.log_std_max,
                       dict(mu=mu, pi=pi, log_pi=log_pi, log_std=log_std)))
        self.outputs['mu'] = out[:, :A]  # the pre-squash mean, as the reference records it (curl_sac.py:92)
        self.outputs['std'] = log_std.exp()
        return mu, pi, log_pi, log_std

    def std_on(self, device):
        """The deterministic actor's ``std`` on ``device`` (moved there once: the kernels read it from device memory)."""
        if self.std.device != torch.device(device) and not (self.std.is_cuda and torch.device(device).type == "cuda"
                                                            and torch.device(device).index is None):
            self.std = self.std.to(device)
        return self.std

    def log(self, L, step, log_freq=LOG_FREQ):
        """Histograms of the recorded outputs and of the three trunk layers, every ``log_freq`` steps
        (curl_sac.py:112-121; same keys)."""
        if step % log_freq:
            return
        for name, value in self.outputs.items():
            L.log_histogram('train_actor/%s_hist' % name, value, step)
        for n, layer in enumerate(_linears(self.trunk), start=1):
            L.log_param('train_actor/fc%d' % n, layer, step)


def _check_int(v, lo, hi, message):
    """``v`` as an ``int`` in lo .. hi (``hi`` None: no upper bound); ValueError(message) for anything else -- a bool, a
    float or a string is not an int."""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo or (hi is not None and v > hi):
        raise ValueError(message)
    return int(v)


def _check_quantiles(m):
    """The quantile atoms per Q function: 0 (off) or an ``int`` in 1 .. ops.TQC_MAX (a bool, a float or a string is not
    one)."""
    return _check_int(m, 0, ops.TQC_MAX, "critic quantiles: %r is not an int in 0 .. %d (0: off; the %d pooled atoms "
                      "of a row are one wave's lanes)" % (m, ops.TQC_MAX, 2 * ops.TQC_MAX))


def _check_drop_quantiles(d, m):
    """The atoms dropped per network, ``0 <= d < M``; only with quantiles on."""
    d = _check_int(d, 0, None, "critic_drop_quantiles: %r is not an int >= 0" % (d,))
    if d and not m:
        raise ValueError("critic_drop_quantiles = %d needs critic_quantiles > 0" % d)
    if m and d >= m:
        raise ValueError("critic_drop_quantiles = %d drops every one of the %d atoms (0 <= d < M)" % (d, m))
    return d


def _check_bins(m):
    """The bins of the categorical HL-Gauss critic: 0 (off) or an ``int`` in 2 .. ops.HLG_MAX."""
    m = _check_int(m, 0, ops.HLG_MAX, "critic bins: %r is not an int, 0 (off) or in 2 .. %d" % (m, ops.HLG_MAX))
    if m == 1:
        raise ValueError("critic bins: 1 is not 0 (off) or in 2 .. %d" % ops.HLG_MAX)
    return m


def _check_width(quantiles, bins):
    """(quantiles, bins) of a Q function's last layer, checked; the two are exclusive."""
    quantiles, bins = _check_quantiles(quantiles), _check_bins(bins)
    if quantiles and bins:
        raise ValueError("critic quantiles = %d and critic bins = %d: a Q function's last layer is one or the other"
                         % (quantiles, bins))
    return quantiles, bins


def _check_value_range(value_range):
    """``(v_min, v_max)`` of the HL-Gauss critic's bins as two floats: finite, v_min < v_max."""
    try:
        v_min, v_max = (float(v) for v in value_range)
    except (TypeError, ValueError):
        raise ValueError("critic_value_range: %r is not a pair (v_min, v_max) of numbers" % (value_range,)) from None
    if not (np.isfinite(v_min) and np.isfinite(v_max) and v_min < v_max):
        raise ValueError("critic_value_range: (%r, %r) is not finite with v_min < v_max" % (v_min, v_max))
    return v_min, v_max


def _check_bin_sigma(s):
    """The HL-Gauss smoothing's standard deviation in bin widths: a finite number > 0."""
    if isinstance(s, (bool, str)) or not isinstance(s, (int, float, np.integer, np.floating)) or \
            not np.isfinite(s) or s <= 0:
        raise ValueError("critic_bin_sigma: %r is not a finite number > 0" % (s,))
    return float(s)


def _widen_last_layers(trunks, m, init=None):
    """Replace the last Linear (hidden -> 1) of each trunk by a hidden -> ``m`` one, ``init`` applied to it.  The new
    tensors' draws are taken from a fork of torch's generator, which is put back afterwards: everything else a seed
    produces -- the layers before, the other networks, CURL.W -- comes out as without quantiles."""
    with torch.random.fork_rng(devices=[]):
        for trunk in trunks:
            wide = nn.Linear(trunk[-1].in_features, m)
            if init is not None:
                init(wide)
            trunk[-1] = wide  # (same position: the state-dict keys stay trunk.4 / trunk.6)


class _QFunctionType(type):
    """``QFunction(..., quantiles=M)``: a keyword of the class call, as ``Critic(..., dropout=p)`` is (_CriticType);
    ``QFunction.__init__`` keeps its parameter list with ``dropout`` last.  ``bins=M`` beside it, exclusive with it."""

    def __call__(cls, *args, quantiles=0, bins=0, **kwargs):
        quantiles, bins = _check_width(quantiles, bins)
        q = super().__call__(*args, **kwargs)
        q.quantiles = quantiles
        if bins:
            q.bins = bins
        if quantiles or bins:
            _widen_last_layers([q.trunk], quantiles or bins)
        return q


class QFunction(nn.Module, metaclass=_QFunctionType):
    """MLP for q-function (curl_sac.py:124-139); parameter container.  ``layer_norm``: an ``nn.LayerNorm(hidden_dim)``
    between each hidden Linear and its ReLU (the Linears are then trunk.0 / .3 / .6, the LayerNorms trunk.1 / .4).
    ``dropout``: DroQ's dropout probability in front of each LayerNorm -- an attribute, no module of the trunk.
    ``QFunction(..., quantiles=M)`` (a keyword of the class call; 0: off): the last Linear has M rows, one per quantile
    atom.  ``QFunction(..., bins=M)`` (likewise; not with quantiles): M rows, the logits over the HL-Gauss critic's bins."""

    quantiles = 0
    bins = 0

    def __init__(self, obs_dim, action_dim, hidden_dim, layer_norm=False, dropout=0.0):
        super().__init__()
        _check_layer_norm_width(layer_norm, hidden_dim)
        self.dropout = _check_dropout(dropout, layer_norm)
        norm = (lambda: [nn.LayerNorm(hidden_dim)]) if layer_norm else (lambda: [])
        self.trunk = nn.Sequential(
            nn.Linear(obs_dim + action_dim, hidden_dim), *norm(), nn.ReLU(),
            nn.Linear(hidden_dim, hidden_dim), *norm(), nn.ReLU(),
            nn.Linear(hidden_dim, 1)
        )


def _check_layer_norm_width(layer_norm, hidden_dim):
    if layer_norm and hidden_dim > ops.MLP_LN_MAX:
        raise ValueError("critic LayerNorm: hidden_dim = %d is wider than the %d features the LayerNorm kernels take "
                         "(one wave per row)" % (hidden_dim, ops.MLP_LN_MAX))


def _check_dropout(p, layer_norm):
    """The critics' dropout probability as a float: 0 <= p < 1, and only in front of a LayerNorm (dropout without the
    normalisation behind it is the configuration DroQ shows to be harmful; it is not offered)."""
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError("critic dropout: p = %r is not in [0, 1)" % (p,))
    if p > 0.0 and not layer_norm:
        raise ValueError("critic dropout needs the critics' LayerNorm (critic_layer_norm=True / layer_norm=True)")
    return p


def _device_generator(device):
    device = torch.device(device)
    torch.cuda.init()  # (the generators exist once the runtime is up; a dropout agent may be the process's first use of it)
    return torch.cuda.default_generators[device.index if device.index is not None else torch.cuda.current_device()]


def _reserve_dropout_counter(device):
    """(seed, counter) of one pass's dropout masks, taken from ``device``'s default torch generator, whose offset moves
    on by 4 (one Philox counter): torch.manual_seed, get_rng_state / set_rng_state (checkpoints) and the per-rank
    seeds keep their meaning.  A CPU agent launches nothing (the trace hook's launch lists): position 0 of torch's
    seed."""
    if torch.device(device).type != "cuda":
        return torch.initial_seed(), 0
    gen = _device_generator(device)
    off = gen.get_offset()
    gen.set_offset(off + 4)
    return gen.initial_seed(), off // 4


class _CriticType(type):
    """``Critic(..., dropout=p)``: the class call takes the keyword, as CurlSacAgent's takes its own (_AgentType), and
    ``Critic.__init__`` keeps its parameter list with ``layer_norm`` last.  ``Critic(..., quantiles=M)`` likewise: the
    critic is built as without it and the Q functions' last layers are then replaced by M-row ones, initialised like
    every other Linear (weight_init).  ``Critic(..., bins=M, value_range=(v_min, v_max))``: the same M-row layers as the
    logits of the HL-Gauss critic, exclusive with quantiles (bins = 0: an instance without either attribute; the range
    may be left out and set later)."""

    def __call__(cls, *args, dropout=0.0, quantiles=0, bins=0, value_range=None, **kwargs):
        quantiles, bins = _check_width(quantiles, bins)
        if value_range is not None:
            if not bins:
                raise ValueError("Critic(value_range=...) needs bins > 0")
            value_range = _check_value_range(value_range)
        critic = super().__call__(*args, **kwargs)
        critic.dropout = critic.Q1.dropout = critic.Q2.dropout = _check_dropout(dropout, critic.layer_norm)
        critic.quantiles = critic.Q1.quantiles = critic.Q2.quantiles = quantiles
        if bins:
            critic.bins = critic.Q1.bins = critic.Q2.bins = bins
            critic.value_range = value_range
        if quantiles or bins:
            _widen_last_layers([critic.Q1.trunk, critic.Q2.trunk], quantiles or bins, weight_init)
        return critic


class Critic(nn.Module, metaclass=_CriticType):
    """Critic network, employs two Q-functions (curl_sac.py:142-180).  ``layer_norm``: QFunction's; so is
    ``Critic(..., dropout=p)``, a keyword of the class call.  ``forward`` drops in training mode only
    (``critic.eval()``: the deterministic Q).  ``Critic(..., quantiles=M)`` (0: off): each Q function outputs M quantile
    atoms and ``forward`` returns ``q1, q2`` of shape [B, M].  ``Critic(..., bins=M, value_range=(v_min, v_max))`` (0:
    off; not with quantiles): the categorical HL-Gauss critic -- each Q function outputs M logits over the
    bins of the value range, ``forward`` returns the two [B, M] logit tensors, ``expected(logits)`` turns them into Q
    values.  ``value_range`` is an attribute that may be edited (the agent keeps its critics' in step with its own)."""

    dropout = 0.0
    quantiles = 0
    bins = 0
    value_range = None

    @property
    def out_dim(self):
        """The width of a Q function's last layer: its quantile atoms, its bins' logits, or the one Q value."""
        return self.quantiles or self.bins or 1

    def bin_centres(self):
        """c_j = v_min + (j + 1/2) w, w = (v_max - v_min) / M: float32 [M], on the critic's device."""
        if not self.bins:
            raise RuntimeError("Critic.bin_centres: this critic has no bins (Critic(..., bins=M))")
        if self.value_range is None:
            raise RuntimeError("Critic.bin_centres: set critic.value_range = (v_min, v_max) first")
        v_min, v_max = _check_value_range(self.value_range)
        w = (v_max - v_min) / self.bins
        dev = self.Q1.trunk[-1].weight.device
        return (v_min + (torch.arange(self.bins, dtype=torch.float64) + 0.5) * w).to(torch.float32).to(dev)

    def expected(self, logits):
        """Q = sum_j softmax(logits)_j c_j of [B, M] logits, as [B, 1]: a plain torch expression, differentiable by
        torch (what an evaluation script or a user's own loss turns ``forward``'s logits into Q values with)."""
        return (torch.softmax(logits, dim=-1) * self.bin_centres().to(logits.device, logits.dtype)).sum(-1, keepdim=True)

    def __init__(self, obs_shape, action_shape, hidden_dim, encoder_feature_dim, num_layers, num_filters,
                 layer_norm=False):
        super().__init__()
        _check_layer_norm_width(layer_norm, hidden_dim)
        self.encoder = CNNEncoder(obs_shape, encoder_feature_dim, num_layers, num_filters, output_logits=True)
        self.Q1 = QFunction(self.encoder.feature_dim, action_shape[0], hidden_dim, layer_norm)
        self.Q2 = QFunction(self.encoder.feature_dim, action_shape[0], hidden_dim, layer_norm)
        self.action_dim = action_shape[0]
        self.hidden_dim = hidden_dim
        self.layer_norm = bool(layer_norm)
        self.outputs = dict()
        self.twin_stride = None  # floats between Q1 and Q2 tensors once flattened by the agent
        self.apply(weight_init)

    def twin(self, grads=False):
        if self.twin_stride is None:
            raise RuntimeError("Critic parameters are not in the flat twin layout (constructed outside CurlSacAgent)")
        return _Mlp(self.Q1.trunk, self.twin_stride, grads)

    def twin_ln(self, xhat=None, rstd=None, grads=False, partial=None, save_first=0, drop=None):
        """The ``ln=`` argument of _mlp_fwd / _mlp_bwd for ``twin()``: None without LayerNorm.  ``xhat`` / ``rstd``:
        a pair of buffers each, one per hidden layer; ``grads``: the backward fills the LayerNorm tensors' .grad;
        ``drop`` = (p, rng, tag) or None: this pass's dropout (_MlpLn)."""
        if not self.layer_norm:
            return None
        ln = _MlpLn(self.Q1.trunk, xhat, rstd, partial=partial, save_first=save_first, drop=drop)
        if grads:
            ln.dg, ln.db = [p.grad for p in ln.g], [p.grad for p in ln.b]
        return ln

    DROP_TAG_FORWARD = 7  # the tags of the dropout masks: 1 + 2 * pass + layer, a forward() call is pass 3

    def forward(self, obs, action, detach_encoder=False, dropout_rng=None):
        """``dropout_rng`` = (seed, counter): the stream position of a training-mode dropout critic's masks (tags 7 / 8);
        None reserves one counter from the device's torch generator per call."""
        assert obs.size(0) == action.size(0)  # curl_sac.py:136
        z = self.encoder(obs, detach=detach_encoder)
        drop = None
        if self.dropout > 0 and self.training:
            _check_dropout(self.dropout, self.layer_norm)
            drop = (self.dropout, dropout_rng or _reserve_dropout_counter(z.device), self.DROP_TAG_FORWARD)
        if autograd.wants_graph(z, action, *self.Q1.parameters(), *self.Q2.parameters()):
            q1, q2 = autograd.critic_forward(self, z, action, drop)  # (differentiable: autograd.CriticFn)
            self.outputs['q1'], self.outputs['q2'] = q1.detach(), q2.detach()
            return q1, q2
        B, A, H, F = z.shape[0], self.action_dim, self.hidden_dim, self.encoder.feature_dim
        dev = z.device
        xa = torch.empty((B, F + A), device=dev)
        ops.concat(z, action.contiguous().float(), B, F, A, xa)
        h1 = torch.empty((2, B, H), device=dev)
        h2 = torch.empty((2, B, H), device=dev)
        q = torch.empty((2, B, self.out_dim), device=dev)
        _mlp_fwd(xa, 0, self.twin(), 2, B, F + A, H, self.out_dim, h1, h2, q, ln=self.twin_ln(drop=drop))
        self.outputs['q1'], self.outputs['q2'] = q[0], q[1]
        return q[0], q[1]

    def log(self, L, step, log_freq=LOG_FREQ):
        """Histograms of the recorded Q values and of both Q trunks, every ``log_freq`` steps
        (curl_sac.py:171-180; same keys)."""
        if step % log_freq:
            return
        for name, value in self.outputs.items():
            L.log_histogram('train_critic/%s_hist' % name, value, step)
        for layer in range(3):  # (the three Linears; a LayerNorm critic's LayerNorms are not histogrammed)
            for tag, q in (('q1', self.Q1), ('q2', self.Q2)):
                L.log_param('train_critic/%s_fc%d' % (tag, layer), _linears(q.trunk)[layer], step)


class CURL(nn.Module):
    """CURL head (curl_sac.py:183-222)."""

    def __init__(self, obs_shape, z_dim, critic, critic_target, output_type="continuous"):
        super().__init__()
        self.encoder = critic.encoder
        self.encoder_target = critic_target.encoder
        self.W = nn.Parameter(torch.rand(z_dim, z_dim))
        self.output_type = output_type

    def encode(self, x, detach=False, ema=False):
        """curl_sac.py:196-209: ``ema`` runs the target encoder without grad, ``detach`` detaches the result."""
        if ema:
            with torch.no_grad():
                z_out = self.encoder_target(x)
        else:
            z_out = self.encoder(x)
        return z_out.detach() if detach else z_out

    def compute_logits(self, z_a, z_pos):
        """(B,B) logits z_a (W z_pos^T) minus the row max (curl_sac.py:211-222),
        both products on the MFMA GEMM; differentiable through both (autograd.CurlLogitsFn) when grad mode is on and
        an input or W requires grad."""
        if autograd.wants_graph(z_a, z_pos, self.W):
            logits = autograd.CurlLogitsFn.apply(z_a.contiguous(), z_pos.contiguous(), self.W)
            return logits - torch.max(logits, 1)[0][:, None]
        B, F = z_a.shape
        WzT = torch.empty((B, F), device=z_a.device)
        logits = torch.empty((B, B), device=z_a.device)
        ops.linear_fwd(z_pos.contiguous(), 0, self.W, 0, None, 0, WzT, 0, B, F, F)
        ops.linear_fwd(z_a.contiguous(), 0, WzT, 0, None, 0, logits, 0, B, B, F)
        return logits - torch.max(logits, 1)[0][:, None]
