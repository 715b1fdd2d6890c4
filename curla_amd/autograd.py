"""Autograd through the HIP encoder, actor, critic and CURL head.

The modules' ``forward`` methods run the same kernel launches whether or not autograd records them; when
``torch.is_grad_enabled()`` and some input or parameter of the call requires grad, those launches run inside a
``torch.autograd.Function`` defined here, whose backward is the matching HIP backward launches:

* encoder: LayerNorm backward, fc backward (data gradient ReLU-masked by the last conv activation), one
  ``conv_s1_bwd_slabs`` per stride-1 layer, ``conv1_wgrad_slabs``, one ``wgrad_reduce_multi``, and for a float
  observation that requires grad ``conv1_dgrad`` (csrc/conv1_dgrad.h);
* actor: ``policy_head_bwd`` (the squashed-Gaussian head for any subset of its four outputs) and the trunk's
  ``_mlp_bwd``;
* critic: the twin Q MLPs' ``_mlp_bwd`` in their flat twin layout and ``split_sum`` into d z and d action;
* CURL logits: ``linear_dx`` / ``linear_dw`` through both products.

Each graph-building forward keeps its activations in buffers of its own (never ``CNNEncoder.workspace``), so any
number of forwards may precede a backward.  Forward values are those of the inference path bit for bit: same
kernels, same options; the saved LayerNorm ``xhat`` / ``rstd`` and the head's ``tanh_ls`` are side outputs of the
same launches.  Every backward is once-differentiable: a double backward raises at once.  Parameter gradients come back as
fresh tensors; ``CurlSacAgent`` moves them into its flat gradient buffers (curl_sac.py, ``_install_grad_views``).
"""
import types

import torch
from torch.autograd.function import once_differentiable

from . import ops
from .mlp import _Mlp, _linears, _mlp_bwd, _mlp_fwd

F32 = torch.float32


def once_differentiable_hip(backward):
    """torch's once_differentiable, and a clear error at the first backward that would build a graph of its own
    (``create_graph=True``): the HIP backward launches have no derivative."""
    inner = once_differentiable(backward)

    def wrapper(ctx, *grads):
        if torch.is_grad_enabled():
            raise RuntimeError("curla_amd: double backward (create_graph=True) is not supported -- the HIP backward "
                               "kernels of the encoder, actor, critic and CURL head are once-differentiable")
        return inner(ctx, *grads)
    return wrapper


def wants_graph(*tensors):
    """Build an autograd graph for this call?  Grad mode on and some tensor among ``tensors`` requires grad."""
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors)


def _empty(*shape, like):
    return torch.empty(shape, device=like.device, dtype=F32)


def _contig(t):
    return None if t is None else t.contiguous()


# ------------------------------------------------------------------------------------------------------------ encoder
def encoder_params(enc):
    """The encoder's Parameters in the order the Functions take them: conv w / b per layer, fc w / b, ln w / b."""
    ps = []
    for m in enc.convs:
        ps += [m.weight, m.bias]
    return ps + [enc.fc.weight, enc.fc.bias, enc.ln.weight, enc.ln.bias]


def _conv_stack_forward(enc, ref):
    acts = [torch.empty((ref.B, h, w, enc.num_filters), device=enc.fc.weight.device, dtype=F32)
            for (h, w) in enc.layer_hw[1:]]
    enc.conv_forward(ref, acts)
    return acts


def _conv_stack_backward(enc, ref, acts, g, want_params, want_obs):
    """From ``g`` = d loss / d (pre-activation of the last conv layer), NHWC: the conv weight / bias gradients (fresh
    tensors, or None when ``want_params`` is False) and, for a float NCHW observation, d loss / d obs."""
    L, dev = enc.num_layers, g.device
    grads = [None] * (2 * L)
    jobs = []
    for layer in range(L, 1, -1):  # layer l: input acts[l-2], output acts[l-1]
        conv = enc.convs[layer - 1]
        gin = torch.empty_like(acts[layer - 2])
        ws = torch.empty(ops.wgrad_workspace_floats(enc.num_filters), device=dev, dtype=F32)
        n = ops.conv_s1_bwd_slabs(acts[layer - 2], g, conv.weight, gin, ws)
        if want_params:
            dw, db = torch.empty_like(conv.weight), torch.empty_like(conv.bias)
            jobs.append((ws, n, dw, db))
            grads[2 * (layer - 1)], grads[2 * (layer - 1) + 1] = dw, db
        g = gin
    if want_params:
        ws = torch.empty(ops.wgrad_workspace_floats(ref.C), device=dev, dtype=F32)
        n = ops.conv1_wgrad_slabs(ref, g, ws, enc.num_filters)
        dw, db = torch.empty_like(enc.convs[0].weight), torch.empty_like(enc.convs[0].bias)
        jobs.append((ws, n, dw, db))
        grads[0], grads[1] = dw, db
        for i in range(0, len(jobs), 8):
            ops.wgrad_reduce_multi(jobs[i:i + 8])
    dobs = None
    if want_obs:
        dobs = torch.empty((ref.B, ref.C, ref.Hc, ref.Wc), device=dev, dtype=F32)
        ops.conv1_dgrad(g, enc.convs[0].weight, dobs)
    return grads, dobs


class EncoderFn(torch.autograd.Function):
    """z = LN(fc(conv stack(obs)))  (+ tanh unless output_logits): encoder.py:77-110 on the kernels."""

    @staticmethod
    def forward(ctx, enc, ref, detach, keep, obs, *params):
        ctx.set_materialize_grads(False)
        B, F = ref.B, enc.feature_dim
        acts = _conv_stack_forward(enc, ref)
        z = _empty(B, F, like=acts[0])
        xhat, rstd = _empty(B, F, like=z), _empty(B, like=z)
        fc_out = torch.empty_like(z) if enc.record_outputs else None
        enc.head_forward(acts[-1].view(B, -1), z, fc_out=fc_out, xhat=xhat, rstd=rstd)
        keep.update(acts=acts, fc_out=fc_out)
        ctx.enc, ctx.ref, ctx.detach, ctx.acts, ctx.xhat, ctx.rstd = enc, ref, detach, acts, xhat, rstd
        ctx.save_for_backward(z)
        return z

    @staticmethod
    @once_differentiable_hip
    def backward(ctx, dz):
        enc, ref, acts = ctx.enc, ctx.ref, ctx.acts
        nconv = 2 * enc.num_layers
        need = ctx.needs_input_grad
        none = (None,) * (5 + nconv + 4)
        if dz is None:
            return none
        (z,) = ctx.saved_tensors
        B, F, K = ref.B, enc.feature_dim, enc.flat_dim
        dz = dz.contiguous()
        if not enc.output_logits:  # z = tanh(LayerNorm(...)): through the tanh first
            dz = dz * (1.0 - z * z)
        dfc = _empty(B, F, like=dz)
        dgamma, dbeta = torch.empty_like(enc.ln.weight), torch.empty_like(enc.ln.bias)
        dbias = torch.empty_like(enc.fc.bias)
        ops.ln_bwd(dz, ctx.xhat, ctx.rstd, enc.ln.weight, B, F, dfc, dgamma=dgamma, dbeta=dbeta, dbias_in=dbias)
        want_params = any(need[5:5 + nconv])
        want_obs = need[4] and ref.is_u8 == 0
        into_convs = not ctx.detach and (want_params or want_obs)
        h = acts[-1]
        dW = torch.empty_like(enc.fc.weight)
        g = torch.empty_like(h) if into_convs else None
        if ops.fc_bwd_streams(F, K):
            if into_convs:  # weight gradient and the data gradient into the conv stack (ReLU-masked) in one launch
                ops.fc_bwd(dfc, enc.fc.weight, h, g, dW, B, F, K)
            else:
                ops.fc_dw(dfc, h, dW, B, F, K)
        else:
            ops.linear_dw(dfc, 0, h, 0, dW, 0, B, F, K)
            if into_convs:
                ops.linear_dx(dfc, 0, enc.fc.weight, 0, g, 0, B, F, K, mask=h)
        conv_grads, dobs = [None] * nconv, None
        if into_convs:
            conv_grads, dobs = _conv_stack_backward(enc, ref, acts, g, want_params, want_obs)
        return (None, None, None, None, dobs, *conv_grads, dW, dbias, dgamma, dbeta)


def encoder_forward(enc, obs, detach):
    """The differentiable ``CNNEncoder.forward``.  ``obs``: float NCHW in [0,255] (differentiable) or an ObsRef
    (never receives a gradient)."""
    if isinstance(obs, ops.ObsRef):
        ref, x = obs, None
    else:
        x = obs.contiguous().float()
        ref = ops.ObsRef.from_tensor(x)
    keep = {}
    z = EncoderFn.apply(enc, ref, bool(detach), keep, x, *encoder_params(enc))
    if enc.record_outputs:
        enc._record(keep["acts"])
        enc.outputs["fc"] = keep["fc_out"]
        enc.outputs["ln" if enc.output_logits else "tanh"] = z.detach()
    return z


class ConvStackFn(torch.autograd.Function):
    """The last conv activation [B, H, W, F] (NHWC, after its ReLU) of the conv stack (encoder.py:77-88)."""

    @staticmethod
    def forward(ctx, enc, ref, keep, obs, *conv_params):
        ctx.set_materialize_grads(False)
        acts = _conv_stack_forward(enc, ref)
        keep.update(acts=acts)
        ctx.enc, ctx.ref, ctx.acts = enc, ref, acts
        return acts[-1]

    @staticmethod
    @once_differentiable_hip
    def backward(ctx, dh):
        enc, ref = ctx.enc, ctx.ref
        nconv = 2 * enc.num_layers
        need = ctx.needs_input_grad
        want_params, want_obs = any(need[4:4 + nconv]), need[3] and ref.is_u8 == 0
        if dh is None or not (want_params or want_obs):
            return (None,) * (4 + nconv)
        # d / d(pre-activation): the ReLU's mask (this path is off the learner's: forward_conv only)
        g = torch.where(ctx.acts[-1] > 0, dh, torch.zeros((), device=dh.device, dtype=dh.dtype)).contiguous()
        conv_grads, dobs = _conv_stack_backward(enc, ref, ctx.acts, g, want_params, want_obs)
        return (None, None, None, dobs, *conv_grads)


class NhwcToNchwFn(torch.autograd.Function):
    """ops.nhwc_to_nchw (a copy); its backward is the inverse layout shuffle."""

    @staticmethod
    def forward(ctx, h):
        out = torch.empty((h.shape[0], h.shape[3], h.shape[1], h.shape[2]), device=h.device, dtype=h.dtype)
        ops.nhwc_to_nchw(h, out)
        return out

    @staticmethod
    @once_differentiable_hip
    def backward(ctx, d):
        return d.permute(0, 2, 3, 1).contiguous()


def forward_conv(enc, obs):
    """The differentiable ``CNNEncoder.forward_conv``: flattened conv features in (c, y, x) order."""
    if isinstance(obs, ops.ObsRef):
        ref, x = obs, None
    else:
        x = obs.contiguous().float()
        ref = ops.ObsRef.from_tensor(x)
    keep = {}
    h = ConvStackFn.apply(enc, ref, keep, x, *encoder_params(enc)[:2 * enc.num_layers])
    if enc.record_outputs:
        enc._record(keep["acts"])
    return NhwcToNchwFn.apply(h).view(ref.B, -1)


# ------------------------------------------------------------------------------------------------------------ actor
def _grad_mlp(layers, stride=0, base=None, span=None):
    """Fresh gradient tensors laid out like the MLP's parameters (one zeroed buffer; twins ``stride`` floats apart).
    ``span``: every module of the MLP with parameters, where ``layers`` (its Linears) are not all of them."""
    if base is None:
        ps = [t for m in (span or layers) for t in (m.weight, m.bias)]
        p0 = min(p.data_ptr() for p in ps)
        span = max(p.data_ptr() + 4 * p.numel() for p in ps) - p0
        n = span // 4 + stride
        base = (torch.zeros(n, device=ps[0].device, dtype=F32), p0)
    buf, p0 = base

    def view(p, twin=0):
        off = (p.data_ptr() - p0) // 4 + twin * stride
        return buf[off:off + p.numel()].view(p.shape)
    G = types.SimpleNamespace(W=[view(m.weight) for m in layers], b=[view(m.bias) for m in layers], stride=stride)
    G.view = view
    return G


class ActorFn(torch.autograd.Function):
    """(mu, pi, log_pi, log_std) of the actor trunk and the squashed-Gaussian head (curl_sac.py:77-108) from the
    features ``z``; ``noise`` is a constant."""

    @staticmethod
    def forward(ctx, actor, keep, noise, compute_pi, compute_log_pi, z, *trunk_params):
        ctx.set_materialize_grads(False)
        B, A, H, F = z.shape[0], actor.action_dim, actor.hidden_dim, actor.encoder.feature_dim
        h1, h2, out = _empty(B, H, like=z), _empty(B, H, like=z), _empty(B, 2 * A, like=z)
        mu, log_std, tanh_ls = _empty(B, A, like=z), _empty(B, A, like=z), _empty(B, A, like=z)
        pi = _empty(B, A, like=z) if compute_pi else None
        log_pi = _empty(B, 1, like=z) if compute_pi and compute_log_pi else None
        _mlp_fwd(z, 0, _Mlp(actor.trunk), 1, B, F, H, 2 * A, h1, h2, out,
                 head=(noise if compute_pi else None, actor.log_std_min, actor.log_std_max,
                       dict(mu=mu, pi=pi, log_pi=log_pi, log_std=log_std, tanh_ls=tanh_ls)))
        ctx.actor, ctx.h1, ctx.h2 = actor, h1, h2
        keep.update(out=out)
        ctx.save_for_backward(z, noise if compute_pi else None, mu, pi, log_std, tanh_ls)
        if not compute_pi:
            return mu, log_std
        if log_pi is None:
            return mu, pi, log_std
        return mu, pi, log_pi, log_std

    @staticmethod
    @once_differentiable_hip
    def backward(ctx, *grads):
        actor = ctx.actor
        z, noise, mu, pi, log_std, tanh_ls = ctx.saved_tensors
        if pi is None:
            dmu, dls = grads
            dpi = dlp = None
        elif len(grads) == 3:
            dmu, dpi, dls = grads
            dlp = None
        else:
            dmu, dpi, dlp, dls = grads
        B, A, H, F = z.shape[0], actor.action_dim, actor.hidden_dim, actor.encoder.feature_dim
        need = ctx.needs_input_grad
        none = (None,) * (6 + 6)
        if all(g is None for g in (dmu, dpi, dlp, dls)) or not any(need[5:]):
            return none
        dout = _empty(B, 2 * A, like=z)
        ops.policy_head_bwd(_contig(dmu), _contig(dpi), _contig(dlp), _contig(dls), noise, mu, pi, log_std, tanh_ls, B, A,
                            actor.log_std_min, actor.log_std_max, dout)
        G = _grad_mlp(_linears(actor.trunk)) if any(need[6:]) else None
        dz = _empty(B, F, like=z) if need[5] else None
        _mlp_bwd(z, 0, _Mlp(actor.trunk), G, 1, B, F, H, 2 * A, ctx.h1, ctx.h2, dout, _empty(B, H, like=z),
                 _empty(B, H, like=z), dz)
        pg = [None] * 6 if G is None else [t for i in range(3) for t in (G.W[i], G.b[i])]
        return (None, None, None, None, None, dz, *pg)


class DetActorFn(torch.autograd.Function):
    """(mu[, pi]) of the deterministic actor (Actor(deterministic=True)) from the features ``z``: the trunk
    and the head on the launches of the no-grad forward.  ``noise`` is a constant; log_pi (zeros) and log_std (log(std))
    are constants too and are written into ``keep``'s plain tensors by the same launch."""

    @staticmethod
    def forward(ctx, actor, keep, noise, z, *trunk_params):
        ctx.set_materialize_grads(False)
        B, A, H, F = z.shape[0], actor.action_dim, actor.hidden_dim, actor.encoder.feature_dim
        h1, h2, out = _empty(B, H, like=z), _empty(B, H, like=z), _empty(B, A, like=z)
        mu = _empty(B, A, like=z)
        pi = _empty(B, A, like=z) if noise is not None else None
        _mlp_fwd(z, 0, _Mlp(actor.trunk), 1, B, F, H, A, h1, h2, out,
                 head=(noise, actor.std_on(z.device), None,
                       dict(mu=mu, pi=pi, log_pi=keep.get("log_pi"), log_std=keep["log_std"]), "det"))
        ctx.actor, ctx.h1, ctx.h2 = actor, h1, h2
        keep.update(out=out)
        ctx.save_for_backward(z, mu)
        return (mu, pi) if pi is not None else mu

    @staticmethod
    @once_differentiable_hip
    def backward(ctx, *grads):
        actor = ctx.actor
        z, mu = ctx.saved_tensors
        dmu, dpi = grads if len(grads) == 2 else (grads[0], None)
        B, A, H, F = z.shape[0], actor.action_dim, actor.hidden_dim, actor.encoder.feature_dim
        need = ctx.needs_input_grad
        if (dmu is None and dpi is None) or not any(need[3:]):
            return (None,) * (4 + 6)
        dout = _empty(B, A, like=z)
        ops.det_policy_head_bwd(_contig(dmu), _contig(dpi), mu, B, A, dout)
        G = _grad_mlp(_linears(actor.trunk)) if any(need[4:]) else None
        dz = _empty(B, F, like=z) if need[3] else None
        _mlp_bwd(z, 0, _Mlp(actor.trunk), G, 1, B, F, H, A, ctx.h1, ctx.h2, dout, _empty(B, H, like=z),
                 _empty(B, H, like=z), dz)
        pg = [None] * 6 if G is None else [t for i in range(3) for t in (G.W[i], G.b[i])]
        return (None, None, None, dz, *pg)


def _det_actor_forward(actor, z, compute_pi, compute_log_pi, noise):
    B, A = z.shape[0], actor.action_dim
    keep = dict(log_std=_empty(B, A, like=z))
    if compute_pi:
        noise = torch.randn((B, A), device=z.device) if noise is None else noise.detach().contiguous().float()
        if compute_log_pi:
            keep["log_pi"] = _empty(B, 1, like=z)
    else:
        noise = None
    outs = DetActorFn.apply(actor, keep, noise, z, *[t for m in _linears(actor.trunk) for t in (m.weight, m.bias)])
    mu, pi = outs if compute_pi else (outs, None)
    actor.outputs['mu'] = keep["out"]
    actor.outputs['std'] = keep["log_std"].exp()
    return mu, pi, keep.get("log_pi"), keep["log_std"]


def actor_forward(actor, z, compute_pi, compute_log_pi, noise):
    if actor.deterministic:
        return _det_actor_forward(actor, z, compute_pi, compute_log_pi, noise)
    B, A = z.shape[0], actor.action_dim
    if compute_pi:
        noise = torch.randn((B, A), device=z.device) if noise is None else noise.detach().contiguous().float()
    keep = {}
    outs = ActorFn.apply(actor, keep, noise, bool(compute_pi), bool(compute_log_pi), z,
                         *[t for m in _linears(actor.trunk) for t in (m.weight, m.bias)])
    if not compute_pi:
        mu, log_std = outs
        pi = log_pi = None
    elif not compute_log_pi:
        (mu, pi, log_std), log_pi = outs, None
    else:
        mu, pi, log_pi, log_std = outs
    actor.outputs['mu'] = keep["out"][:, :A]  # the pre-squash mean and the std, as the inference path records them
    actor.outputs['std'] = log_std.detach().exp()
    return mu, pi, log_pi, log_std


# ------------------------------------------------------------------------------------------------------------ critic
def _q_modules(q):
    """The modules of a Q function's trunk that hold parameters, in order: its three Linears and, in a LayerNorm
    critic, the LayerNorm behind each hidden one."""
    return [m for m in q.trunk if isinstance(m, (torch.nn.Linear, torch.nn.LayerNorm))]


def _q_params(critic):
    return [t for q in (critic.Q1, critic.Q2) for m in _q_modules(q) for t in (m.weight, m.bias)]


class CriticFn(torch.autograd.Function):
    """(q1, q2) of the twin Q functions on [z | action] (curl_sac.py:129-139,157-169) in their flat twin layout.
    ``drop`` = (p, (seed, counter), tag) or None: a dropout critic's masks (Critic.twin_ln), kept for the backward,
    which draws them again."""

    @staticmethod
    def forward(ctx, critic, z, action, drop, *q_params):
        ctx.set_materialize_grads(False)
        B, A, H, F = z.shape[0], critic.action_dim, critic.hidden_dim, critic.encoder.feature_dim
        xa = _empty(B, F + A, like=z)
        ops.concat(z, action, B, F, A, xa)
        M = critic.out_dim  # (the quantile atoms of a Critic(quantiles=M), else the one Q value)
        h1, h2, q = _empty(2, B, H, like=z), _empty(2, B, H, like=z), _empty(2, B, M, like=z)
        ctx.ln_saves = (None, None)
        if critic.layer_norm:  # what the LayerNorms' backward reads, per hidden layer
            ctx.ln_saves = ([_empty(2, B, H, like=z) for _ in range(2)], [_empty(2, B, like=z) for _ in range(2)])
        _mlp_fwd(xa, 0, critic.twin(), 2, B, F + A, H, M, h1, h2, q,
                 ln=critic.twin_ln(*ctx.ln_saves, drop=drop))
        ctx.critic, ctx.xa, ctx.h1, ctx.h2, ctx.B, ctx.drop, ctx.M = critic, xa, h1, h2, B, drop, M
        return q[0], q[1]

    @staticmethod
    @once_differentiable_hip
    def backward(ctx, dq1, dq2):
        critic, B = ctx.critic, ctx.B
        A, H, F = critic.action_dim, critic.hidden_dim, critic.encoder.feature_dim
        need = ctx.needs_input_grad
        mods = _q_modules(critic.Q1)
        if dq1 is None and dq2 is None:
            return (None,) * (4 + 4 * len(mods))
        M = ctx.M
        dq = torch.zeros((2, B, M), device=ctx.xa.device, dtype=F32)
        if dq1 is not None:
            dq[0].copy_(dq1)
        if dq2 is not None:
            dq[1].copy_(dq2)
        G = _grad_mlp(_linears(critic.Q1.trunk), critic.twin_stride, span=mods) if any(need[4:]) else None
        want_x = need[1] or need[2]
        dxa = _empty(2, B, F + A, like=dq) if want_x else None
        ln = critic.twin_ln(*ctx.ln_saves, drop=ctx.drop)
        if ln is not None and G is not None:
            ln.dg, ln.db = [G.view(p) for p in ln.g], [G.view(p) for p in ln.b]
            ln.partial = torch.empty(ops.mlp_ln_partial_floats(B, H, 2), device=dq.device, dtype=F32)
        _mlp_bwd(ctx.xa, 0, critic.twin(), G, 2, B, F + A, H, M, ctx.h1, ctx.h2, dq, _empty(2, B, H, like=dq),
                 _empty(2, B, H, like=dq), dxa, ln=ln)
        dz = dact = None
        if want_x:
            dz = _empty(B, F, like=dq) if need[1] else None
            dact = _empty(B, A, like=dq) if need[2] else None
            ops.split_sum(dxa, B * (F + A), B, F, A, dz=dz, dact=dact)
        pg = [None] * (4 * len(mods))
        if G is not None:
            # (Q2's gradients sit twin_stride floats behind Q1's, as the parameters do)
            pg = [G.view(p, twin) for twin in (0, 1) for m in mods for p in (m.weight, m.bias)]
        return (None, dz, dact, None, *pg)


def critic_forward(critic, z, action, drop=None):
    action = action.contiguous().float()
    return CriticFn.apply(critic, z, action, drop, *_q_params(critic))


# ------------------------------------------------------------------------------------------------------------ CURL
class CurlLogitsFn(torch.autograd.Function):
    """z_a (W z_pos^T) (curl_sac.py:211-220), both products on the kernels' GEMM; the row-max subtraction stays a
    torch op outside."""

    @staticmethod
    def forward(ctx, z_a, z_pos, W):
        B, F = z_a.shape
        WzT, logits = _empty(B, F, like=z_a), _empty(B, B, like=z_a)
        ops.linear_fwd(z_pos, 0, W, 0, None, 0, WzT, 0, B, F, F)
        ops.linear_fwd(z_a, 0, WzT, 0, None, 0, logits, 0, B, B, F)
        ctx.save_for_backward(z_a, z_pos, W)
        ctx.WzT = WzT
        return logits

    @staticmethod
    @once_differentiable_hip
    def backward(ctx, dlogits):
        z_a, z_pos, W = ctx.saved_tensors
        B, F = z_a.shape
        need = ctx.needs_input_grad
        dlogits = dlogits.contiguous()
        dz_a = dz_pos = dW = None
        if need[0]:
            dz_a = _empty(B, F, like=z_a)
            ops.linear_dx(dlogits, 0, ctx.WzT, 0, dz_a, 0, B, B, F)
        if need[1] or need[2]:
            dWzT = _empty(B, F, like=z_a)  # d (W z_pos^T)^T
            ops.linear_dw(dlogits, 0, z_a, 0, dWzT, 0, B, B, F)
            if need[1]:
                dz_pos = _empty(B, F, like=z_a)
                ops.linear_dx(dWzT, 0, W, 0, dz_pos, 0, B, F, F)
            if need[2]:
                dW = torch.empty_like(W)
                ops.linear_dw(dWzT, 0, z_pos, 0, dW, 0, B, F, F)
        return dz_a, dz_pos, dW
