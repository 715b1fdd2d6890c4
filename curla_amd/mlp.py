"""The launch sequences of a 3-layer MLP (the actor trunk, the twin Q functions), forward and backward."""
import torch.nn as nn

from . import ops


class _Mlp:
    """Pointers of a 3-layer MLP (or of the first of two identically laid-out
    twins, ``stride`` floats apart)."""

    def __init__(self, seq, stride=0, grads=False):
        lin = _linears(seq)
        pick = (lambda p: p.grad) if grads else (lambda p: p)
        self.W = [pick(layer.weight) for layer in lin]
        self.b = [pick(layer.bias) for layer in lin]
        self.stride = stride


def _linears(seq):
    """The three Linears of a trunk, by type: a LayerNorm critic's sit at 0, 3, 6 instead of 0, 2, 4."""
    lin = [m for m in seq if isinstance(m, nn.Linear)]
    assert len(lin) == 3, "a 3-layer MLP"
    return lin


class _MlpLn:
    """The LayerNorm side of a _Mlp whose hidden layers are Linear - LayerNorm - ReLU (Critic(layer_norm=True)), layer
    by layer: the LayerNorms' parameters ``g`` / ``b`` (twins and groups addressed as the _Mlp's), the buffers
    ``xhat`` [2, B, H] / ``rstd`` [2, B] a forward saves for its backward (None: a no-grad pass) and, for a backward
    that wants parameter gradients, their destinations ``dg`` / ``db`` and the ``partial`` workspace
    (ops.mlp_ln_partial_floats).  ``save_first``: with _mlp_fwd's ``outer``, the first group that saves.
    ``drop`` = (p, rng, tag): DroQ's dropout in front of each LayerNorm (Critic(dropout=p)) -- the mask of hidden layer i
    is drawn under ``rng`` = (seed, counter[, device address]) and tag + i (group o of ``outer`` under tag + i + 2 o;
    ops.mlp_drop_ln_relu_fwd), in the forward and again in the backward.  None: no dropout, the plain launches."""

    def __init__(self, seq, xhat=None, rstd=None, dg=None, db=None, partial=None, save_first=0, drop=None):
        ln = [m for m in seq if isinstance(m, nn.LayerNorm)]
        assert len(ln) == 2, "a LayerNorm behind each hidden layer"
        self.g = [m.weight for m in ln]
        self.b = [m.bias for m in ln]
        self.xhat, self.rstd, self.dg, self.db, self.partial, self.save_first = xhat, rstd, dg, db, partial, save_first
        self.drop = drop

    def fwd(self, i, h, s, nb, B, H, outer):
        """LayerNorm + ReLU of hidden layer ``i`` in place on ``h``, which linear_fwd(relu=0) has just written."""
        saves = self.xhat is not None
        kw = dict(xhat=self.xhat[i] if saves else None, rstd=self.rstd[i] if saves else None,
                  outer=None if outer is None else (outer[0], nb * B * H, outer[1]),
                  save_first=self.save_first if outer is not None and saves else 0)
        if self.drop is None:
            ops.mlp_ln_relu_fwd(h, B * H, self.g[i], self.b[i], s, B, H, nb, **kw)
        else:
            p, rng, tag = self.drop
            ops.mlp_drop_ln_relu_fwd(h, B * H, self.g[i], self.b[i], s, B, H, p, rng, tag + i, nb, **kw)

    def bwd(self, i, dh, s, nb, B, H, dbias):
        """``dh`` (ReLU-masked by the layer behind) -> the gradient of Linear ``i``'s output, in place; with ``dbias``
        (that Linear's bias gradient) also the LayerNorm's parameter gradients."""
        kw = {} if dbias is None else dict(partial=self.partial, dgamma=self.dg[i], dbeta=self.db[i], dbias=dbias, sg=s)
        if self.drop is None:
            ops.mlp_ln_bwd(dh, B * H, self.xhat[i], self.rstd[i], self.g[i], s, B, H, nb, **kw)
        else:
            p, rng, tag = self.drop
            ops.mlp_drop_ln_bwd(dh, B * H, self.xhat[i], self.rstd[i], self.g[i], s, B, H, p, rng, tag + i, nb, **kw)


def _mlp_fwd(x, sx, P, nb, B, din, H, dout, h1, h2, out, relu_out=0, outer=None, head=None, ln=None):
    """``outer`` = (n2, sW2): n2 such MLP groups in the same launches, their parameters sW2 floats apart (the target
    critic's and the critic's twins); x [n2][B, din] and h1 / h2 / out [n2][nb][B, .] then.
    ``head`` = (noise, lo, hi, outputs): the MLP is the actor trunk and the policy head (ops.actor_head_fwd with these
    arguments) follows its last layer -- in the same launch when the layer is small enough.  ``head`` = (noise, std,
    clip, outputs, "det"): the deterministic head (ops.det_head_fwd) instead, over ``dout`` = A outputs.
    ``ln`` (_MlpLn): a LayerNorm sits between each hidden Linear and its ReLU -- the GEMM leaves the ReLU out and one
    launch per hidden layer normalises in place."""
    s = P.stride
    o0 = o1 = o2 = None
    if outer is not None:
        n2, sW2 = outer
        o0, o1, o2 = (n2, B * din, sW2, nb * B * H), (n2, nb * B * H, sW2, nb * B * H), (n2, nb * B * H, sW2, nb * B * dout)
    relu = 1 if ln is None else 0
    ops.linear_fwd(x, sx, P.W[0], s, P.b[0], s, h1, B * H, B, H, din, nb, relu=relu, outer=o0)
    if ln is not None:
        ln.fwd(0, h1, s, nb, B, H, outer)
    ops.linear_fwd(h1, B * H, P.W[1], s, P.b[1], s, h2, B * H, B, H, H, nb, relu=relu, outer=o1)
    if ln is not None:
        ln.fwd(1, h2, s, nb, B, H, outer)
    small = dout <= ops.MLP_OUT_MAX and H % 4 == 0 and not relu_out
    det = head is not None and len(head) == 5
    if det and small and nb == 1 and outer is None:
        noise, std, clip, outs, _ = head
        ops.mlp_out_det_head_fwd(h2, P.W[2], P.b[2], out, noise, B, dout, H, std, clip, **outs)
        return
    if head is not None and not det and small and nb == 1 and outer is None:
        noise, lo, hi, outs = head
        ops.mlp_out_head_fwd(h2, P.W[2], P.b[2], out, noise, B, dout // 2, H, lo, hi, **outs)
        return
    if small:  # a handful of outputs: row dot products, not a GEMM
        ops.mlp_out_fwd(h2, B * H, P.W[2], s, P.b[2], s, out, B * dout, B, dout, H, nb, outer=o2)
    else:
        ops.linear_fwd(h2, B * H, P.W[2], s, P.b[2], s, out, B * dout, B, dout, H, nb, relu=relu_out, outer=o2)
    if det:
        noise, std, clip, outs, _ = head
        ops.det_head_fwd(out, noise, std, clip, B, dout, **outs)
    elif head is not None:
        noise, lo, hi, outs = head
        ops.actor_head_fwd(out, noise, B, dout // 2, lo, hi, **outs)


def _mlp_bwd(x, sx, P, G, nb, B, din, H, dout, h1, h2, dy, dh2, dh1, dx, loss=None, ln=None):
    """Backward of _mlp_fwd.  G (parameter gradients) and dx are optional.
    ``loss`` = (fields, launch): the output gradient dy is that of a loss over the twin Q values -- ``fields`` for
    ops.mlp_out_bwd_loss, which computes it inside the last layer's backward launch; ``launch()`` runs the loss kernel
    on its own where that form does not apply (``fields`` None: always -- the quantile losses have no fused form).
    ``ln`` (_MlpLn, with the forward's xhat / rstd): h1 / h2 are the post-LayerNorm ReLU outputs, so the masks below
    (h2 > 0, mask=h1) are still the ReLUs' and leave dh2 / dh1 as the gradients of the LayerNorms' outputs; one
    launch per hidden layer turns each, in place, into the gradient of its Linear's output.  The hidden Linears' bias
    gradients are then column sums of THAT, not of the masked dh: they come from the same launch, and the folds of
    them into the neighbouring launches are off."""
    s = P.stride
    fused_loss = loss is not None and loss[0] is not None and dout == 1 and nb == 2  # (no fields: the launch alone)
    if loss is not None and not fused_loss:
        loss[1]()
    # the three bias gradients (column sums of dy, dh2, dh1) ride in the launches that walk those matrices anyway --
    # the last layer's backward pass and the first layer's weight-gradient product -- where both take their small forms
    fold = G is not None and dout <= ops.MLP_OUT_MAX and ops.linear_dw_folds_bias(B, H, din, nb)
    fold_h = fold and ln is None
    if fused_loss:
        ops.mlp_out_bwd_loss(loss[0], h2, B * H, P.W[2], s, dh2, B * H, G.W[2] if G is not None else None, s, B, H,
                             db_out=G.b[2] if fold else None, db_hidden=G.b[1] if fold_h else None, sdb=s)
    elif dout <= ops.MLP_OUT_MAX:  # last layer: data and weight gradient in one pass over h2
        ops.mlp_out_bwd(dy, B * dout, h2, B * H, P.W[2], s, dh2, B * H, G.W[2] if G is not None else None, s, B, dout,
                        H, nb, db_out=G.b[2] if fold else None, db_hidden=G.b[1] if fold_h else None, sdb=s)
    else:
        if G is not None:
            ops.linear_dw(dy, B * dout, h2, B * H, G.W[2], s, B, dout, H, nb)
        ops.linear_dx(dy, B * dout, P.W[2], s, dh2, B * H, B, dout, H, nb, mask=h2, smask=B * H)
    if ln is not None:
        ln.bwd(1, dh2, s, nb, B, H, G.b[1] if G is not None else None)
    # a layer's weight and data gradient are independent products over the same dy: one launch for the pair
    if G is not None:
        ops.linear_bwd(dh2, B * H, h1, B * H, P.W[1], s, G.W[1], s, dh1, B * H, B, H, H, nb, mask=h1, smask=B * H)
    else:
        ops.linear_dx(dh2, B * H, P.W[1], s, dh1, B * H, B, H, H, nb, mask=h1, smask=B * H)
    if ln is not None:
        ln.bwd(0, dh1, s, nb, B, H, G.b[0] if G is not None else None)
    if G is not None and dx is not None:
        ops.linear_bwd(dh1, B * H, x, sx, P.W[0], s, G.W[0], s, dx, B * din, B, H, din, nb,
                       db=G.b[0] if fold_h else None, sdb=s)
    elif G is not None:
        ops.linear_dw(dh1, B * H, x, sx, G.W[0], s, B, H, din, nb, colsum=G.b[0] if fold_h else None, s_colsum=s)
    elif dx is not None:
        ops.linear_dx(dh1, B * H, P.W[0], s, dx, B * din, B, H, din, nb)
    if G is not None and not fold:
        if ln is None:
            ops.colsum3(dy, dout, dh2, H, dh1, H, B, G.b[2], G.b[1], G.b[0], s, nb)
        else:  # (the hidden layers' bias gradients are there already)
            ops.colsum(dy, B, dout, dout, B * dout, G.b[2], s, nb)
