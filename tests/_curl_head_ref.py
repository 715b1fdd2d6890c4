"""Float64 stage references, derived error bounds, input builders and the case list of the one-launch CURL head
(curl_head_kernel<NTILE>, csrc/curl_head.h; entry curla_curl_head) for tests/test_gpu_curl_head_edges.py.  CPU only;
checked by tests/test_curl_head_ref_host.py.

The head is a chain of seven stages.  Each stage's reference is computed in float64 FROM THE KERNEL'S OWN float32 OUTPUT
OF THE STAGE BEFORE IT (logits -> row_loss / dlogits -> dz, T -> dfc -> the 16-row partials -> their sums), so that no
stage's error is charged to the next and every bound stays the bound of one short formula.

Bounds are |got - ref64| <= n * 2^-24 * S element by element (tests/_loss_head_ref.py, "error bounds"): S is the stage's
formula evaluated on absolute values, n twice the float32 roundings on the longest path to an element, counted from
csrc/curl_head.h; 2^-126 absolute is added where a term may be a denormal (dlogits near 0 at large scales, and all that
is formed from them).  The f32 MFMA (v_mfma_f32_16x16x4_f32) is a k-ordered chain of fused multiply-adds, one rounding
per product and none inside.  The counts, stage by stage:

logits         N_LOGITS(F) = 2 (F + 1).  Phase A: lg = mfma16(af[s], bf[s], lg), s = 0 .. 12: 52 fused multiply-adds on
               one accumulator, F of them with a non-zero z_a operand (the others add an exact zero): F roundings, one spare.
row_loss,      curl_ce_bounds(adds = B / 128 + 11).  The sum of exponentials: a lane's NTILE = B / 128 serial adds, four
dlogits        __shfl_xor levels inside the 16-lane group, seven adds across the eight waves' sums in LDS; the row maximum
               is exact (fmaxf).  The rest is curl_ce's formula, rounding for rounding: expf(l - m), logf(sum) + m,
               lse - l_aa; (expf(l - lse) - [j == a]) * (1.f / B).
dz             N_PRODUCT(B) = 2 (B / 8 + 9).  Phase B: a wave multiplies its eighth of k into one accumulator per
               feature tile: B / 32 MFMAs of 4 k each, B / 8 roundings; the eight waves' partial tiles are then added
               in order (seven adds); two spare.
w_partial      2 (B / 8 + 9 + 17).  T = dlogits . z_pos by the same chain; then wp[i][k] = sum over the block's 16 rows of
               zs[r][i] * t0[r][k]: a product and an add per row, the product's rounding and the 16 adds on top of T's.
dfc            N_DFC = 28.  Per element o = rstd * (g - m1 - xhat * m2): the longest path is m2's: g = d * gamma (1),
               g * xhat (1), wave_sum's six __shfl_xor levels (6), / F (1), xhat * m2 (1), two subtractions (2), the
               product with rstd (1): 13, one spare.  (m1's path is one shorter, g's own is 4.)
ln_partial     N_LN_PARTIAL = 22.  p0 += d * xhat over a wave's two rows (one product, two adds), then the eight waves'
               partials added in order (seven adds): 10, one spare.  (sum d and sum dfc are the same without the product.)
dgamma, dbeta, N_SUM(B) = 2 B / 16.  ln_reduce_block (csrc/fc_bwd.h) adds the B / 16 partials of an element one after the
dbias, dW      other into one float.
loss           the mean of the row bounds (the kernel means its own float32 row losses) + R.scalar_bound(row losses).
"""
import math

import torch
import torch.nn.functional as F_

from tests import _loss_head_ref as R

F64 = torch.float64
DENORM = 2.0 ** -126
EPS = 1e-5  # the encoder's LayerNorm

BS = (128, 256, 384, 512, 640, 768, 896, 1024)  # every NTILE 1..8: PRELOAD (1..4), CH = 4 (5, 7), CH = 8 (6, 8)
FS = (49, 50, 51, 52)                           # nrest 1, 2, 3, 0; the last lane group's k run moved back at 49..51
SCALES = (3.0, 40.0, 300.0)
FULL_BS = (128, 640)                            # the full F x shift x scale cross


def shifts(B):
    """Where row a's maximum sits, relative to the diagonal: on it; the next column (same tile, over a tile's edge at
    li = 15); the next wave's tile; the same wave's next i tile (B >= 256); the column before, round the corner."""
    return (0, 1, 16) + ((128,) if B >= 256 else ()) + (B - 1,)


def _cases():
    out = []
    for B in FULL_BS:
        for Fd in FS:
            for sh in shifts(B):
                for sc in SCALES:
                    out.append((B, Fd, sh, sc))
    # the other B: one case per shift, F and the scale rotating with t = i + 2 b + 1: five consecutive t hold every F and
    # every scale, and t runs over 1 .. 15, whose (t % 4, t % 3) are all twelve (F, scale) pairs
    for b, B in enumerate(x for x in BS if x not in FULL_BS):
        for i, sh in enumerate(shifts(B)):
            t = i + 2 * b + 1
            out.append((B, FS[t % 4], sh, SCALES[t % 3]))
    return tuple(out)


CASES = _cases()  # (B, F, shift, scale)
# (B, F) of the special inputs, one supported shape per F; 384 and 640 hold the twins' second pair (j' = j + 128)
SPECIAL_SHAPES = ((128, 49), (384, 50), (640, 51), (1024, 52))
SPECIALS = ("uniform", "twins", "flat_row", "zero_row")
TWIN_J = 3
SPECIAL_ROW = 21  # flat_row / zero_row: in the second block of 16, an odd row of its wave


# The builder's conditions (tests/test_curl_head_ref_host.py checks them at every case) ask for every row loss below
# 1e-6 at shift 0 and scale 40, that is a gap of about 14 between a row's maximum and its runner-up.  Past B = 512 one
# draw in twenty to a hundred has it: these cases walk their seed on in steps of SEED_STRIDE, by the number of steps
# at which the conditions first held.
SEED_STRIDE = 7919
SEED_STEPS = {(640, 49, 0, 40.0): 24, (640, 50, 0, 40.0): 91, (640, 51, 0, 40.0): 46, (640, 52, 0, 40.0): 19,
              (768, 52, 0, 40.0): 30}


def case_seed(B, Fd, shift, scale):
    return B * 100003 + Fd * 1009 + shift * 17 + int(scale) + SEED_STRIDE * SEED_STEPS.get((B, Fd, shift, scale), 0)


def case_inputs(case):
    return head_inputs(*case, seed=case_seed(*case))


def odd_offset(B, Fd, shift, scale):
    """The one case per F whose operands start at an odd float offset."""
    return B == 128 and shift == 1 and scale == 3.0


# ---------------------------------------------------------------------------------------------------------- inputs
def head_inputs(B, Fd, shift, scale, seed):
    """float32 z_a, z_pos, wz [B, F], xhat [B, F], rstd [B], gamma [F] with a planted row maximum: column (a + shift) % B
    is row a's partner, logits[a, partner] = scale up to the noise.  gamma is 0 at every 7th feature and negative at
    3, 14, 25, ...; xhat / rstd are the float64 LayerNorm state of fc = 2 randn + 0.5 rounded to float32."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)  # noqa: E731
    fc = 2 * r(B, Fd) + 0.5
    gamma = 1 + 0.1 * r(Fd)
    gamma[::7] = 0
    gamma[3::11] = -gamma[3::11]
    beta = 0.1 * r(Fd)
    mean = fc.mean(1, keepdim=True)
    rstd = (fc.var(1, unbiased=False, keepdim=True) + EPS).rsqrt()
    xhat = ((fc - mean) * rstd).float()
    rstd, gamma, beta = rstd.flatten().float(), gamma.float(), beta.float()
    z_a = (xhat.double() * gamma.double() + beta.double()).float()
    z_pos = (0.7 * r(B, Fd)).float()
    a_j = (torch.arange(B) - shift) % B
    za = z_a.double()[a_j]
    wz = (scale * za / za.pow(2).sum(1, keepdim=True) + 0.02 * scale * r(B, Fd) / math.sqrt(Fd)).float()
    return z_a, z_pos, wz, xhat, rstd, gamma


def special_inputs(kind, B, Fd, seed):
    """head_inputs(B, F, shift 1, scale 3) with one thing changed (the tensors are fresh, the change is made in place):
    uniform   wz = 0: every logit is exactly 0
    twins     rows j and j' of wz and of z_pos identical: j = 3 and j' = 16 + 3 (the next wave's tile), and, B >= 256,
              j' = 128 + 3 (the same wave's next i tile)
    flat_row  anchor row SPECIAL_ROW is a constant fc row: xhat = 0, rstd = eps^-1/2, z_a = beta
    zero_row  anchor row SPECIAL_ROW of z_a is all zeros"""
    z_a, z_pos, wz, xhat, rstd, gamma = head_inputs(B, Fd, 1, 3.0, seed)
    if kind == "uniform":
        wz.zero_()
    elif kind == "twins":
        for j2 in twin_partners(B):
            wz[j2], z_pos[j2] = wz[TWIN_J], z_pos[TWIN_J]
    elif kind == "flat_row":
        beta = 0.1 * torch.randn(Fd, generator=torch.Generator().manual_seed(seed + 1))
        xhat[SPECIAL_ROW], rstd[SPECIAL_ROW], z_a[SPECIAL_ROW] = 0.0, EPS ** -0.5, beta
    elif kind == "zero_row":
        z_a[SPECIAL_ROW] = 0.0
    else:
        raise ValueError(kind)
    return z_a, z_pos, wz, xhat, rstd, gamma


def twin_partners(B):
    return (16 + TWIN_J,) + ((128 + TWIN_J,) if B >= 256 else ())


# ------------------------------------------------------------------------------------------------ stage references
def n_logits(Fd):
    return 2 * (Fd + 1)


def ce_adds(B):
    return B // 128 + 11


def n_product(B):
    return 2 * (B // 8 + 9)


def n_w_partial(B):
    return 2 * (B // 8 + 9 + 17)


N_DFC = 28
N_LN_PARTIAL = 22


def n_sum(B):
    return 2 * (B // 16)


def ref_logits(z_a, wz):
    """1. logits = z_a wz^T.  Returns (ref, bound)."""
    za, w = R.f64(z_a), R.f64(wz)
    return za @ w.t(), n_logits(za.shape[1]) * R.U * (za.abs() @ w.abs().t())


def ref_ce(logits):
    """2. R.curl_ce of the logits handed in, and curl_ce_bounds with the head's chain of adds.
    Returns (curl_ce's dict, dict(row_loss, dlogits, loss) of bounds)."""
    ref = R.curl_ce(logits)
    b = R.curl_ce_bounds(ref, logits, adds=ce_adds(ref["mx"].numel()))
    b["loss"] = float(b["row_loss"].mean()) + R.scalar_bound(ref["row_loss"])
    return ref, b


def ref_dz(dlogits, wz):
    """3. dz = dlogits wz."""
    dl, w = R.f64(dlogits), R.f64(wz)
    return dl @ w, n_product(dl.shape[0]) * R.U * (dl.abs() @ w.abs()) + DENORM


def ref_w_partial(z_a, dlogits, z_pos):
    """4. w_partial[blk] = z_a[blk]^T (dlogits[blk] z_pos) for each block of 16 rows: [B / 16, F, F]."""
    za, dl, zp = R.f64(z_a), R.f64(dlogits), R.f64(z_pos)
    B, Fd = za.shape
    T, Ta = dl @ zp, dl.abs() @ zp.abs()
    blk = lambda x: x.view(B // 16, 16, Fd)  # noqa: E731
    ref = torch.einsum("bri,brk->bik", blk(za), blk(T))
    S = torch.einsum("bri,brk->bik", blk(za.abs()), blk(Ta))
    return ref, n_w_partial(B) * R.U * S + DENORM


def ref_dfc(dz, xhat, rstd, gamma):
    """5. The LayerNorm backward dfc = rstd (g - mean g - xhat mean(g xhat)), g = dz gamma."""
    d, xh, rs, gm = R.f64(dz), R.f64(xhat), R.f64(rstd).reshape(-1, 1), R.f64(gamma)
    g = d * gm
    ref = rs * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
    S = rs.abs() * (g.abs() + g.abs().mean(1, keepdim=True) + xh.abs() * (g * xh).abs().mean(1, keepdim=True))
    return ref, N_DFC * R.U * S + DENORM


def ref_ln_partial(dz, dfc, xhat):
    """6. ln_partial[blk] = (sum d xhat, sum d, sum dfc) over the block's 16 rows: [B / 16, 3, F]."""
    d, o, xh = R.f64(dz), R.f64(dfc), R.f64(xhat)
    B, Fd = d.shape
    rows = torch.stack([d * xh, d, o], 1).view(B // 16, 16, 3, Fd)  # [blk, row, 3, F]
    return rows.sum(1), N_LN_PARTIAL * R.U * rows.abs().sum(1) + DENORM


def ref_sums(ln_partial, w_partial, B, Fd):
    """7. dgamma, dbeta, dbias [F], dW [F, F]: the sums over blocks of the partials.  Returns {name: (ref, bound)}."""
    lp, wp = R.f64(ln_partial).reshape(B // 16, 3, Fd), R.f64(w_partial).reshape(B // 16, Fd, Fd)
    n = n_sum(B) * R.U
    out = {k: (lp[:, q].sum(0), n * lp[:, q].abs().sum(0) + DENORM) for q, k in enumerate(("dgamma", "dbeta", "dbias"))}
    out["dW"] = (wp.sum(0), n * wp.abs().sum(0) + DENORM)
    return out


STAGES = ("logits", "row_loss", "dlogits", "loss", "dz", "w_partial", "dfc", "ln_partial", "dgamma", "dbeta", "dbias", "dW")


def stage_checks(inp, out):
    """[(stage, got, ref64, bound)] for the outputs in `out` (float32 tensors by the names of STAGES; "loss" and the
    four sums are optional) of the head run on inp = (z_a, z_pos, wz, xhat, rstd, gamma)."""
    z_a, z_pos, wz, xhat, rstd, gamma = inp
    B, Fd = z_a.shape
    ce, ce_b = ref_ce(out["logits"])
    checks = [("logits", out["logits"]) + ref_logits(z_a, wz),
              ("row_loss", out["row_loss"], ce["row_loss"], ce_b["row_loss"]),
              ("dlogits", out["dlogits"], ce["dlogits"], ce_b["dlogits"])]
    if out.get("loss") is not None:
        checks.append(("loss", out["loss"].reshape(1), ce["loss"].reshape(1), torch.tensor([ce_b["loss"]], dtype=F64)))
    checks += [("dz", out["dz"]) + ref_dz(out["dlogits"], wz),
               ("w_partial", out["w_partial"]) + ref_w_partial(z_a, out["dlogits"], z_pos),
               ("dfc", out["dfc"]) + ref_dfc(out["dz"], xhat, rstd, gamma),
               ("ln_partial", out["ln_partial"]) + ref_ln_partial(out["dz"], out["dfc"], xhat)]
    if out.get("dW") is not None:
        sums = ref_sums(out["ln_partial"], out["w_partial"], B, Fd)
        checks += [(k, out[k]) + sums[k] for k in ("dgamma", "dbeta", "dbias", "dW")]
    return checks


def ratios(inp, out):
    """{stage: worst |got - ref| / bound}, inf where an output is not finite."""
    res = {}
    for stage, got, ref, bound in stage_checks(inp, out):
        got = R.f64(got).reshape(ref.shape)
        if not bool(torch.isfinite(got).all()):
            res[stage] = float("inf")
            continue
        err = (got - ref).abs()
        res[stage] = float(torch.where(err == 0, torch.zeros_like(err), err / bound.expand(ref.shape).clamp_min(1e-300)).max())
    return res


# ------------------------------------------------------------------------- the float32 evaluation, right and wrong
VARIANTS = ("drop_k", "no_max", "shifted_identity", "inv_b_minus_1", "z_pos_in_dz", "w_partial_transposed", "no_m2")


def eval32(inp, variant=None):
    """The head's formulas in float32 torch on the CPU, as a kernel would chain them (every stage from the float32
    result of the one before): all of STAGES.  `variant`: one of VARIANTS, a head that is wrong in one place."""
    assert variant is None or variant in VARIANTS
    z_a, z_pos, wz, xhat, rstd, gamma = inp
    B, Fd = z_a.shape
    logits = z_a[:, :-1] @ wz[:, :-1].t() if variant == "drop_k" else z_a @ wz.t()
    mx = torch.zeros(B, 1) if variant == "no_max" else logits.max(1, keepdim=True).values
    lse = (logits - mx).exp().sum(1, keepdim=True).log() + mx
    row_loss = lse.flatten() - logits.diagonal()
    eye = torch.eye(B)
    if variant == "shifted_identity":
        eye = eye.roll(1, 1)
    inv = torch.tensor(1.0) / (B - 1 if variant == "inv_b_minus_1" else B)
    dlogits = ((logits - lse).exp() - eye) * inv
    dz = dlogits @ (z_pos if variant == "z_pos_in_dz" else wz)
    T = dlogits @ z_pos
    w_partial = torch.einsum("bri,brk->bik", z_a.view(B // 16, 16, Fd), T.view(B // 16, 16, Fd))
    if variant == "w_partial_transposed":
        w_partial = w_partial.transpose(1, 2).contiguous()
    g = dz * gamma
    m2 = torch.zeros(B, 1) if variant == "no_m2" else (g * xhat).mean(1, keepdim=True)
    dfc = rstd[:, None] * (g - g.mean(1, keepdim=True) - xhat * m2)
    ln_partial = torch.stack([dz * xhat, dz, dfc], 1).view(B // 16, 16, 3, Fd).sum(1)
    sums = ln_partial.sum(0)
    return dict(logits=logits, row_loss=row_loss, dlogits=dlogits, loss=row_loss.mean(), dz=dz, w_partial=w_partial, dfc=dfc,
                ln_partial=ln_partial, dgamma=sums[0], dbeta=sums[1], dbias=sums[2], dW=w_partial.sum(0))


# ---------------------------------------------------------------------------------------------- the composition
def chain64(fc, gamma, beta, W, z_pos):
    """The stage references chained in float64 (each fed the float64 result of the one before) from the anchors'
    pre-LayerNorm features: dict(loss, dfc, dgamma, dbeta, dbias, dW) -- what autograd gives for
    LayerNorm -> z_a W z_pos^T -> cross_entropy(arange)."""
    fc, gamma, beta, W, z_pos = (R.f64(t) for t in (fc, gamma, beta, W, z_pos))
    B, Fd = fc.shape
    rstd = (fc.var(1, unbiased=False, keepdim=True) + EPS).rsqrt()
    xhat = (fc - fc.mean(1, keepdim=True)) * rstd
    z_a = xhat * gamma + beta
    wz = z_pos @ W.t()
    logits = ref_logits(z_a, wz)[0]
    ce = R.curl_ce(logits)
    dz = ref_dz(ce["dlogits"], wz)[0]
    wp = ref_w_partial(z_a, ce["dlogits"], z_pos)[0]
    dfc = ref_dfc(dz, xhat, rstd, gamma)[0]
    lp = ref_ln_partial(dz, dfc, xhat)[0]
    sums = {k: v[0] for k, v in ref_sums(lp, wp, B, Fd).items()}
    return dict(loss=ce["loss"], dfc=dfc, **sums)


def autograd64(fc, gamma, beta, W, z_pos):
    fc, gamma, beta, W = (R.f64(t).clone().requires_grad_(True) for t in (fc, gamma, beta, W))
    z_a = F_.layer_norm(fc, (fc.shape[1],), gamma, beta, EPS)
    logits = z_a @ W @ R.f64(z_pos).t()
    loss = F_.cross_entropy(logits, torch.arange(fc.shape[0]))
    loss.backward()
    return dict(loss=loss.detach(), dfc=fc.grad, dgamma=gamma.grad, dbeta=beta.grad, dbias=fc.grad.sum(0), dW=W.grad)
