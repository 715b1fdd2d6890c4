"""The definition of the dormant-neuron scores and of ReDo's recycling rule, written once in NumPy: the
kernels (curla_dormant_colsum, curla_dormant_mask, curla_redo_recycle) and the agent are held to it by
tests/test_redo_host.py and tests/test_gpu_redo.py.

    sum_j     = sum over b of |h[b][j]|                float32, b in index order
    total     = sum over j of (double) sum_j           float64, j in index order
    mean      = total / H                              float64
    score_j   = (float)((double) sum_j / mean)         (the batch size cancels)
    dormant_j = (mean == 0) or (score_j <= tau)        float32 compare: false for a NaN

The kernel adds ``total`` up in another fixed order (256 interleaved partial sums, then those in index order); the two
orders differ by rounding in float64 -- at most H * 2**-53 relative -- and not at all where the sums are exact.

    weight[i][j] = 0            if c[j]                 c: the dormant mask of the Linear's input units
                 = fresh[i][j]  else if r[i]            r: the dormant mask of its output units
                 = not written  otherwise
    a vector (bias, LayerNorm weight / bias): fresh[i] if r[i], else not written
    Adam's m and v: 0 wherever the rule writes, not written elsewhere
"""
import numpy as np

LAYERS = ("Q1.h1", "Q1.h2", "Q2.h1", "Q2.h2", "actor.h1", "actor.h2")


def colsum(h):
    """h [B][H] float32 -> the float32 sums of |h| down the columns, rows added in index order."""
    h = np.asarray(h, dtype=np.float32)
    s = np.zeros(h.shape[1], dtype=np.float32)
    for b in range(h.shape[0]):
        s = (s + np.abs(h[b])).astype(np.float32)
    return s


def dormant(sums, tau):
    """sums [H] float32 -> (score [H] float32, mask [H] bool, count int, fraction float32)."""
    sums = np.asarray(sums, dtype=np.float32)
    H = sums.shape[0]
    with np.errstate(all="ignore"):
        total = np.float64(0.0)
        for x in sums:
            total = total + np.float64(x)
        mean = total / np.float64(H)
        score = (sums.astype(np.float64) / mean).astype(np.float32)
        mask = np.full(H, bool(mean == 0)) | (score <= np.float32(tau))
    count = int(mask.sum())
    return score, mask, count, np.float32(np.float64(count) / np.float64(H))


def rule(param, fresh, r=None, c=None):
    """One tensor of a trunk under the rule: ``param`` / ``fresh`` [rows][cols] or [rows]; ``r`` [rows] / ``c`` [cols]
    bool or None.  Returns (the new tensor, the bool array of the elements written); unwritten elements keep their
    bits."""
    param, fresh = np.asarray(param), np.asarray(fresh)
    rows = param.shape[0]
    r = np.zeros(rows, bool) if r is None else np.asarray(r, bool)
    if param.ndim == 1:
        assert c is None
        written = r.copy()
        value = fresh
    else:
        c = np.zeros(param.shape[1], bool) if c is None else np.asarray(c, bool)
        written = r[:, None] | c[None, :]
        value = np.where(c[None, :], np.float32(0.0), fresh)
    out = param.copy()
    out[written] = value[written]
    return out, written


def recycle(param, m, v, fresh, r=None, c=None):
    """``rule`` with the moments: (param', m', v', written)."""
    out, written = rule(param, fresh, r, c)
    m2, v2 = np.asarray(m).copy(), np.asarray(v).copy()
    m2[written] = 0.0
    v2[written] = 0.0
    return out, m2, v2, written


def trunk_masks(named_shapes, h1, h2):
    """{name -> (r, c)} for the parameters of a trunk ``Linear [LayerNorm] ReLU Linear [LayerNorm] ReLU Linear`` given
    as [(name, shape)] in module order, and its two hidden layers' masks.  A matrix is a Linear's weight; the vectors
    behind it (its bias, its LayerNorm's weight and bias) share its row mask.  The last Linear has no row mask: its
    bias maps to (None, None) and is never written."""
    hidden, out, k = (h1, h2), {}, -1
    for name, shape in named_shapes:
        if len(shape) == 2:
            k += 1
            out[name] = (hidden[k] if k < 2 else None, hidden[k - 1] if k > 0 else None)
        else:
            out[name] = (hidden[k] if k < 2 else None, None)
    assert k == 2, "a 3-layer MLP"
    return out
