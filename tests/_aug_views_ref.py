"""Float64 statements of the two ``aug_views = 2`` kernels -- the TD loss that averages the targets of a transition's two
views (curla_critic_td_loss_views) and the InfoNCE that does not count a position's partner among its negatives
(curla_curl_ce_views) --, their input builders and their error bounds, in the manner of tests/_loss_head_ref.py, whose
helpers they are built from.  CPU only; checked by tests/test_aug_views_host.py against torch's own mse_loss and
cross_entropy.

A minibatch of B positions (B even, H = B / 2) holds H transitions, each at positions b and b + H under two independent
augmentations (DrQ, Kostrikov et al. 2021, K = 2 and M = 2).

Bounds, derived as there (|got - ref64| <= n * 2^-24 * S, n = twice the float32 roundings):
  tbar      each view's target carries R.N_TARGET relative to its own magnitudes S_b; their sum rounds once more, relative
            to at most S_b + S_b'; the multiply by 0.5 is exact: (R.N_TARGET + 1) * U * 0.5 (S_b + S_b').
  dq        2 (q - tbar) (1 / H) on the float32 tbar the kernel wrote: R.N_CRITIC_DQ and one rounding more,
            relative to 2 (|q| + |tbar|) / H.
  loss      a float32 sum over the batch divided by H: R.scalar_bound of the H per-transition summands (the four squares of
            a transition; a thread adds two per pass, 2 ceil(H / 256) <= 6 serial adds at B <= 1030, inside that bound's
            count).
  InfoNCE   R.curl_ce_bounds of the logits with the partner entries at -inf: the kernel's sums have one term fewer than
            that bound counts, nothing else differs."""
import torch
import torch.nn.functional as F

from tests import _loss_head_ref as R

F64 = R.F64
N_TARGET_VIEWS = R.N_TARGET + 1
N_CRITIC_DQ_VIEWS = R.N_CRITIC_DQ + 1


def partner(B, device=None):
    """Row a's partner column (a + B / 2) % B, for every row."""
    return (torch.arange(B, device=device) + B // 2) % B


# ------------------------------------------------------------------------------------------------ the TD loss
def views_target(tq1, tq2, log_pi, reward, not_done, log_alpha, discount):
    """tbar[b] = tbar[b + H] = 0.5 (t_b + t_{b + H}), t = R.td_target's.  Returns (tbar [B], Sbar [B]): Sbar the mean of
    the two views' magnitudes."""
    t, S = R.td_target(tq1, tq2, log_pi, reward, not_done, log_alpha, discount)
    H = t.numel() // 2
    assert t.numel() == 2 * H
    tbar = 0.5 * (t[:H] + t[H:])
    Sbar = 0.5 * (S[:H] + S[H:])
    return torch.cat([tbar, tbar]), torch.cat([Sbar, Sbar])


def views_critic_loss(q1, q2, tbar):
    """loss = (1 / H) sum over the B positions and both twins of (q - tbar)^2, dq = d loss / d q by autograd (tbar is a
    constant, as the reference's no_grad target is).  Returns dict(loss, terms [H] = the summands per transition,
    dq [2, B], dq_S [2, B] = 2 (|q_i| + |tbar|) / H)."""
    q = torch.stack([R.f64(q1).reshape(-1), R.f64(q2).reshape(-1)]).requires_grad_(True)
    t = R.f64(tbar).reshape(-1)
    B = t.numel()
    H = B // 2
    sq = ((q - t) ** 2).sum(0)
    terms = sq[:H] + sq[H:]
    loss = terms.sum() / H
    dq, = torch.autograd.grad(loss, q)
    qd = q.detach()
    return dict(loss=loss.detach(), terms=terms.detach(), dq=dq, dq_S=2 * (qd.abs() + t.abs()) / H)


def views_bounds_target(Sbar):
    return N_TARGET_VIEWS * R.U * Sbar


def views_bounds_dq(ref):
    return N_CRITIC_DQ_VIEWS * R.U * ref["dq_S"]


def mirrored(d):
    """R.loss_inputs' dict with the second half of every input a copy of the first (B even): both views identical."""
    B, stride = d["B"], d["stride"]
    H = B // 2
    out = dict(d)
    for k in ("q1", "q2", "tq1", "tq2", "log_pi", "reward", "not_done"):
        out[k] = torch.cat([d[k][:H], d[k][:H]])
    out["q"], out["tq"] = R.twin(out["q1"], out["q2"], stride), R.twin(out["tq1"], out["tq2"], stride)
    return out


# ------------------------------------------------------------------------------------------------ the InfoNCE
def without_partner(logits):
    """[B, B] -> ([B, B - 1], labels [B]): every row without its partner column, and where its diagonal entry went."""
    l = torch.as_tensor(logits)
    B = l.shape[0]
    p, a = partner(B, l.device), torch.arange(B, device=l.device)
    rows = l[a[None, :] != p[:, None]].reshape(B, B - 1)
    return rows, a - (p < a).long()


def curl_ce_views(logits):
    """cross_entropy over the logits with the partner column removed, row by row, and its gradient scattered back into
    [B, B] (the partner entries 0).  Returns dict(row_loss, loss, dlogits)."""
    l = R.f64(logits)
    B = l.shape[0]
    rows, labels = without_partner(l)
    rows = rows.clone().requires_grad_(True)
    row_loss = F.cross_entropy(rows, labels, reduction="none")
    loss = row_loss.mean()
    g, = torch.autograd.grad(loss, rows)
    dl = torch.zeros(B, B, dtype=F64)
    dl[torch.arange(B)[None, :] != partner(B)[:, None]] = g.reshape(-1)
    return dict(row_loss=row_loss.detach(), loss=loss.detach(), dlogits=dl)


def masked(logits):
    """A copy of the logits with the partner entries at -inf."""
    l = torch.as_tensor(logits).clone()
    B = l.shape[0]
    l[torch.arange(B), partner(B)] = float("-inf")
    return l


def curl_ce_views_bounds(logits):
    """R.curl_ce_bounds on the masked logits (|-inf| times the partner's p = 0 would be NaN: the entries are set to 0
    where only their magnitude is read -- they enter no sum)."""
    lm = masked(logits)
    ref = R.curl_ce(lm)
    finite = torch.where(torch.isinf(lm), torch.zeros_like(lm), lm)
    return R.curl_ce_bounds(ref, finite)
