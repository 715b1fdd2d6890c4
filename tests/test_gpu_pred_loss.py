"""``curla_pred_loss`` (csrc/pred_loss.h) on the MI355X against the float64 reference of tests/_pred_ref.py.

Shapes: B in {1, 2, 67} (less than a workgroup's four rows; a second, partly filled workgroup and B no multiple of any
block size) x F in {1, 50, 63, 64, 65, 200, 1024} (a partial wave, an exact one, one element past it, the stride loop's
last partial trip, the widest latent).  Inputs: _pred_ref.inputs -- normal rows with entries to about 1e3 and the
hand-made rows p = t, p = -t, p orthogonal to t, p zero, t zero, a row scaled by 1e-6 and one by 1e6.

Tolerance: not a number chosen here.  The same definition is evaluated by torch in float32 on the CPU on the same inputs;
its largest error against float64 per F (over the three batch sizes: the row loss in absolute terms, dp per row relative
to the row's largest |dp|, or to the size of a gradient at unit distance where the exact gradient vanishes --
_pred_ref.errors) is float32's own error on this formula, and the kernel, whose reductions run in another order, is
allowed 4x that.  Every figure is printed before it is asserted.

Every buffer the kernel touches lies between NaN guards: a read outside [B, F] would poison an output, a write outside
would overwrite a guard."""
import functools

import numpy as np
import pytest
import torch

from tests import _pred_ref as R

pytestmark = pytest.mark.gpu

BATCHES = (1, 2, 67)
WIDTHS = (1, 50, 63, 64, 65, 200, 1024)
LEAD, TAIL = 3, 5  # NaN floats in front of and behind every buffer
FACTOR = 4.0


@functools.lru_cache(maxsize=None)
def case(B, Fd):
    """(p, t, hand rows, float64 reference, float32 CPU errors) of one shape, computed once."""
    p, t, where = R.inputs(B, Fd)
    ref = R.loss(p, t)
    rows32, _, dp32 = R.loss(p, t, torch.float32)
    return p, t, where, ref, R.errors(rows32, dp32, ref[0], ref[2], p)


@functools.lru_cache(maxsize=None)
def bound(Fd):
    """4x the float32 CPU evaluation's largest errors at this width, over the batch sizes: (row_loss, dp)."""
    errs = [case(B, Fd)[4] for B in BATCHES]
    return FACTOR * max(e[0] for e in errs), FACTOR * max(e[1] for e in errs)


def guarded(values=None, n=None):
    """A NaN-filled device buffer with ``values`` (or n NaN floats) between LEAD and TAIL guard floats: (buffer, view)."""
    n = values.numel() if values is not None else n
    buf = torch.full((LEAD + n + TAIL,), float("nan"), dtype=torch.float32, device="cuda")
    view = buf[LEAD:LEAD + n]
    if values is not None:
        view.copy_(values.reshape(-1))
    return buf, view


def guards_intact(buf):
    return bool(torch.isnan(buf[:LEAD]).all()) and bool(torch.isnan(buf[-TAIL:]).all())


def run(p, t, with_total=True):
    from curla_amd import ops
    B, Fd = p.shape
    bufs = [guarded(p), guarded(t), guarded(n=B), guarded(n=1), guarded(n=B * Fd)]
    (_, dp_), (_, dt_), (_, rows), (_, total), (_, dp) = bufs
    ops.pred_loss(dp_, dt_, B, Fd, rows, total if with_total else None, dp)
    torch.cuda.synchronize()
    assert all(guards_intact(b) for b, _ in bufs), "a guard float was overwritten"
    same_bits = lambda a, b: torch.equal(a.cpu().view(torch.int32), b.reshape(-1).view(torch.int32))  # noqa: E731
    assert same_bits(dp_, p) and same_bits(dt_, t)  # (the inputs are read only; bits, so that a NaN input compares)
    return rows.cpu(), total.cpu(), dp.cpu().view(B, Fd)


@pytest.mark.parametrize("Fd", WIDTHS)
@pytest.mark.parametrize("B", BATCHES)
def test_kernel_against_float64(B, Fd):
    p, t, where, (ref_rows, ref_total, ref_dp), cpu32 = case(B, Fd)
    b_rows, b_dp = bound(Fd)
    rows, total, dp = run(p, t)
    e_rows, e_dp = R.errors(rows, dp, ref_rows, ref_dp, p)
    print(f"B{B} F{Fd}: row_loss {e_rows:.3e} (float32 CPU {cpu32[0]:.3e}, bound {b_rows:.3e}); "
          f"dp {e_dp:.3e} (float32 CPU {cpu32[1]:.3e}, bound {b_dp:.3e})")
    assert bool(torch.isfinite(rows).all()) and bool(torch.isfinite(dp).all())  # (the zero rows included)
    assert e_rows <= b_rows and e_dp <= b_dp
    # the mean over rows: curla_mean's order on the kernel's own row losses, bit for bit
    assert np.float32(total.item()) == R.fixed_order_mean(rows.numpy())
    # (the rows' own errors on average, and the mean's: 6 butterfly steps, 2 across the waves and the division, each one
    # rounding of a partial sum of at most 4 per row summed -- 12 x 2^-24 x 4 is above all of them)
    assert abs(float(total) - float(ref_total)) <= b_rows + 12 * 2.0 ** -24 * 4
    # the hand-made rows
    if "p_is_t" in where:
        b = where["p_is_t"]
        assert float(rows[b]) == 0.0 and not bool(dp[b].any())  # (ph == th bit for bit: d = 0 exactly)
    if "p_is_minus_t" in where:
        assert abs(float(rows[where["p_is_minus_t"]]) - 4.0) <= b_rows
    if "orthogonal" in where and Fd >= 2:
        assert abs(float(rows[where["orthogonal"]]) - 2.0) <= b_rows
    if "p_zero" in where:  # loss |th|^2 = 1, gradient (2 / B)(-th) / eps: large, finite
        b = where["p_zero"]
        assert abs(float(rows[b]) - 1.0) <= b_rows and float(dp[b].abs().max()) > 1e6
    if "t_zero" in where:
        assert abs(float(rows[where["t_zero"]]) - 1.0) <= b_rows
    # reruns write the same bits; without the total pointer the rows and the gradient are the same and it stays untouched
    rows2, total2, dp2 = run(p, t)
    assert torch.equal(rows, rows2) and torch.equal(dp, dp2) and torch.equal(total, total2)
    rows3, total3, dp3 = run(p, t, with_total=False)
    assert torch.equal(rows, rows3) and torch.equal(dp, dp3) and bool(torch.isnan(total3).all())


@pytest.mark.parametrize("Fd", [50, 65])
def test_the_loss_does_not_depend_on_the_scale_of_p(Fd):
    p, t, where, (ref_rows, _, _), _ = case(67, Fd)
    rows, _, _ = run(p, t)
    for name, s in (("scaled_down", 1e6), ("scaled_up", 1e-6)):
        b = where[name]
        q = p.clone()
        q[b] *= s  # (back to the row's original scale, up to the rounding of the two multiplications)
        rows_q, _, _ = run(q, t)
        # (each is within the bound of its exact value; the two roundings move the direction by at most 2^-23: 2^-21 in
        # a loss whose gradient in the direction is at most 4)
        assert abs(float(rows[b]) - float(rows_q[b])) <= 2 * bound(Fd)[0] + 2.0 ** -21


@pytest.mark.parametrize("value", [float("nan"), float("inf")])
@pytest.mark.parametrize("in_t", [False, True])
def test_a_non_finite_input_stays_in_its_row(value, in_t):
    B, Fd, b = 67, 65, 5
    p, t, _, _, _ = case(B, Fd)
    rows, total, dp = run(p, t)
    p2, t2 = p.clone(), t.clone()
    (t2 if in_t else p2)[b, 64] = value  # (the one element past the wave)
    rows2, total2, dp2 = run(p2, t2)
    keep = torch.arange(B) != b
    assert torch.equal(rows[keep], rows2[keep]) and torch.equal(dp[keep], dp2[keep])
    assert not bool(torch.isfinite(rows2[b])) and not bool(torch.isfinite(dp2[b]).any())
    assert not bool(torch.isfinite(total2).any())  # (the mean sees the row)


@pytest.mark.parametrize("B", [255, 257, 515])
def test_total_past_one_trip_of_the_mean(B):
    """More rows than curla_mean's 256 threads: its stride loop, against the restatement bit for bit."""
    p, t, _ = R.inputs(B, 50)
    ref_rows, ref_total, ref_dp = R.loss(p, t)
    rows, total, dp = run(p, t)
    assert np.float32(total.item()) == R.fixed_order_mean(rows.numpy())
    e_rows, e_dp = R.errors(rows, dp, ref_rows, ref_dp, p)
    assert e_rows <= bound(50)[0] and e_dp <= bound(50)[1]


def test_arguments_are_checked_before_any_launch():
    from curla_amd import _lib
    lib = _lib.load()
    a = 4096  # a non-NULL address that is never dereferenced
    ok = dict(p=a, t=a, B=4, F=50, rows=a, total=None, dp=a)
    for bad in (dict(p=None), dict(t=None), dict(rows=None), dict(dp=None), dict(B=0), dict(B=-1), dict(F=0), dict(F=1025)):
        k = {**ok, **bad}
        assert lib.curla_pred_loss(k["p"], k["t"], k["B"], k["F"], k["rows"], k["total"], k["dp"], None) == -1, bad
