"""tests/_curl_head_ref.py checked on the CPU, before any kernel is involved: the stage references chained in float64
against float64 autograd through LayerNorm -> z_a W z_pos^T -> cross_entropy; the input builder's conditions at every
case tests/test_gpu_curl_head_edges.py runs; the case list's coverage; the derived bounds shown passable by a correct
float32 evaluation (torch on the CPU) and not vacuous: each of seven heads that are wrong in one place exceeds one."""
import functools

import pytest
import torch

from tests import _curl_head_ref as H
from tests import _loss_head_ref as R

EXACT = 1e-12  # two float64 statements of one quantity, relative to its scale


@functools.lru_cache(maxsize=None)
def _inputs(case):
    return H.case_inputs(case)


@pytest.mark.parametrize("B,Fd", [(16, 5), (128, 50), (256, 49)])
def test_stages_compose_to_autograd(B, Fd):
    g = torch.Generator().manual_seed(B + Fd)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    args = (2 * r(B, Fd) + 0.5, 1 + 0.1 * r(Fd), 0.1 * r(Fd), torch.rand(Fd, Fd, generator=g, dtype=torch.float64), 0.7 * r(B, Fd))
    got, want = H.chain64(*args), H.autograd64(*args)
    for k, w in want.items():
        scale = max(float(w.abs().max()), 1e-300)
        assert float((got[k] - w).abs().max()) <= EXACT * scale, (k, float((got[k] - w).abs().max()), scale)


def test_case_list_coverage():
    cases = H.CASES
    assert len(set(cases)) == len(cases)
    ntile = lambda B: B // 128  # noqa: E731
    assert {ntile(B) for B, *_ in cases} == set(range(1, 9))
    for B in H.FULL_BS:  # the full cross
        assert {c[1:] for c in cases if c[0] == B} == {(Fd, sh, sc) for Fd in H.FS for sh in H.shifts(B) for sc in H.SCALES}
    assert {(ntile(B), Fd) for B, Fd, _, _ in cases} == {(n, Fd) for n in range(1, 9) for Fd in H.FS}
    assert {(B, sh) for B, _, sh, _ in cases} == {(B, sh) for B in H.BS for sh in H.shifts(B)}
    assert {(Fd, sc) for B, Fd, _, sc in cases if B not in H.FULL_BS} == {(Fd, sc) for Fd in H.FS for sc in H.SCALES}
    assert {ntile(B) for B, _, _, sc in cases if sc == 300.0} == set(range(1, 9))
    for B in H.BS:
        assert H.shifts(B) == ((0, 1, 16, 128, B - 1) if B >= 256 else (0, 1, 16, 127))
    assert sorted(c[1] for c in cases if H.odd_offset(*c)) == list(H.FS)  # one odd-offset case per F
    assert sorted(Fd for _, Fd in H.SPECIAL_SHAPES) == list(H.FS)
    assert all(B in H.BS for B, _ in H.SPECIAL_SHAPES) and any(B >= 256 for B, _ in H.SPECIAL_SHAPES)


@pytest.mark.parametrize("B", H.BS)
def test_builder_conditions(B):
    for case in (c for c in H.CASES if c[0] == B):
        _, Fd, shift, scale = case
        z_a, z_pos, wz, xhat, rstd, gamma = _inputs(case)
        assert all(t.dtype == torch.float32 and bool(torch.isfinite(t).all()) for t in (z_a, z_pos, wz, xhat, rstd, gamma))
        assert z_a.shape == z_pos.shape == wz.shape == xhat.shape == (B, Fd) and rstd.shape == (B,) and gamma.shape == (Fd,)
        neg = [f for f in range(3, Fd, 11) if f % 7]  # (feature 14 is both: a zero)
        assert bool((gamma[::7] == 0).all()) and bool((gamma[neg] < 0).all()) and int((gamma < 0).sum()) == len(neg) == 4
        logits = R.f64(z_a) @ R.f64(wz).t()
        planted = (torch.arange(B) + shift) % B
        assert torch.equal(logits.argmax(1), planted), case
        top2 = logits.topk(2, dim=1).values
        gap = float((top2[:, 0] - top2[:, 1]).min())
        if scale == 3.0:
            assert gap >= 0.5, (case, gap)
        if scale == 300.0:
            assert float(logits.max()) > 89.0  # expf of it overflows: what the max subtraction is for
        if shift == 0 and scale >= 40.0:
            assert float(R.curl_ce(logits)["row_loss"].max()) < 1e-6, case  # the trained-encoder regime


@pytest.mark.parametrize("B,Fd", H.SPECIAL_SHAPES)
def test_special_inputs(B, Fd):
    bits = lambda t: t.view(torch.int32)  # noqa: E731
    z_a, z_pos, wz, *_ = H.special_inputs("uniform", B, Fd, seed=B)
    lg = z_a @ wz.t()
    assert not bool(wz.any()) and not bool(lg.any())
    assert torch.equal(bits(lg[:, :1].expand(B, B).contiguous()), bits(lg))  # bit-equal logits in float32
    z_a, z_pos, wz, *_ = H.special_inputs("twins", B, Fd, seed=B)
    assert len(H.twin_partners(B)) == (2 if B >= 256 else 1)
    for j2 in H.twin_partners(B):
        assert (j2 // 16) % 8 != (H.TWIN_J // 16) % 8 or j2 - H.TWIN_J == 128  # another wave's tile, or the wave's next i tile
        assert torch.equal(bits(wz[j2]), bits(wz[H.TWIN_J])) and torch.equal(bits(z_pos[j2]), bits(z_pos[H.TWIN_J]))
        lg = z_a @ wz.t()
        assert torch.equal(bits(lg[:, j2].contiguous()), bits(lg[:, H.TWIN_J].contiguous()))
    z_a, _, _, xhat, rstd, _ = H.special_inputs("flat_row", B, Fd, seed=B)
    r = H.SPECIAL_ROW
    assert not bool(xhat[r].any()) and float(rstd[r]) == pytest.approx(1e-5 ** -0.5, rel=1e-7) and float(z_a[r].abs().max()) < 1
    z_a, *_ = H.special_inputs("zero_row", B, Fd, seed=B)
    assert not bool(z_a[r].any()) and bool(z_a[r - 1].any())


@pytest.mark.parametrize("B", H.BS)
def test_float32_evaluation_passes_every_bound(B):
    """A correct float32 head (torch on the CPU) is inside every bound at every case and every special input."""
    runs = [(c, _inputs(c)) for c in H.CASES if c[0] == B]
    runs += [((kind, B, Fd), H.special_inputs(kind, B, Fd, seed=B)) for B2, Fd in H.SPECIAL_SHAPES if B2 == B for kind in H.SPECIALS]
    worst = {}
    for case, inp in runs:
        for stage, ratio in H.ratios(inp, H.eval32(inp)).items():
            if ratio > worst.get(stage, (0.0,))[0]:
                worst[stage] = (ratio, case)
            assert ratio <= 1.0, (case, stage, ratio)
    print(f"float32 CPU head at B = {B}, worst error / bound: " + ", ".join(f"{s} {worst[s][0]:.3f}" for s in H.STAGES if s in worst))


# the cases the wrong heads are run at: every F, both ends of the batch range, a maximum on and off the diagonal
MUTANT_CASES = [c for c in H.CASES if c in {(128, 49, 0, 3.0), (128, 50, 1, 40.0), (128, 51, 16, 300.0), (128, 52, 127, 3.0),
                                            (640, 50, 128, 300.0), (1024, 52, 1023, 3.0)}]


@pytest.mark.parametrize("variant", H.VARIANTS)
def test_a_wrong_head_exceeds_a_bound(variant):
    """Each of the seven wrong heads is outside at least one bound at at least one case -- and at the stage that is
    wrong: every stage's reference starts from the head's own output of the stage before."""
    assert len(MUTANT_CASES) == 6
    stage_of = dict(drop_k={"logits"}, no_max={"row_loss", "dlogits", "loss"}, shifted_identity={"dlogits"},
                    inv_b_minus_1={"dlogits"}, z_pos_in_dz={"dz"}, w_partial_transposed={"w_partial"}, no_m2={"dfc"})[variant]
    worst = 0.0
    for case in MUTANT_CASES:
        inp = _inputs(case)
        for stage, ratio in H.ratios(inp, H.eval32(inp, variant)).items():
            if stage in stage_of:
                worst = max(worst, ratio)
            elif variant != "no_max":  # (an overflowed row leaves NaN in everything behind it)
                assert ratio <= 1.0, (variant, case, stage, ratio)  # nothing else is charged with it
    print(f"{variant}: worst error / bound {worst:.3g}")
    assert worst > 1.0, (variant, worst)
