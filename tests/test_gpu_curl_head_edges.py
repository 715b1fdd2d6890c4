"""The one-launch CURL head (curl_head_kernel<NTILE>, entry curla_curl_head) on the MI355X, stage by stage against the
float64 references of tests/_curl_head_ref.py (checked on the CPU by tests/test_curl_head_ref_host.py): every NTILE =
B / 128 from 1 to 8 (phase B's preloaded operand, its runs of 4 and of 8 k-steps), F = 49 .. 52 (every tail lane of
fix_bv, the moved k run of phase A), a planted row maximum on the diagonal, in the next column, in the next wave's
tile, in the same wave's next i tile and round the corner, logits of scale 3, 40 and 300 (the last overflow expf
without the max subtraction; on the diagonal the last two are the trained-encoder regime, dlogits next to 0), gamma
with zeros and negative entries; a head whose logits are all equal, twin columns, a constant fc row, a zero anchor row,
a NaN that must stay in its row and its block, and the shapes the entry point refuses.

Every output is NaN before the launch with five NaN floats behind it that must still be NaN after it; every operand is
a view into a NaN-filled buffer, in one case per F at an odd float offset (the kernel's 16-byte loads promise 4-byte
alignment only).  Every stage is held to its own derived bound, n * 2^-24 * S element by element, against a float64
reference that starts from the kernel's float32 output of the stage before (tests/_curl_head_ref.py has the counts);
the sums that the fc backward's extra workgroup finishes (dgamma, dbeta, dbias, dW) likewise.  Every measured error
goes, with its bound, into the kernel parity report, a group per stage.

Measured on the MI355X (worst error / bound per stage, 163 tests in 5 s): logits 0.08; row_loss 0.03; dlogits 0.30 -- at
B = 896, the rounding of 1 / B (the float32 CPU evaluation has the same 0.30 at the same case); loss 0.01; dz 0.14;
w_partial 0.10; dfc 0.09; ln_partial 0.20; dgamma 0.16, dbeta 0.13, dbias 0.16, dW 0.19.  No stage of the kernel is
outside its bound anywhere; the float32 CPU evaluation's worst are 0.30 (dz, dlogits) and 0.28 (ln_partial)."""
import math

import pytest
import torch

from tests import _curl_head_ref as H
from tests import test_gpu_loss_head_edges as E
from tests.test_gpu_kernels import REPORT as PARITY_LINES, _report as _kernel_parity_report  # noqa: F401

pytestmark = pytest.mark.gpu

TAIL = E.TAIL
K_FC = 64  # the fc backward that finishes the partial sums
OUTPUTS = ("row_loss", "dfc", "ln_partial", "w_partial", "logits", "dlogits", "dz", "loss")
OPTIONAL = ("logits", "dlogits", "dz")


@pytest.fixture(scope="module", autouse=True)
def _report(_kernel_parity_report):
    """This module's lines for the kernel parity report (tests/test_gpu_loss_head_edges.py has the route: set up behind
    the report's writer, so torn down in front of it).  within / record are that module's and append to its list: what
    this module appended is taken out again here."""
    start = len(E.REPORT)
    yield
    mine = E.REPORT[start:]
    del E.REPORT[start:]
    worst = {}
    for grp, n, e, b in mine:
        PARITY_LINES.append((f"curl_head {grp} {n} (bound {b:.3e})", e))
        r = e / b if b > 0 else (0.0 if e == 0 else float("inf"))
        if r >= worst.get(grp, (-1.0,))[0]:
            worst[grp] = (r, n, e, b)
    for grp in H.STAGES:
        if grp in worst:
            r, n, e, b = worst[grp]
            print(f"curl_head edges, {grp}: worst error / bound {r:.3f} ({n}: {e:.3e} of {b:.3e})")
            PARITY_LINES.append((f"curl_head edges, {grp}: worst error / bound, at {n}", r))


@pytest.fixture(scope="module")
def ops():
    from curla_amd import ops as o
    return o


def guarded(t, odd=False):
    """t on the device as a view into a NaN-filled buffer: 8 (odd: 9) NaN floats in front of it, 7 behind."""
    off = 9 if odd else 8
    buf = E.nan(off + t.numel() + 7)
    buf[off:off + t.numel()] = t.reshape(-1).cuda()
    return buf[off:off + t.numel()].view(t.shape)


def sizes(B, Fd):
    return dict(row_loss=B, dfc=B * Fd, ln_partial=(B // 16) * 3 * Fd, w_partial=(B // 16) * Fd * Fd, logits=B * B,
                dlogits=B * B, dz=B * Fd, loss=1)


def shapes(B, Fd):
    return dict(row_loss=(B,), dfc=(B, Fd), ln_partial=(B // 16, 3, Fd), w_partial=(B // 16, Fd, Fd), logits=(B, B),
                dlogits=(B, B), dz=(B, Fd), loss=(1,))


def launch(ops, dinp, B, Fd, optional=True, sums=None):
    """One launch into NaN-prefilled outputs with NaN tails.  Returns ({name: the whole buffer}, the fc-backward token)."""
    n = sizes(B, Fd)
    bufs = {k: E.nan(n[k] + TAIL) for k in OUTPUTS if optional or k not in OPTIONAL}
    s = sums if sums is not None else dict(dgamma=E.nan(Fd + TAIL), dbeta=E.nan(Fd + TAIL), dbias=E.nan(Fd + TAIL),
                                          dW=E.nan(Fd * Fd + TAIL))
    tok = ops.curl_head(*dinp, B, Fd, bufs["row_loss"], bufs["dfc"], bufs["ln_partial"], bufs["w_partial"], s["dgamma"],
                        s["dbeta"], s["dbias"], s["dW"], loss=bufs["loss"], **{k: bufs.get(k) for k in OPTIONAL})
    return bufs, tok, s


def trimmed(bufs, B, Fd, finite=True):
    """The outputs without their tails, after checking that the tails are still NaN and (finite) no NaN is left inside."""
    n, sh = sizes(B, Fd), shapes(B, Fd)
    out = {}
    for k, v in bufs.items():
        assert E.all_nan(v[n[k]:]), f"{k}: the tail was written"
        out[k] = v[:n[k]].view(sh[k])
        if finite:
            assert bool(torch.isfinite(out[k]).all()), f"{k}: not finite"
    return out


def run_case(ops, inp, tag, odd=False):
    """The whole per-case protocol on the CPU tensors inp; returns the outputs (device tensors, sums included)."""
    z_a = inp[0]
    B, Fd = z_a.shape
    dinp = tuple(guarded(t, odd) for t in inp)
    bufs, tok, s = launch(ops, dinp, B, Fd)
    out = trimmed(bufs, B, Fd)
    assert all(E.all_nan(v) for v in s.values())  # finished by the fc backward, not here
    # the fc backward that follows in the agent finishes the sums (any activations will do)
    g = torch.Generator().manual_seed(B + Fd)
    Wfc, x = (torch.randn(Fd, K_FC, generator=g) * 0.1).cuda(), torch.relu(torch.randn(B, K_FC, generator=g)).cuda()
    gx, dwfc = E.nan(B * K_FC + TAIL), E.nan(Fd * K_FC + TAIL)
    ops.fc_bwd(out["dfc"], Wfc, x, gx, dwfc, B, Fd, K_FC, ln=tok)
    assert E.all_nan(gx[B * K_FC:]) and E.all_nan(dwfc[Fd * K_FC:])
    for k, v in s.items():
        m = Fd * Fd if k == "dW" else Fd
        assert E.all_nan(v[m:]), f"{k}: the tail was written"
        out[k] = v[:m].view((Fd, Fd) if k == "dW" else (Fd,))
    cpu = {k: v.cpu() for k, v in out.items()}
    for stage, got, ref, bound in H.stage_checks(inp, cpu):
        E.within(stage, f"{tag}", got, ref, bound)
    # without the three optional outputs: the same bits
    bufs2, _, _ = launch(ops, dinp, B, Fd, optional=False, sums=s)
    assert set(bufs2) == set(OUTPUTS) - set(OPTIONAL)
    for k, v in bufs2.items():
        assert E.bits_equal(v, bufs[k]), f"{k} differs without the optional outputs"
    for t, d in zip(inp, dinp):  # the operands were only read
        assert torch.equal(d.cpu(), t)
    return out


def _id(case):
    B, Fd, sh, sc = case
    return f"B{B}-F{Fd}-shift{sh}-x{sc:g}"


@pytest.mark.parametrize("case", H.CASES, ids=_id)
def test_curl_head_stages(ops, case):
    assert ops.curl_head_supported(case[0], case[1])
    run_case(ops, H.case_inputs(case), _id(case), odd=H.odd_offset(*case))


@pytest.mark.parametrize("B,Fd", H.SPECIAL_SHAPES)
def test_curl_head_uniform(ops, B, Fd):
    """wz = 0: every logit exactly 0, every row loss log B within its bound, every dz and dfc element exactly zero."""
    inp = H.special_inputs("uniform", B, Fd, seed=B)
    out = run_case(ops, inp, f"uniform B{B} F{Fd}")
    assert not bool(out["logits"].any())
    ref = torch.full((B,), math.log(B), dtype=torch.float64)
    E.within("row_loss", f"uniform B{B} F{Fd} vs log B", out["row_loss"], ref, H.ref_ce(out["logits"].cpu())[1]["row_loss"])
    assert not bool(out["dz"].any()) and not bool(out["dfc"].any())


@pytest.mark.parametrize("B,Fd", H.SPECIAL_SHAPES)
def test_curl_head_twins(ops, B, Fd):
    """Columns j and j' with identical wz and z_pos rows, in different waves' tiles and in different i tiles of one
    wave: their logits are bit-equal, and their dlogits in every row but j and j' (whose diagonal the identity takes)."""
    inp = H.special_inputs("twins", B, Fd, seed=B)
    out = run_case(ops, inp, f"twins B{B} F{Fd}")
    j = H.TWIN_J
    for j2 in H.twin_partners(B):
        assert torch.equal(out["logits"][:, j], out["logits"][:, j2])
        rows = torch.ones(B, dtype=torch.bool, device="cuda")
        rows[[j, j2]] = False
        assert torch.equal(out["dlogits"][rows, j], out["dlogits"][rows, j2])


@pytest.mark.parametrize("kind", ["flat_row", "zero_row"])
@pytest.mark.parametrize("B,Fd", H.SPECIAL_SHAPES)
def test_curl_head_degenerate_rows(ops, B, Fd, kind):
    inp = H.special_inputs(kind, B, Fd, seed=B)
    out = run_case(ops, inp, f"{kind} B{B} F{Fd}")
    if kind == "zero_row":  # its logits are exactly 0
        assert not bool(out["logits"][H.SPECIAL_ROW].any())


@pytest.mark.parametrize("B,Fd", H.SPECIAL_SHAPES)
def test_curl_head_nan_stays_in_its_row(ops, B, Fd):
    """One NaN in row r of z_a: row r's outputs are not finite, every other row of row_loss, logits, dlogits, dz, dfc
    and every other block's partials are the clean run's, bit for bit."""
    inp = H.head_inputs(B, Fd, 16, 3.0, seed=B + 1)
    r, blk = B - 7, (B - 7) // 16
    dinp = tuple(guarded(t) for t in inp)
    clean = trimmed(launch(ops, dinp, B, Fd)[0], B, Fd)
    dirty_za = inp[0].clone()
    dirty_za[r, 7] = float("nan")
    dirty = trimmed(launch(ops, (guarded(dirty_za),) + dinp[1:], B, Fd)[0], B, Fd, finite=False)
    others = torch.ones(B, dtype=torch.bool, device="cuda")
    others[r] = False
    for k in ("row_loss", "logits", "dlogits", "dz", "dfc"):
        assert not bool(torch.isfinite(dirty[k][r]).any()), f"{k}: a finite value in the NaN row"
        assert torch.equal(dirty[k][others], clean[k][others]), f"{k}: another row changed"
    oblk = torch.ones(B // 16, dtype=torch.bool, device="cuda")
    oblk[blk] = False
    for k in ("ln_partial", "w_partial"):
        assert not bool(torch.isfinite(dirty[k][blk]).any()), f"{k}: a finite value in the NaN row's block"
        assert torch.equal(dirty[k][oblk], clean[k][oblk]), f"{k}: another block changed"
    assert not bool(torch.isfinite(dirty["loss"]).any())


@pytest.mark.parametrize("B,Fd", [(64, 50), (192, 50), (1152, 50), (128, 48), (128, 53)])
def test_curl_head_refusals(ops, B, Fd):
    from curla_amd._lib import CurlaHipError
    assert not ops.curl_head_supported(B, Fd)
    g = torch.Generator().manual_seed(B)
    inp = tuple(torch.randn(*s, generator=g) for s in ((B, Fd), (B, Fd), (B, Fd), (B, Fd), (B,), (Fd,)))
    n = sizes(B, Fd)
    n["ln_partial"], n["w_partial"] = (B // 16 + 1) * 3 * Fd, (B // 16 + 1) * Fd * Fd
    bufs = {k: E.nan(n[k] + TAIL) for k in OUTPUTS}
    s = [E.nan(Fd), E.nan(Fd), E.nan(Fd), E.nan(Fd * Fd)]
    with pytest.raises(CurlaHipError):
        ops.curl_head(*(t.cuda() for t in inp), B, Fd, bufs["row_loss"], bufs["dfc"], bufs["ln_partial"], bufs["w_partial"], *s,
                      loss=bufs["loss"], **{k: bufs[k] for k in OPTIONAL})
    torch.cuda.synchronize()
    assert all(E.all_nan(v) for v in bufs.values()) and all(E.all_nan(v) for v in s)
