"""Dormant-neuron scores and ReDo recycling on the MI355X, held to tests/_redo_ref.py.
The kernels alone: curla_dormant_colsum / curla_dormant_mask at B in {1, 3, 64, 257}, H in {4, 96, 1024}, one and two
networks, dense and strided inside NaN-filled guard buffers, signed inputs -- once with inputs whose sums are exact
(everything compared bit for bit) and once with random ones against float64 at RTOL, the masks exactly;
curla_redo_recycle against the NumPy rule bit for bit over whole guarded buffers.  The whole agent: two agents from one
seed with planted dead units, one with ``redo_interval``; they differ exactly where the rule writes."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _redo_ref as R
from tests._util import RTOL, rel_err
from tests.test_gpu_critic_ln import HP, NullLogger
from tests.test_gpu_reset import B, FLAT_OPTS, _assert_same, _bits, _seed, _state, make, nccl_world1, ring  # noqa: F401

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 16
SHAPES = [(b, h, nb) for b in (1, 3, 64, 257) for h in (4, 96, 1024) for nb in (1, 2)]


def _same(got, want):
    """Bit for bit, a NaN equal to any NaN (0 / 0 has no agreed sign or payload)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype
    if got.dtype.kind != "f":
        return np.array_equal(got, want)
    n = np.isnan(want)
    return np.array_equal(np.isnan(got), n) and np.array_equal(_bits(got[~n]), _bits(want[~n]))


# ---------------------------------------------------------------------------------------------- 1. colsum and mask alone
def _guarded(values, stride, lead=0):
    """values [n][k] at ``stride`` floats apart, ``lead`` floats off 16-byte alignment, in a NaN-filled device buffer
    with guard bands; returns (buffer, view of the first element on, host image)."""
    n, k = values.shape
    img = np.full(2 * GUARD + lead + (n - 1) * stride + k, NAN, np.float32)
    for i in range(n):
        img[GUARD + lead + i * stride:GUARD + lead + i * stride + k] = values[i]
    buf = torch.from_numpy(img).cuda()
    return buf, buf[GUARD + lead:], img


def _colsum(h, pad_h, pad_s, lead=0):
    """ops.dormant_colsum over h [nb][B][H]; the networks ``pad_h`` floats further apart than dense on the way in and
    ``pad_s`` on the way out.  Returns sums [nb][H] after checking that nothing else was written."""
    from curla_amd import ops
    nb, Bn, H = h.shape
    sh, ss = Bn * H + pad_h, H + pad_s
    _, hv, _ = _guarded(h.reshape(nb, Bn * H), sh, lead)
    out, ov, img = _guarded(np.full((nb, H), 7.0, np.float32), ss, lead)
    ops.dormant_colsum(hv, sh, nb, Bn, H, ov, ss)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    sums = np.stack([got[GUARD + lead + i * ss:GUARD + lead + i * ss + H] for i in range(nb)])
    for i in range(nb):
        img[GUARD + lead + i * ss:GUARD + lead + i * ss + H] = sums[i]
    assert np.array_equal(_bits(got), _bits(img)), "written outside sums"
    return sums


def _mask(sums, tau):
    """ops.dormant_mask over sums [L][H] in guarded buffers -> (score, mask, count, fraction)."""
    from curla_amd import ops
    L, H = sums.shape
    dev = torch.from_numpy(np.ascontiguousarray(sums)).cuda()
    score = torch.full((L * H + GUARD,), NAN, device="cuda")
    mask = torch.full((L * H + GUARD,), -7, device="cuda", dtype=torch.int32)
    count = torch.full((L + GUARD,), -7, device="cuda", dtype=torch.int32)
    frac = torch.full((L + GUARD,), NAN, device="cuda")
    ops.dormant_mask(dev, L, H, tau, score, mask, count, frac)
    torch.cuda.synchronize()
    assert torch.isnan(score[L * H:]).all() and torch.isnan(frac[L:]).all()
    assert bool((mask[L * H:] == -7).all()) and bool((count[L:] == -7).all())
    assert np.array_equal(_bits(dev.cpu().numpy()), _bits(sums)), "sums were written"
    return (score[:L * H].view(L, H).cpu().numpy(), mask[:L * H].view(L, H).cpu().numpy(), count[:L].cpu().numpy(),
            frac[:L].cpu().numpy())


def _ref_layers(sums, tau):
    out = [R.dormant(s, tau) for s in sums]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]).astype(np.int32),
            np.array([o[2] for o in out], np.int32), np.array([o[3] for o in out], np.float32))


def _exact_inputs(Bn, H, nb, seed):
    """Small integers times 2**-3: every float32 sum, the float64 totals and hence scores and masks are exact in any
    order.  Signed; some columns all zero, some a single small entry."""
    rs = np.random.RandomState(seed)
    h = (rs.randint(-8, 9, (nb, Bn, H)) * 0.125).astype(np.float32)
    h[:, :, rs.rand(H) < 0.2] = 0.0
    h[:, 1:, rs.rand(H) < 0.2] = 0.0
    return h


@pytest.mark.parametrize("Bn,H,nb", SHAPES)
def test_colsum_and_mask_on_exact_inputs_bit_for_bit(Bn, H, nb):
    h = _exact_inputs(Bn, H, nb, seed=Bn + H + nb)
    want = np.stack([R.colsum(x) for x in h])
    assert np.array_equal(want.astype(np.float64), np.abs(h.astype(np.float64)).sum(1)), "the inputs are not exact"
    for pad_h, pad_s, lead in ((0, 0, 0), (5, 3, 1)):
        sums = _colsum(h, pad_h, pad_s, lead)
        assert np.array_equal(_bits(sums), _bits(want)), (pad_h, pad_s, lead)
    assert np.array_equal(_bits(_colsum(h, 0, 0)), _bits(sums)), "a rerun changed bits"
    for tau in (0.0, 0.5, 1.0):
        got, ref = _mask(sums, tau), _ref_layers(sums, tau)
        for g, r, name in zip(got, ref, ("score", "mask", "count", "fraction")):
            assert _same(g, r), (name, tau)
        again = _mask(sums, tau)
        assert all(_same(a, g) for a, g in zip(again, got)), "a rerun changed bits"
        if tau == 0.0:
            assert np.array_equal(got[1] != 0, sums == 0)


def _random_inputs(Bn, H, nb, tau):
    """Signed normal activations, the columns scaled over four decades so that scores lie on both sides of ``tau``; the
    seed is the first (chosen here, on the host) at which no float64 reference score lies within 1e-5 relative of tau."""
    for seed in range(1000):
        rs = np.random.RandomState(1000 * seed + Bn + H + nb)
        h = (rs.randn(nb, Bn, H) * 10.0 ** rs.uniform(-3, 1, (nb, 1, H))).astype(np.float32)
        s64 = np.abs(h.astype(np.float64)).sum(1)
        score64 = s64 / s64.mean(1, keepdims=True)
        if np.abs(score64 - tau).min() <= 1e-5 * tau:
            continue
        # (and the definition's own float32 sums fall on the same sides: decided here, without the device)
        if all(np.array_equal(R.dormant(R.colsum(h[n]), tau)[1], score64[n] <= tau) for n in range(nb)):
            return h, s64, score64
    raise AssertionError("no seed")


@pytest.mark.parametrize("Bn,H,nb", SHAPES)
def test_colsum_and_mask_on_random_inputs_against_float64(Bn, H, nb):
    tau = 0.1
    h, s64, score64 = _random_inputs(Bn, H, nb, tau)
    assert np.abs(score64 - tau).min() > 1e-5 * tau
    mask64 = score64 <= tau
    assert H < 96 or (mask64.any() and not mask64.all())  # (wide layers: units on both sides of tau)
    for pad_h, pad_s, lead in ((0, 0, 0), (7, 1, 3)):
        sums = _colsum(h, pad_h, pad_s, lead)
        assert np.array_equal(_bits(sums), _bits(np.stack([R.colsum(x) for x in h])))  # the definition's order: exact
        for n in range(nb):
            e = rel_err(sums[n], s64[n])
            print("colsum B=%d H=%d network %d: rel %.2e" % (Bn, H, n, e))
            assert e <= RTOL
    score, mask, count, frac = _mask(sums, tau)
    for n in range(nb):
        e = rel_err(score[n], score64[n])
        print("score B=%d H=%d network %d: rel %.2e" % (Bn, H, n, e))
        assert e <= RTOL
    assert np.array_equal(mask != 0, mask64)
    assert np.array_equal(count, mask64.sum(1)) and np.array_equal(frac, (mask64.sum(1) / H).astype(np.float32))
    again = _mask(sums, tau)
    assert all(_same(a, g) for a, g in zip(again, (score, mask, count, frac))), "a rerun changed bits"


def test_a_zero_layer_and_a_nan_layer():
    """Total 0: every unit dormant whatever tau.  A NaN anywhere in a layer: its total is NaN, nothing is dormant."""
    h = _exact_inputs(3, 96, 2, seed=5)
    h[0] = 0.0
    h[1, 2, 17] = NAN
    sums = _colsum(h, 0, 0)
    assert not sums[0].any() and np.isnan(sums[1, 17]) and int(np.isnan(sums[1]).sum()) == 1
    for tau in (0.0, 0.1):
        score, mask, count, frac = _mask(sums, tau)
        ref = _ref_layers(sums, tau)
        assert all(_same(g, r) for g, r in zip((score, mask, count, frac), ref))
        assert mask[0].all() and count[0] == 96 and frac[0] == 1.0
        assert not mask[1].any() and count[1] == 0 and frac[1] == 0.0 and np.isnan(score[1]).all()


# ------------------------------------------------------------------------------------------------------- 2. recycle alone
def _trunk_layout(din, H, dout, ln, lead):
    """[(name, shape, offset)] of a trunk's parameters in a flat block, each on a 4-float slot as the agent lays them out,
    the block ``lead`` floats off; and the block's length."""
    shapes = [("0.weight", (H, din)), ("0.bias", (H,))] + ([("0.ln.weight", (H,)), ("0.ln.bias", (H,))] if ln else []) + \
        [("1.weight", (H, H)), ("1.bias", (H,))] + ([("1.ln.weight", (H,)), ("1.ln.bias", (H,))] if ln else []) + \
        [("2.weight", (dout, H)), ("2.bias", (dout,))]
    out, off = [], lead
    for name, shape in shapes:
        out.append((name, shape, off))
        off += (int(np.prod(shape)) + 3) & ~3
    return out, off


def _segments(layout, l1, l2):
    masks = R.trunk_masks([(n, s) for n, s, _ in layout], l1, l2)
    segs = []
    for name, shape, off in layout:
        r, c = masks[name]
        if r is None and c is None:
            continue
        segs.append((off, shape[0], shape[1] if len(shape) == 2 else 1, -1 if r is None else r, -1 if c is None else c))
    return segs


def _planted(n, rs):
    """Old values with a -0.0 and NaNs (one with a payload) planted: whatever is not written must keep its bits."""
    x = rs.randn(n).astype(np.float32)
    x[::7] = -0.0
    x[3::11] = NAN
    x.view(np.uint32)[5::13] = 0x7FC01234
    return x


def _run_recycle(din, H, dout, ln, nb, lead, pad, masks, offs=(0, 0, 0, 0)):
    """One launch over ``nb`` trunks ``pad`` floats further apart than their length, the four arrays ``offs`` floats off
    16-byte alignment each, inside NaN guards; everything -- guards and padding included -- against the NumPy rule."""
    from curla_amd import ops
    rs = np.random.RandomState(H + din + nb + lead)
    layout, length = _trunk_layout(din, H, dout, ln, lead)
    stride = length + pad
    total = (nb - 1) * stride + length
    L = masks.shape[0]
    twin = 2 if nb > 1 else 0
    host = {k: _planted(total, rs) for k in ("param", "m", "v")}
    host["fresh"] = rs.randn(total).astype(np.float32)
    img, dev = {}, {}
    for (k, x), o in zip(host.items(), offs):
        img[k] = np.full(total + 2 * GUARD + 3, NAN, np.float32)
        img[k][GUARD + o:GUARD + o + total] = x
        dev[k] = torch.from_numpy(img[k]).cuda()
    mask_dev = torch.from_numpy(masks.astype(np.int32)).cuda()
    views = {k: dev[k][GUARD + o:] for k, o in zip(host, offs)}
    assert all(views[k].data_ptr() % 16 == 4 * o for k, o in zip(host, offs))
    ops.redo_recycle(views["param"], views["m"], views["v"], views["fresh"], stride, nb, _segments(layout, 0, 1), mask_dev,
                     L, H, twin)
    torch.cuda.synchronize()
    want = {k: v.copy() for k, v in img.items()}
    written_any = 0
    for n in range(nb):
        named = R.trunk_masks([(nm, s) for nm, s, _ in layout], masks[2 * n if nb > 1 else 0] != 0,
                              masks[(2 * n if nb > 1 else 0) + 1] != 0)
        for name, shape, off in layout:
            r, c = named[name]
            size = int(np.prod(shape))
            at = n * stride + off
            cut = lambda k, o: want[k][GUARD + o + at:GUARD + o + at + size].reshape(shape)  # noqa: E731
            p, m, v, w = R.recycle(cut("param", offs[0]), cut("m", offs[1]), cut("v", offs[2]),
                                   host["fresh"][at:at + size].reshape(shape), r, c)
            cut("param", offs[0])[...], cut("m", offs[1])[...], cut("v", offs[2])[...] = p, m, v
            written_any += int(w.sum())
    for k in want:
        got = dev[k].cpu().numpy()
        assert np.array_equal(_bits(got), _bits(want[k])), (k, din, H, nb, lead, offs)
    assert np.array_equal(mask_dev.cpu().numpy(), masks)
    return written_any


def _masks(L, H, kind, seed=0):
    rs = np.random.RandomState(seed)
    if kind == "empty":
        return np.zeros((L, H), np.int32)
    if kind == "full":
        return np.ones((L, H), np.int32)
    m = (rs.rand(L, H) < 0.3).astype(np.int32)
    m[:, 0] = 1   # row 0 and column 0 cross in the second Linear: zero beats fresh there
    return m


@pytest.mark.parametrize("kind", ["empty", "full", "crossing"])
@pytest.mark.parametrize("din,H,dout,ln,nb,lead,pad,offs", [
    (56, 96, 1, False, 2, 0, 0, (0, 0, 0, 0)),      # the twins, dense, everything 16-byte aligned: whole float4s
    (56, 96, 5, True, 2, 0, 8, (0, 0, 0, 0)),       # LayerNorm vectors, atoms, the twins a padded stride apart
    (51, 96, 4, False, 1, 0, 0, (0, 0, 0, 0)),      # a first layer whose rows are no multiple of 4: that segment by element
    (56, 96, 1, True, 2, 1, 3, (0, 0, 0, 0)),       # the block one float off, an odd stride: by element throughout
    (56, 96, 1, False, 2, 0, 0, (0, 1, 0, 0)),      # m alone off 16-byte alignment
    (56, 96, 1, False, 1, 0, 0, (3, 3, 3, 2)),      # every array off
    (8, 4, 2, True, 2, 0, 0, (0, 0, 0, 0)),         # the smallest: one float4 per row
    (52, 1024, 1, False, 2, 0, 4, (0, 0, 0, 0)),    # the widest trunk: several workgroups per segment
], ids=["aligned", "ln_atoms_padded", "din51", "lead1", "m_off", "all_off", "tiny", "wide"])
def test_recycle_against_the_numpy_rule_bit_for_bit(kind, din, H, dout, ln, nb, lead, pad, offs):
    masks = _masks(6, H, kind, seed=H + din)
    if nb == 1:
        masks = masks[:2]
    written = _run_recycle(din, H, dout, ln, nb, lead, pad, masks, offs)
    assert (written == 0) == (kind == "empty")


def test_bad_arguments_are_refused_with_nothing_written():
    from curla_amd import _lib
    from curla_amd.ops import _RedoSeg
    lib = _lib.load()
    Bn, H, L = 4, 8, 2
    f = lambda n, v=3.0: torch.full((n,), v, device="cuda")  # noqa: E731
    h, sums, score, frac = f(2 * Bn * H), f(L * H), f(L * H), f(L)
    mask = torch.full((L * H,), 1, device="cuda", dtype=torch.int32)
    count = torch.full((L,), 5, device="cuda", dtype=torch.int32)
    param, m, v, fresh = f(256), f(256), f(256), f(256, 9.0)
    p = lambda t: t.data_ptr()  # noqa: E731
    nan = float("nan")

    def colsum(h_=p(h), sh=Bn * H, nb=2, B_=Bn, H_=H, s=p(sums), ss=H):
        return lib.curla_dormant_colsum(h_, sh, nb, B_, H_, s, ss, None)

    def dmask(s=p(sums), L_=L, H_=H, tau=0.1, sc=p(score), mk=p(mask), ct=p(count), fr=p(frac)):
        return lib.curla_dormant_mask(s, L_, H_, tau, sc, mk, ct, fr, None)

    def recycle(pa=p(param), m_=p(m), v_=p(v), fr=p(fresh), stride=128, nb=2, segs=((0, H, 4, 0, -1),), n=None, mk=p(mask),
                L_=L, H_=H, twin=1):
        arr = (_RedoSeg * max(1, len(segs)))()
        for a, sg in zip(arr, segs):
            a.offset, a.rows, a.cols, a.row_layer, a.col_layer = sg
        return lib.curla_redo_recycle(pa, m_, v_, fr, stride, nb, ctypes.addressof(arr) if segs is not None else None,
                                      len(segs) if n is None else n, mk, L_, H_, twin, None)
    for bad in (dict(h_=None), dict(s=None), dict(B_=0), dict(H_=0), dict(nb=0), dict(sh=Bn * H - 1), dict(ss=H - 1)):
        assert colsum(**bad) == -1, bad
    for bad in (dict(s=None), dict(sc=None), dict(mk=None), dict(ct=None), dict(fr=None), dict(L_=0), dict(H_=0),
                dict(tau=-1e-6), dict(tau=nan)):
        assert dmask(**bad) == -1, bad
    for bad in (dict(pa=None), dict(m_=None), dict(v_=None), dict(fr=None), dict(mk=None), dict(nb=0), dict(H_=0), dict(L_=0),
                dict(n=0), dict(n=13), dict(twin=-1), dict(twin=2), dict(segs=((0, 0, 4, 0, -1),)),
                dict(segs=((0, H, 0, 0, -1),)), dict(segs=((-4, H, 4, 0, -1),)), dict(segs=((0, H, 4, 1, -1),)),
                dict(segs=((0, H, 4, -2, -1),)), dict(segs=((0, H, 4, -1, 0),)), dict(segs=((0, H - 1, 4, 0, -1),)),
                dict(segs=((100, H, 4, 0, -1),)), dict(stride=31)):
        assert recycle(**bad) == -1, bad
    torch.cuda.synchronize()
    for t, val in ((sums, 3.0), (score, 3.0), (frac, 3.0), (param, 3.0), (m, 3.0), (v, 3.0), (fresh, 9.0)):
        assert bool((t == val).all())
    assert bool((mask == 1).all()) and bool((count == 5).all())
    assert colsum() == 0 and dmask() == 0 and recycle() == 0  # (the good calls of the same builders go through)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------- 3. whole agent
PLANT_1, PLANT_2 = 5, 11  # the dead unit planted in the first / the second hidden layer of every trunk


def _plant(agent):
    """A first-layer and a second-layer unit of Q1, Q2 and the actor trunk dead for every input: zero incoming weights,
    bias -1e3; behind a LayerNorm, gamma 0 and beta -1."""
    from curla_amd.mlp import _linears
    with torch.no_grad():
        for seq in (agent.critic.Q1.trunk, agent.critic.Q2.trunk, agent.actor.trunk):
            lin = _linears(seq)
            lns = [m for m in seq if isinstance(m, torch.nn.LayerNorm)]
            for k, unit in ((0, PLANT_1), (1, PLANT_2)):
                lin[k].weight[unit].zero_()
                lin[k].bias[unit] = -1e3
                if lns:
                    lns[k].weight[unit] = 0.0
                    lns[k].bias[unit] = -1.0
        agent.critic_target.load_state_dict(agent.critic.state_dict())


def _trunks(agent):
    """[(flat name, optimizer name, trunk, mask rows)] of the three recycled trunks."""
    return [("critic", "critic", agent.critic.Q1.trunk, (0, 1)), ("critic", "critic", agent.critic.Q2.trunk, (2, 3)),
            ("actor", "actor", agent.actor.trunk, (4, 5))]


def _pair(kw, rb_kw=None, steps=(1, 2), redo=None, dp=False):
    """(agent with redo_interval=2, its ring, its logger, the agent without the keywords after the same updates, the
    reset stream's state before any pass)."""
    out = []
    for on in (True, False):
        extra = dict(redo_interval=2, reset_seed=3, **(redo or {})) if on else dict(reset_seed=3)
        agent, aug = make(seed=2, **{**kw, **extra})
        _plant(agent)
        rb = ring(aug, **(rb_kw or {}))
        stream = agent._reset_stream().clone()
        if dp and on:
            agent.enable_data_parallel(single_rank_collectives=True, overlap=False, check_every=1)
        _seed(21)
        L = NullLogger()
        for step in steps:
            agent.update(rb, L, step)
        torch.cuda.synchronize()
        out.append((agent, rb, L, stream))
    (a, rb, L, stream), (b, rb_b, _, _) = out
    return a, rb, L, b, rb_b, stream


def _expected_masks(agent):
    """The six masks by the definition, from the activations the pass left in the workspace -- and that the agent's
    own sums, scores, masks, counts and fractions are the definition's, bit for bit."""
    ws = agent._workspaces[B]
    acts = [ws.q_h1[0], ws.q_h2[0], ws.q_h1[1], ws.q_h2[1], ws.a_h1, ws.a_h2]
    sums = np.stack([R.colsum(x.cpu().numpy()) for x in acts])
    buf = agent._redo_buf
    assert np.array_equal(_bits(buf["sums"].cpu().numpy()), _bits(sums))
    ref = _ref_layers(sums, agent.redo_tau)
    for key, want in zip(("score", "mask", "count", "fraction"), ref):
        assert _same(buf[key].cpu().numpy(), want), key
    assert buf["count"] is agent.dormant_counts and buf["fraction"] is agent.dormant_fractions
    assert agent.dormant_counts.dtype == torch.int32 and agent.dormant_fractions.dtype == torch.float32
    report = agent.dormant_report()
    assert list(report) == list(R.LAYERS) and [np.float32(x) for x in report.values()] == list(ref[3])
    masks = ref[1] != 0
    for layer, unit in zip(range(6), (PLANT_1, PLANT_2) * 3):
        assert masks[layer, unit] and not sums[layer, unit], (layer, unit)  # the planted units: exactly dead
    return masks


def _check_recycled(a, b, stream):
    """Agent ``a`` after its redo step against agent ``b`` (the same updates, no pass): parameters and moments differ
    exactly at the elements the rule writes, where they are the stream's fresh values / zeros; all else is bitwise b's."""
    from tests.test_gpu_reset import _fresh_named
    masks = _expected_masks(a)
    assert np.array_equal(a.dormant_counts.cpu().numpy(), masks.sum(1))
    b._reset_rng = stream.clone()
    fresh = _fresh_named(b, b._draw_fresh())
    sa, sb = _state(a), _state(b)
    want = {k: sb[k].numpy().copy() for k in ("critic", "actor", "critic_m", "critic_v", "actor_m", "actor_v")}
    touched = 0
    for (flat, opt, seq_a, rows), (_, _, seq_b, _) in zip(_trunks(a), _trunks(b)):
        named = [(n, p) for n, p in seq_a.named_parameters()]
        rc = R.trunk_masks([(n, tuple(p.shape)) for n, p in named], masks[rows[0]], masks[rows[1]])
        prefix = {0: "critic.Q1.trunk.", 2: "critic.Q2.trunk.", 4: "actor.trunk."}[rows[0]]
        base = getattr(a, "_%s_flat" % flat).data_ptr()
        lo = a._optimizers()[opt]._lo
        for n, p in named:
            off, size = (p.data_ptr() - base) // 4, p.numel()
            r, c = rc[n]
            cut = lambda k, o: want[k][o:o + size].reshape(tuple(p.shape))  # noqa: E731
            new, m2, v2, w = R.recycle(cut(flat, off), cut(opt + "_m", off - lo), cut(opt + "_v", off - lo),
                                       fresh[prefix + n], r, c)
            cut(flat, off)[...], cut(opt + "_m", off - lo)[...], cut(opt + "_v", off - lo)[...] = new, m2, v2
            touched += int(w.sum())
    assert touched > 0
    for k, v in want.items():
        assert np.array_equal(_bits(sa[k].numpy()), _bits(v)), k
    for k in sa:  # the target critic, log_alpha, the other optimizers, every step count: b's
        if k not in want:
            assert torch.equal(sa[k].reshape(-1).view(torch.uint8), sb[k].reshape(-1).view(torch.uint8)), k
    assert bool((sa["critic"] != sb["critic"]).any()) and bool((sa["actor"] != sb["actor"]).any())
    assert bool((sb["critic_m"] != 0).any()) and bool((sb["actor_m"] != 0).any())  # (there were moments to clear)


AGENT_CONFIGS = [("plain", {}, None), ("ln_dropout", dict(critic_layer_norm=True, critic_dropout=0.01), None),
                 ("tqc", dict(critic_quantiles=5), None), ("utd3", dict(utd_ratio=3, critic_target_update_freq=1), None),
                 ("prioritized", {}, dict(prioritized=True)), ("detach_encoder", dict(detach_encoder=True), None)]


@pytest.mark.parametrize("name,kw,rb_kw", AGENT_CONFIGS, ids=[c[0] for c in AGENT_CONFIGS])
def test_a_redo_step_writes_exactly_what_the_rule_names(name, kw, rb_kw):
    a, rb, L, b, _, stream = _pair(kw, rb_kw)
    assert a.redo_count == 1 and b.redo_count == 0 and b._redo_buf is None and b.dormant_counts is None
    _check_recycled(a, b, stream)
    crit, act = L.scalars["train_critic/dormant_fraction"], L.scalars["train_actor/dormant_fraction"]
    fr = a.dormant_fractions.cpu().numpy()
    # (a float32 mean of at most four values <= 1, in whatever order the device adds them: within 4 * 2**-24)
    assert abs(crit - fr[:4].astype(np.float64).mean()) <= 2.0 ** -22
    assert abs(act - fr[4:].astype(np.float64).mean()) <= 2.0 ** -22
    assert crit >= 1 / 96 and act >= 1 / 96
    for step in (3, 4):  # and training goes on, the planted units on fresh incoming weights
        a.update(rb, L, step)
    torch.cuda.synchronize()
    assert a.redo_count == 2 and all(np.isfinite(v) for v in L.scalars.values())
    assert bool(a.critic.Q1.trunk[0].weight[PLANT_1].any()) and bool(a.actor.trunk[0].weight[PLANT_1].any())


def test_score_only_leaves_the_agent_bitwise_alone():
    a, rb, L, b, rb_b, _ = _pair({}, redo=dict(redo_recycle=False))
    _assert_same(_state(a, rb), _state(b, rb_b))
    _expected_masks(a)
    assert a.redo_count == 1 and a._reset_stage is None and "train_critic/dormant_fraction" in L.scalars
    assert torch.equal(a._reset_stream(), b._reset_stream())  # nothing was drawn


def test_a_pass_leaves_the_global_streams_alone():
    agent, aug = make(seed=3, redo_interval=0)
    _plant(agent)
    rb = ring(aug)
    agent.update(rb, NullLogger(), 1)
    obs, action = rb.sample_cpc_refs()[:2]
    torch.cuda.synchronize()
    before = (torch.get_rng_state().clone(), torch.cuda.get_rng_state().clone(), np.random.get_state())
    agent.redo_recycle = False
    agent.redo_pass(obs, action)
    _expected_masks(agent)
    agent.redo_recycle, agent.redo_tau = True, 0.0  # (tau 0: the exactly dead units; this pass draws from the stream)
    agent.redo_pass(obs, action)
    torch.cuda.synchronize()
    after = (torch.get_rng_state(), torch.cuda.get_rng_state(), np.random.get_state())
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    assert np.array_equal(before[2][1], after[2][1]) and before[2][2:] == after[2][2:]
    assert agent.redo_count == 2 and int(agent.dormant_counts.min()) >= 1 and agent._reset_stage is not None


def _float64_hidden(seq, x):
    """The two post-ReLU hidden outputs of a trunk in float64 on the host, by torch's own functions, evaluation mode
    (no dropout)."""
    import torch.nn.functional as F
    d = lambda t: t.detach().double().cpu()  # noqa: E731
    x, out = d(x), []
    for m in seq:
        if isinstance(m, torch.nn.Linear):
            x = F.linear(x, d(m.weight), d(m.bias))
        elif isinstance(m, torch.nn.LayerNorm):
            x = F.layer_norm(x, (x.shape[1],), d(m.weight), d(m.bias), m.eps)
        elif isinstance(m, torch.nn.ReLU):
            x = torch.relu(x)
            out.append(x)
    assert len(out) == 2
    return out


@pytest.mark.parametrize("kw", [{}, dict(critic_layer_norm=True, critic_dropout=0.1)], ids=["plain", "ln_dropout"])
def test_the_forward_of_a_pass_against_float64(kw):
    """What the pass scores, checked on its own: the six activation buffers it leaves against the oracle's float64
    encoder and torch's float64 Linear / LayerNorm / ReLU on the agent's parameters as they stand after an update, the
    user's observations and actions, and no dropout -- at RTOL."""
    from oracle import curla_oracle as O
    agent, aug = make(seed=9, redo_recycle=False, **kw)
    rb = ring(aug)
    agent.update(rb, NullLogger(), 1)  # (parameters an optimizer step away from their initialisation)
    rs = np.random.RandomState(4)
    obs = torch.from_numpy(rs.randint(0, 256, (B, 9) + tuple(agent.image_shape)).astype(np.float32)).cuda()
    action = torch.from_numpy(rs.uniform(-1, 1, (B, 2)).astype(np.float32)).cuda()
    assert agent.training and agent.critic.training
    agent.redo_pass(obs, action)
    torch.cuda.synchronize()
    ws = agent._workspaces[B]
    obs64, layers = obs.double().cpu(), HP["num_layers"]
    z = {}
    for name, net in (("critic", agent.critic), ("actor", agent.actor)):
        sd = O.as_dtype({k: v.cpu() for k, v in net.state_dict().items()}, torch.float64)
        z[name] = O.encoder_forward(sd, "encoder.", obs64, layers, output_logits=net.encoder.output_logits)
    xa = torch.cat([z["critic"], action.double().cpu()], 1)
    want = _float64_hidden(agent.critic.Q1.trunk, xa) + _float64_hidden(agent.critic.Q2.trunk, xa) + \
        _float64_hidden(agent.actor.trunk, z["actor"])
    got = [ws.q_h1[0], ws.q_h2[0], ws.q_h1[1], ws.q_h2[1], ws.a_h1, ws.a_h2]
    for layer, g, w in zip(R.LAYERS, got, want):
        e = rel_err(g, w)
        print("%s: rel %.2e" % (layer, e))
        assert e <= RTOL, layer
    # and the scores are those of these activations
    sums = np.stack([R.colsum(g.cpu().numpy()) for g in got])
    assert np.array_equal(_bits(agent._redo_buf["sums"].cpu().numpy()), _bits(sums))


def test_one_rank_data_parallel(nccl_world1):  # noqa: F811
    a, rb, L, b, _, stream = _pair({}, dp=True)
    a.check_replicas()
    _check_recycled(a, b, stream)


def test_update_graphs_across_a_redo_step():
    hp = dict(redo_interval=6, reset_seed=2, log_interval=10 ** 9)

    def run(graphs):
        agent, aug = make(seed=6, **hp)
        _plant(agent)
        rb = ring(aug)
        _seed(12)
        if graphs:
            agent.enable_update_graphs(rb, warm=1, depth=2)
        L = NullLogger()
        for step in range(1, 10):
            if graphs and step == 6:
                ids = [id(st["graph"]) for r in agent._graphs.values() for st in r]
                assert ids and not agent._graph_usable(rb, 6, False) and agent._graph_usable(rb, 7, False)
            agent.update(rb, L, step)
        if graphs:  # addresses did not move: nothing was captured again
            assert set(ids) <= {id(st["graph"]) for r in agent._graphs.values() for st in r}
        assert agent.redo_count == 1 and int(agent.dormant_counts.sum()) >= 6
        return _state(agent, rb)
    _assert_same(run(False), run(True))


def test_checkpoint_across_a_redo_step(tmp_path):
    hp = dict(redo_interval=4, redo_tau=0.2, reset_seed=4)
    agent, aug = make(seed=8, **hp)
    _plant(agent)
    rb, L = ring(aug), NullLogger()
    _seed(14)
    for step in (1, 2, 3):
        agent.update(rb, L, step)
    ck = str(tmp_path / "redo.pt")
    agent.save_checkpoint(ck, 3)
    for step in (4, 5, 6):
        agent.update(rb, L, step)
    assert agent.redo_count == 1
    want = _state(agent, rb), dict(L.scalars)

    other, aug2 = make(seed=99, **{**hp, "reset_seed": 1234})
    rb2, L2 = ring(aug2), NullLogger()
    _seed(99)
    assert other.load_checkpoint(ck) == 3 and other.redo_count == 0
    for step in (4, 5, 6):
        other.update(rb2, L2, step)
    assert other.redo_count == 1
    got = _state(other, rb2), dict(L2.scalars)
    _assert_same(got[0], want[0])
    assert got[1] == want[1]
    other.save_checkpoint(ck, 6)
    third, _ = make(seed=5, redo_interval=4)
    assert third.load_checkpoint(ck) == 6 and third.redo_count == 1 and third.redo_tau == 0.1  # its own settings
