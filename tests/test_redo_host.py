"""Dormant-neuron scores and ReDo recycling on the host, under the launch-trace hook: nothing is computed
on a device.  The NumPy definition (tests/_redo_ref.py) against plain loops; the three keywords and their validation;
the C entry points (declared, bound, exported, argument checks); that an update off the schedule launches what an agent
without the keywords launches; the launches of a redo step; ``_graph_usable``; checkpoints."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import curla_amd
from curla_amd import _lib, agent_redo
from tests import _redo_ref as R
from tests.test_reset_host import C, NET, OUT_HW, ROOT, Log, make, traced

REDO_KEYS = {"redo_interval", "redo_tau", "redo_recycle", "redo_count"}
NAN = float("nan")


def _batch(n=8):
    """A user's minibatch for redo_pass: float observations and actions."""
    return torch.zeros(n, C, *OUT_HW), torch.zeros(n, 2)


# ------------------------------------------------------------------------------------------ the definition, by plain loops
def _loops_dormant(h, tau):
    Bn, H = len(h), len(h[0])
    sums = []
    for j in range(H):
        s = np.float32(0.0)
        for b in range(Bn):
            s = np.float32(s + np.float32(abs(h[b][j])))
        sums.append(s)
    total = 0.0
    for s in sums:
        total += float(s)
    mean = total / H
    score, mask = [], []
    for s in sums:
        x = np.float32(float(s) / mean) if mean != 0 else np.float32(NAN if s == 0 or math.isnan(s) else math.inf)
        score.append(x)
        mask.append(bool(mean == 0 or x <= np.float32(tau)))
    return np.array(sums, np.float32), np.array(score, np.float32), np.array(mask), sum(mask)


@pytest.mark.parametrize("tau", [0.0, 0.1, 1.0])
def test_reference_scores_against_plain_loops(tau):
    rs = np.random.RandomState(1)
    h = (rs.randn(7, 12) * 10.0 ** rs.uniform(-2, 1, 12)).astype(np.float32)
    h[:, 3] = 0.0            # an exactly dead unit: dormant at every tau, tau = 0 included
    h[:, 8] *= 1e-3
    sums, score, mask, count = _loops_dormant(h.tolist(), tau)
    got_sums = R.colsum(h)
    got = R.dormant(got_sums, tau)
    assert got_sums.dtype == np.float32 and np.array_equal(got_sums, sums)
    assert got[0].dtype == np.float32 and np.array_equal(got[0], score) and np.array_equal(got[1], mask)
    assert got[2] == count and got[3] == np.float32(count / 12) and isinstance(got[3], np.float32)
    assert mask[3] and (tau > 0 or count == 1) and (tau < 1 or 1 < count < 12)
    # float32 along b, in index order: not the float64 sum rounded
    big = np.array([[1.0], [2.0 ** -24], [2.0 ** -24]], np.float32)
    assert R.colsum(big)[0] == np.float32(1.0)


def test_reference_zero_layer_and_nan_layer():
    zero = np.zeros((5, 8), np.float32)
    for tau in (0.0, 0.1):
        score, mask, count, frac = R.dormant(R.colsum(zero), tau)
        assert mask.all() and count == 8 and frac == 1.0 and np.isnan(score).all()
    h = np.ones((5, 8), np.float32)
    h[2, 4] = NAN
    h[:, 1] = 0.0
    sums = R.colsum(h)
    assert np.isnan(sums[4]) and np.isnan(sums).sum() == 1
    score, mask, count, frac = R.dormant(sums, 0.1)
    assert not mask.any() and count == 0 and frac == 0.0 and np.isnan(score).all()  # (the dead unit 1 included)
    _, _, mask_loops, n = _loops_dormant(h.tolist(), 0.1)
    assert not mask_loops.any() and n == 0
    _, _, mask_loops, n = _loops_dormant(zero.tolist(), 0.1)
    assert mask_loops.all() and n == 8


def _loops_rule(param, m, v, fresh, r, c):
    param, m, v = [list(map(float, row)) for row in param], [list(row) for row in m], [list(row) for row in v]
    written = [[False] * len(param[0]) for _ in param]
    for i in range(len(param)):
        for j in range(len(param[0])):
            if c is not None and c[j]:
                param[i][j] = 0.0
            elif r is not None and r[i]:
                param[i][j] = float(fresh[i][j])
            else:
                continue
            m[i][j] = v[i][j] = 0.0
            written[i][j] = True
    return param, m, v, written


def test_reference_rule_against_plain_loops():
    rs = np.random.RandomState(2)
    rows, cols = 6, 5
    param, m, v, fresh = (rs.randn(rows, cols).astype(np.float32) for _ in range(4))
    param[1, 1], param[4, 4], m[4, 4] = -0.0, NAN, NAN
    r = np.array([1, 0, 1, 0, 0, 0], bool)
    c = np.array([0, 0, 1, 1, 0], bool)
    for rr, cc in ((r, c), (r, None), (None, c), (None, None), (np.ones(rows, bool), np.ones(cols, bool))):
        got = R.recycle(param, m, v, fresh, rr, cc)
        want = _loops_rule(param, m, v, fresh, rr, cc)
        for g, w in zip(got, want):
            w = np.array(w, dtype=g.dtype)
            assert np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g,
                                  w.view(np.uint32) if w.dtype == np.float32 else w)
    out, m2, v2, w = R.recycle(param, m, v, fresh, r, c)
    assert out[0, 2] == 0.0 and out[2, 3] == 0.0             # a masked row crossing a masked column: zero beats fresh
    assert out[0, 0] == fresh[0, 0] and out[1, 2] == 0.0 and w[1, 2] and not w[1, 1]
    assert np.signbit(out[1, 1]) and np.isnan(out[4, 4]) and np.isnan(m2[4, 4])  # unwritten: the bits they had
    assert not m2[w].any() and not v2[w].any() and np.array_equal(m2[~w].view(np.uint32), m[~w].view(np.uint32))
    # a vector: its own row mask only
    b, wb = R.rule(param[:, 0], fresh[:, 0], r)
    assert np.array_equal(wb, r) and np.array_equal(b[r], fresh[r, 0]) and np.array_equal(b[~r], param[~r, 0])


def test_trunk_masks_follow_the_modules():
    h1, h2 = np.array([1, 0, 0], bool), np.array([0, 1, 0], bool)
    plain = [("0.weight", (3, 7)), ("0.bias", (3,)), ("2.weight", (3, 3)), ("2.bias", (3,)), ("4.weight", (2, 3)),
             ("4.bias", (2,))]
    got = R.trunk_masks(plain, h1, h2)
    assert got["0.weight"] == (h1, None) and got["0.bias"] == (h1, None) and got["2.weight"] == (h2, h1)
    assert got["2.bias"] == (h2, None) and got["4.weight"] == (None, h2) and got["4.bias"] == (None, None)
    ln = plain[:2] + [("1.weight", (3,)), ("1.bias", (3,))] + plain[2:]
    got = R.trunk_masks(ln, h1, h2)
    assert got["1.weight"] == (h1, None) and got["1.bias"] == (h1, None) and got["2.weight"] == (h2, h1)


# ------------------------------------------------------------------------------------------------ keywords, validation
def test_keyword_positions_and_defaults():
    init = list(inspect.signature(curla_amd.CurlSacAgent.__init__).parameters)
    assert init[-1] == "pixel_sac" and not REDO_KEYS & set(init)
    call = inspect.signature(curla_amd.CurlSacAgent).parameters
    names = list(call)
    for k, default in (("redo_interval", 0), ("redo_tau", 0.1), ("redo_recycle", True)):
        assert call[k].default == default and type(call[k].default) is type(default)
        assert call[k].kind is inspect.Parameter.KEYWORD_ONLY
        assert names.index(k) < names.index("reset_interval")
    assert names[-2] == "critic_layer_norm"
    off, _ = make()
    assert (off.redo_interval, off.redo_tau, off.redo_recycle, off.redo_count) == (0, 0.1, True, 0)
    assert off.dormant_counts is None and off.dormant_fractions is None and off.dormant_report() == {}
    on, _ = make(redo_interval=np.int64(10), redo_tau=0, redo_recycle=False)
    assert (on.redo_interval, on.redo_tau, on.redo_recycle) == (10, 0.0, False)
    assert type(on.redo_interval) is int and type(on.redo_tau) is float and type(on.redo_recycle) is bool
    assert agent_redo.LAYERS == R.LAYERS == ("Q1.h1", "Q1.h2", "Q2.h1", "Q2.h2", "actor.h1", "actor.h2")


@pytest.mark.parametrize("kw", [dict(redo_interval=-1), dict(redo_interval=True), dict(redo_interval=2.0),
                                dict(redo_interval="10"), dict(redo_interval=None),
                                dict(redo_tau=-0.1), dict(redo_tau=True), dict(redo_tau=NAN), dict(redo_tau="0.1"),
                                dict(redo_tau=None),
                                dict(redo_recycle=1), dict(redo_recycle=0), dict(redo_recycle="yes"), dict(redo_recycle=None)])
def test_rejected_values(kw):
    with pytest.raises(ValueError):
        curla_amd.CurlSacAgent((C,) + OUT_HW, (2,), "cpu", None, **NET, **kw)


def test_edited_attributes_are_checked_again():
    agent, rb = make(redo_interval=2)
    agent.redo_interval = 2.5
    with pytest.raises(ValueError):
        traced(lambda: agent.update(rb, Log(), 1))
    agent.redo_interval = 2
    for name, bad in (("redo_tau", -1.0), ("redo_tau", NAN), ("redo_recycle", 1)):
        good = getattr(agent, name)
        setattr(agent, name, bad)
        with pytest.raises(ValueError):
            traced(lambda: agent.update(rb, Log(), 2))
        setattr(agent, name, good)
    assert agent.redo_count == 0
    traced(lambda: agent.update(rb, Log(), 2))
    assert agent.redo_count == 1


def test_a_cpu_agent_without_the_trace_hook_refuses():
    agent, rb = make()
    obs, action = _batch()
    with pytest.raises(RuntimeError):
        agent.redo_pass(obs, action)
    assert agent.redo_count == 0 and agent._redo_buf is None


def test_recycling_needs_the_flat_optimizers():
    """torch's own Adam keeps no mirror of the flat layout: refused before anything is launched or drawn; scoring alone
    does not need the moments."""
    agent, rb = make()
    obs, action = _batch()
    stream = agent._reset_stream().clone()
    hook, agent_redo._lib._trace_hook = agent_redo._lib._trace_hook, None
    try:
        with pytest.raises(RuntimeError, match="FlatAdam"):
            agent._redo_moments(agent.critic_optimizer, 0, 4)
    finally:
        agent_redo._lib._trace_hook = hook
    assert torch.equal(agent._reset_stream(), stream)
    agent.redo_recycle = False
    names = [n for n, _ in traced(lambda: agent.redo_pass(obs, action))]
    assert names[-1] == "curla_dormant_mask" and agent.redo_count == 1


# --------------------------------------------------------------------------------------------------------------- C ABI
ENTRY_POINTS = {
    "curla_dormant_colsum": ["h", "h_stride", "nb", "B", "H", "sums", "sums_stride", "stream"],
    "curla_dormant_mask": ["sums", "L", "H", "tau", "score", "mask", "count", "fraction", "stream"],
    "curla_redo_recycle": ["param", "m", "v", "fresh", "stride", "nb", "segs", "nsegs", "mask", "L", "H", "mask_twin",
                           "stream"],
}


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_entry_points_are_declared_bound_and_exported(name):
    from curla_amd import ops
    text = open(os.path.join(ROOT, "include", "curla_hip.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:#define[^\n]*\n|typedef struct[^;]*;[^;]*;[^;]*;[^}]*}[^;]*;\s*)*int %s\(([^;]*)\);"
                  % name, text, flags=re.S)
    assert m, "include/curla_hip.h does not declare %s behind a comment" % name
    assert "Additive: CURLA_ABI_VERSION stays 8" in " ".join(m.group(1).replace("*", " ").split())
    params = [p.strip() for p in m.group(2).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == ENTRY_POINTS[name]
    assert len(params) == len(_lib.SIGNATURES[name])
    for p, t in zip(params, _lib.SIGNATURES[name]):
        want = _lib.vp if "*" in p else _lib.c_ll if p.startswith("long long") else _lib.c_float if p.startswith("float") \
            else _lib.c_int
        assert t is want, (name, p)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert _lib.ABI_VERSION == 8 and _lib.load().curla_abi_version() == 8
    assert callable(getattr(ops, name[len("curla_"):]))
    heads = open(os.path.join(ROOT, "curla_amd", "csrc", "heads.hip")).read()
    assert '#include "redo.h"' in heads and heads.index('#include "tqc.h"') < heads.index('#include "redo.h"')
    kernels = open(os.path.join(ROOT, "curla_amd", "csrc", "redo.h")).read()
    assert all(k in kernels for k in ("dormant_colsum_kernel(", "dormant_mask_kernel(", "redo_recycle_kernel("))
    assert "atomic" not in kernels.lower().replace("no atomics", "")
    assert "#define CURLA_REDO_MAX_SEGS 12" in text and ops.REDO_MAX_SEGS == 12
    assert ctypes.sizeof(ops._RedoSeg) == 24


def test_entry_points_check_their_arguments_before_any_launch():
    """CURLA_ERR_ARG (-1), decided on the host: a machine without a GPU sees it too (nothing is dereferenced)."""
    from curla_amd.ops import _RedoSeg
    lib = _lib.load()
    p = 4096  # a non-NULL, aligned, never dereferenced address
    H = 8

    def colsum(h=p, sh=32, nb=2, B=4, H_=H, s=p, ss=H):
        return lib.curla_dormant_colsum(h, sh, nb, B, H_, s, ss, None)

    def dmask(s=p, L=2, H_=H, tau=0.1, sc=p, mk=p, ct=p, fr=p):
        return lib.curla_dormant_mask(s, L, H_, tau, sc, mk, ct, fr, None)

    def recycle(pa=p, m=p, v=p, fr=p, stride=128, nb=2, seg=(0, H, 4, 0, -1), n=1, mk=p, L=2, H_=H, twin=1, segs=True):
        arr = (_RedoSeg * 1)()
        arr[0].offset, arr[0].rows, arr[0].cols, arr[0].row_layer, arr[0].col_layer = seg
        return lib.curla_redo_recycle(pa, m, v, fr, stride, nb, ctypes.addressof(arr) if segs else None, n, mk, L, H_, twin,
                                      None)
    for bad in (dict(h=None), dict(s=None), dict(B=0), dict(H_=0), dict(nb=0), dict(sh=31), dict(ss=H - 1), dict(h=p + 2)):
        assert colsum(**bad) == -1, bad
    for bad in (dict(s=None), dict(sc=None), dict(mk=None), dict(ct=None), dict(fr=None), dict(L=0), dict(H_=0),
                dict(tau=-1e-6), dict(tau=NAN), dict(tau=-math.inf)):
        assert dmask(**bad) == -1, bad
    for bad in (dict(pa=None), dict(m=None), dict(v=None), dict(fr=None), dict(mk=None), dict(segs=False), dict(nb=0),
                dict(H_=0), dict(L=0), dict(n=0), dict(n=13), dict(twin=-1), dict(twin=2), dict(seg=(0, 0, 4, 0, -1)),
                dict(seg=(0, H, 0, 0, -1)), dict(seg=(-4, H, 4, 0, -1)), dict(seg=(0, H, 4, 1, -1)),
                dict(seg=(0, H, 4, -2, -1)), dict(seg=(0, H, 4, -1, 0)), dict(seg=(0, H - 1, 4, 0, -1)),
                dict(seg=(100, H, 4, 0, -1)), dict(stride=31)):
        assert recycle(**bad) == -1, bad


def test_ops_wrappers_pass_what_the_abi_takes():
    from curla_amd import ops
    t = torch.zeros(64)
    i = torch.zeros(64, dtype=torch.int32)
    calls = traced(lambda: (ops.dormant_colsum(t, 16, 2, 4, 4, t, 8), ops.dormant_mask(t, 2, 8, np.float32(0.25), t, i, i, t),
                            ops.redo_recycle(t, None, None, t, 32, 2, [(0, 8, 4, 0, -1), (32, 8, 1, 0, -1)], i, 2, 8, 1)))
    assert [n for n, _ in calls] == ["curla_dormant_colsum", "curla_dormant_mask", "curla_redo_recycle"]
    assert calls[0][1] == ("ptr", 16, 2, 4, 4, "ptr", 8, 0)
    assert calls[1][1] == ("ptr", 2, 8, 0.25, "ptr", "ptr", "ptr", "ptr", 0)
    assert calls[2][1] == ("ptr", None, None, "ptr", 32, 2, "ptr", 2, "ptr", 2, 8, 1, 0)


# ------------------------------------------------------------------------------------------------------- launch lists
REDO_NAMES = {"curla_dormant_colsum", "curla_dormant_mask", "curla_redo_recycle"}
CONFIGS = [{}, dict(critic_layer_norm=True, critic_dropout=0.1, critic_quantiles=5), dict(utd_ratio=3)]


@pytest.mark.parametrize("kw", CONFIGS, ids=["plain", "ln_dropout_tqc", "utd3"])
@pytest.mark.parametrize("step", [1, 3])
def test_off_the_schedule_an_update_launches_what_it_launched(kw, step, tmp_path):
    plain, rb_p = make(**kw)
    on, rb_o = make(redo_interval=2, redo_tau=0.3, **kw)
    a = traced(lambda: plain.update(rb_p, Log(), step))
    b = traced(lambda: on.update(rb_o, Log(), step))
    assert a == b and len(a) > 10 and not REDO_NAMES & {n for n, _ in a}
    assert on._redo_buf is None and on._reset_stage is None and on.redo_count == 0  # nothing allocated either
    assert on._graph_key() == plain._graph_key()
    zero, rb_z = make(redo_interval=0, **kw)
    assert traced(lambda: zero.update(rb_z, Log(), 2)) == traced(lambda: plain.update(rb_p, Log(), 2))
    assert zero.redo_count == 0 and zero._redo_buf is None
    # step 0 and an only_cpc update are off the schedule as well
    assert not REDO_NAMES & {n for n, _ in traced(lambda: on.update(rb_o, Log(), 0))}
    assert not REDO_NAMES & {n for n, _ in traced(lambda: on.update(rb_o, Log(), 2, only_cpc=True))}


@pytest.mark.parametrize("kw", CONFIGS, ids=["plain", "ln_dropout_tqc", "utd3"])
@pytest.mark.parametrize("recycle", [True, False])
def test_the_launches_of_a_redo_step(kw, recycle):
    plain, rb_p = make(**kw)
    on, rb_o = make(redo_interval=2, redo_tau=0.25, redo_recycle=recycle, **kw)
    logged = []

    class Keep(Log):
        def log(self, key, value, step, n=1):
            logged.append((key, value, step))
    a = traced(lambda: plain.update(rb_p, Log(), 2))
    b = traced(lambda: on.update(rb_o, Keep(), 2))
    assert b[:len(a)] == a  # the update as it was, then the pass
    tail = b[len(a):]
    names = [n for n, _ in tail]
    ln = bool(kw.get("critic_layer_norm"))
    H, Bn, F, A = NET["hidden_dim"], 8, 50, 2
    fwd = ["curla_conv1_fwd", "curla_conv3x3_s1_fwd", "curla_gemm_multi", "curla_fc_ln_fwd_multi"] + \
        (["curla_gemm", "curla_mlp_ln_relu_fwd"] * 2 if ln else ["curla_gemm"] * 2) + ["curla_mlp_out_fwd"] + \
        ["curla_gemm"] * 2 + ["curla_mlp_out_fwd"]
    assert "curla_mlp_drop_ln_relu_fwd" not in names  # no dropout in the pass
    score = ["curla_dormant_colsum"] * 4 + ["curla_dormant_mask"]
    assert names == fwd + score + (["curla_redo_recycle"] * 2 if recycle else [])
    cs = [args for n, args in tail if n == "curla_dormant_colsum"]
    assert cs == [("ptr", Bn * H, 2, Bn, H, "ptr", 2 * H, 0)] * 2 + [("ptr", Bn * H, 1, Bn, H, "ptr", H, 0)] * 2
    mk, = [args for n, args in tail if n == "curla_dormant_mask"]
    assert mk == ("ptr", 6, H, 0.25, "ptr", "ptr", "ptr", "ptr", 0)
    if recycle:
        q, act = [args for n, args in tail if n == "curla_redo_recycle"]
        q_sz = on.critic.twin_stride
        assert q == ("ptr", None, None, "ptr", q_sz, 2, "ptr", 9 if ln else 5, "ptr", 6, H, 2, 0)
        assert act[4:6] == (H * F + H + H * H + H + 2 * A * H + 2 * A, 1) and act[7:] == (5, "ptr", 6, H, 0, 0)
        assert on._reset_stage is not None
    else:
        assert on._reset_stage is None
    assert on.redo_count == 1 and on._anchor_cache is None and on._pos_cache is None and on._pos_fc_done is False
    keys = [k for k, _, _ in logged]
    assert keys[-2:] == ["train_critic/dormant_fraction", "train_actor/dormant_fraction"]
    assert all(torch.is_tensor(v) and v.dim() == 0 and s == 2 for _, v, s in logged[-2:])
    assert on.dormant_counts.dtype == torch.int32 and tuple(on.dormant_counts.shape) == (6,)
    assert on.dormant_fractions.dtype == torch.float32 and tuple(on.dormant_fractions.shape) == (6,)
    assert list(on.dormant_report()) == list(R.LAYERS)


def test_the_segments_of_the_two_recycle_launches():
    from curla_amd.agent_redo import _trunk_segments
    agent, _ = make(critic_layer_norm=True)
    H, F, A = NET["hidden_dim"], 50, 2
    t = agent.critic.Q1.trunk
    segs = _trunk_segments(t, t[0].weight.data_ptr(), 0, 1)
    pad = lambda n: (n + 3) & ~3  # noqa: E731
    o = [0]
    for n in (H * (F + A), H, H, H, H * H, H, H, H, H):
        o.append(o[-1] + pad(n))
    # Linear 0 (+ bias), its LayerNorm, Linear 1 (+ bias), its LayerNorm, Linear 2: offsets by the flat layout
    assert segs == [(o[0], H, F + A, 0, -1), (o[1], H, 1, 0, -1), (o[4], H, H, 1, 0), (o[5], H, 1, 1, -1), (o[8], 1, H, -1, 1),
                    (o[2], H, 1, 0, -1), (o[3], H, 1, 0, -1), (o[6], H, 1, 1, -1), (o[7], H, 1, 1, -1)]
    assert o[8] + H <= agent.critic.twin_stride and len(segs) <= 12
    a = agent.actor.trunk
    segs = _trunk_segments(a, a[0].weight.data_ptr(), 4, 5)
    assert [s[3:] for s in segs] == [(4, -1), (4, -1), (5, 4), (5, -1), (-1, 5)] and segs[-1][1:3] == (2 * A, H)


def test_update_graphs_are_not_used_on_a_redo_step():
    agent, rb = make(redo_interval=4, log_interval=10 ** 9)
    agent._graph_rb = rb
    assert agent._graph_usable(rb, 3, False) and agent._graph_usable(rb, 5, False)
    assert not agent._graph_usable(rb, 4, False) and not agent._graph_usable(rb, 8, False)
    agent.redo_interval = 0
    assert agent._graph_usable(rb, 4, False)
    plain, rb_p = make(log_interval=10 ** 9)
    agent.redo_interval = 4
    assert agent._graph_key() == plain._graph_key()  # addresses do not move: the key gains nothing


# -------------------------------------------------------------------------------------------------------- checkpoints
def test_checkpoint_keys_and_an_old_file(tmp_path):
    plain, _ = make()
    on, rb = make(redo_interval=2, redo_tau=0.3, redo_recycle=False)
    traced(lambda: on.update(rb, Log(), 2))
    keys = {}
    for agent, name in ((plain, "p.pt"), (on, "o.pt")):
        agent.save_checkpoint(str(tmp_path / name), 2)
        keys[name] = torch.load(str(tmp_path / name), weights_only=False)
    assert set(keys["o.pt"]) - set(keys["p.pt"]) == REDO_KEYS and not REDO_KEYS & set(keys["p.pt"])
    ck = keys["o.pt"]
    assert (ck["redo_interval"], ck["redo_tau"], ck["redo_recycle"], ck["redo_count"]) == (2, 0.3, False, 1)
    assert "reset_rng" in ck  # the stream the fresh values come from travels as it did
    other, _ = make(redo_interval=5, redo_tau=0.2)
    assert other.load_checkpoint(str(tmp_path / "o.pt")) == 2
    assert (other.redo_count, other.redo_interval, other.redo_tau, other.redo_recycle) == (1, 5, 0.2, True)
    # a file from before the keywords
    assert other.load_checkpoint(str(tmp_path / "p.pt")) == 2 and other.redo_count == 0
    # an agent that made a pass by hand records it too
    obs, action = _batch()
    traced(lambda: plain.redo_pass(obs, action))
    plain.save_checkpoint(str(tmp_path / "p2.pt"), 3)
    assert torch.load(str(tmp_path / "p2.pt"), weights_only=False)["redo_count"] == 1
