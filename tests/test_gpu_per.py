"""Prioritized replay on the device (``ReplayBuffer(prioritized=True)``): the three kernels against NumPy restatements,
then through the buffer's routes and through the agent.

Stored values are small integers wherever a drawn ROW is compared: their float64 sums are exact in any order, so the
kernel's rows must EQUAL those of ``np.searchsorted(np.cumsum(s), u * total, side="right")``.  Tolerances: 2^-20 relative
for what goes through a handful of float32 roundings and one ``powf`` (curla_per_td), the suite's parity bar RTOL for
gradients and parameters of whole updates."""
import collections
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from tests._util import GOLDEN, RTOL, load, rel_err
from tests.test_gpu_agent import HP, NullLogger, _tiny_agent, grads_of
from tests.test_gpu_graph_aug import _episode, _state

pytestmark = pytest.mark.gpu

NEW = ("curla_per_set", "curla_per_sample", "curla_per_td")
TOL = 2.0 ** -20


def _ops():
    from curla_amd import ops
    return ops


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _storage(capacity, vmax=1.0):
    P = _ops().PER_CHUNK
    return (torch.zeros(capacity, dtype=torch.float32, device="cuda"),
            torch.zeros((capacity + P - 1) // P, dtype=torch.float64, device="cuda"),
            torch.full((1,), vmax, dtype=torch.float32, device="cuda"))


def numpy_rows(s, u):
    """The rule of the draw: the smallest row whose float64 cumulative sum exceeds u * total, clamped to the last row
    with a positive value."""
    cs = np.cumsum(s.astype(np.float64))
    total = cs[-1]
    idx = np.searchsorted(cs, u * total, side="right")
    return np.minimum(idx, np.flatnonzero(s > 0).max()), total


def _chunk_sums(s):
    P = _ops().PER_CHUNK
    pad = np.zeros((len(s) + P - 1) // P * P, dtype=np.float64)
    pad[:len(s)] = s
    return pad.reshape(-1, P).sum(axis=1)


# ------------------------------------------------------------------------------------------------- 1. the draw
def _patterns(cap, valid):
    P = _ops().PER_CHUNK
    out = {}
    s = np.zeros(cap, dtype=np.float32)
    s[:valid] = 3
    out["all equal"] = s
    for name, r in (("all mass in one row", valid // 2), ("all mass in the last row", valid - 1), ("all mass in row 0", 0)):
        s = np.zeros(cap, dtype=np.float32)
        s[r] = 7
        out[name] = s
    s = np.zeros(cap, dtype=np.float32)
    s[:valid] = 1 + np.arange(valid) % 4
    s[:2] = 0
    s[max(2, valid - 2):valid] = 0
    if valid > P + 3:
        s[P - 3:P + 3] = 0
    if valid > 2 * P + 3:
        s[2 * P - 1:2 * P + 1] = 0
    if s.sum() > 0:
        out["zero rows at the start, the end and across chunk boundaries"] = s
    s = np.zeros(cap, dtype=np.float32)
    lo = (valid - 1) // P * P
    s[lo:valid] = 1 + np.arange(valid - lo) % 3
    out["mass only in the last (partial) chunk"] = s
    return out


def _targets(s):
    """u values: 0, every u found whose u * total is EXACTLY a prefix sum (which pins the strict >) and its two float64
    neighbours, the largest float64 below 1, and a stratified random set."""
    cs = np.cumsum(s.astype(np.float64))
    total = cs[-1]
    us, exact = [0.0, np.nextafter(1.0, 0.0)], 0
    for p in np.unique(cs[cs < total])[:64]:
        c = p / total
        for cand in (c, np.nextafter(c, 0.0), np.nextafter(c, 1.0)):
            if 0.0 <= cand < 1.0 and cand * total == p:
                exact += 1
                us += [cand, np.nextafter(cand, 1.0)] + ([np.nextafter(cand, 0.0)] if cand > 0 else [])
                break
    rs = np.random.RandomState(len(s))
    us += list((np.arange(24) + rs.random_sample(24)) / 24)
    return np.array(us, dtype=np.float64), exact


@pytest.mark.parametrize("fill", ["part", "full"])
@pytest.mark.parametrize("cap", ["5", "P", "P+1", "3P-7"])
def test_the_draw_is_exact(cap, fill):
    ops = _ops()
    P = ops.PER_CHUNK
    cap = {"5": 5, "P": P, "P+1": P + 1, "3P-7": 3 * P - 7}[cap]
    valid = cap if fill == "full" else max(3, cap - max(2, cap // 3))
    hits = 0
    for name, s in _patterns(cap, valid).items():
        assert not s[valid:].any()
        st, sums, vmax = _storage(cap)
        ops.per_set(st, sums, vmax, valid, rows=torch.arange(valid, device="cuda"), values=_dev(s[:valid]))
        u, exact = _targets(s)
        hits += exact
        B = len(u)
        u_off, prob_off = 16 * B, 24 * B
        block = torch.zeros(24 * B + (4 * B + 7) // 8 * 8, dtype=torch.uint8, device="cuda")
        block[u_off:u_off + 8 * B].view(torch.float64).copy_(_dev(u))
        ops.per_sample(st, sums, block, u_off, prob_off, B)
        rows = block[:16 * B].view(torch.int64).cpu().numpy()
        prob = block[prob_off:prob_off + 4 * B].view(torch.float32).cpu().numpy()
        want, total = numpy_rows(s, u)
        assert total == s.astype(np.float64).sum() and np.array_equal(sums.cpu().numpy(), _chunk_sums(s)), name
        assert np.array_equal(rows[:B], want), (name, u[rows[:B] != want], rows[:B][rows[:B] != want], want[rows[:B] != want])
        assert np.array_equal(rows[B:], want + cap), name
        assert (s[rows[:B]] > 0).all(), name
        p64 = s[want].astype(np.float64) / total
        assert (np.abs(prob.astype(np.float64) - p64) <= 2.0 ** -23 * p64).all(), name
        assert np.array_equal(block[u_off:u_off + 8 * B].view(torch.float64).cpu().numpy(), u)  # u is only read
    assert hits >= 3  # targets that ARE a prefix sum were found and drawn from


# ------------------------------------------------------------------------------------------------- 2. per_set
class _Model:
    def __init__(self, cap):
        self.s, self.vmax = np.zeros(cap, dtype=np.float32), np.float32(1.0)

    def set(self, rows, values=None):
        rows = np.asarray(rows)
        if values is None:
            self.s[rows] = self.vmax
            return
        values = np.asarray(values, dtype=np.float32)
        self.s[rows] = 0
        np.maximum.at(self.s, rows, values)
        self.vmax = max(self.vmax, values.max())


def test_per_set_against_a_numpy_model():
    ops = _ops()
    P = ops.PER_CHUNK
    cap = 3 * P - 7
    st, sums, vmax = _storage(cap)
    model = _Model(cap)
    rs = np.random.RandomState(0)

    def step(what, rows=None, first=0, n=None, values=None):
        if rows is None:
            ops.per_set(st, sums, vmax, n, first_row=first, values=None if values is None else _dev(values))
            rows = (first + np.arange(n)) % cap
        else:
            ops.per_set(st, sums, vmax, len(rows), rows=_dev(np.asarray(rows, dtype=np.int64)),
                        values=None if values is None else _dev(np.asarray(values, dtype=np.float32)))
        model.set(rows, values)
        got = st.cpu().numpy()
        assert np.array_equal(got, model.s), (what, np.flatnonzero(got != model.s)[:8])  # the WHOLE array
        assert np.array_equal(sums.cpu().numpy(), _chunk_sums(model.s)), what  # (integers: exact in any order)
        assert vmax.item() == model.vmax, what

    step("new rows take the maximum scalar (1.0)", first=0, n=cap - 20)
    step("every row of one chunk in one call", rows=P + rs.permutation(P), values=rs.randint(0, 50, P))
    top = float(model.vmax)
    assert sums[1].item() == model.s[P:2 * P].astype(np.float64).sum() and top > 1.0
    step("rows spread over all chunks", rows=rs.permutation(cap)[:97], values=rs.randint(1, 30, 97))
    step("lower values do not lower the maximum", rows=[3, P + 3, 2 * P + 3], values=[2, 1, 0])
    assert vmax.item() == top
    rows = np.array([5, 5, 5, P - 1, P, P, 2 * P + 9, 5, P - 1])
    step("duplicates take their maximum, whatever the order", rows=rows, values=[4, 90, 6, 1, 8, 7, 3, 2, 60])
    assert st[5].item() == 90.0 and st[P - 1].item() == 60.0 and st[P].item() == 8.0 and vmax.item() == 90.0
    step("a duplicate may lower a row below its old value", rows=[5, 5], values=[1, 2])
    assert st[5].item() == 2.0 and vmax.item() == 90.0
    step("no values: the maximum scalar, a run that wraps", first=cap - 3, n=6)
    assert st[cap - 1].item() == 90.0 and st[2].item() == 90.0
    step("no values, rows given (with a duplicate)", rows=[7, 7, 2 * P + 1])
    step("one row", first=11, n=1)
    step("a run longer than the ring writes every row once or twice", first=P, n=cap + 5)
    assert (model.s == 90.0).all()
    step("a value of zero takes a row out of the draw", rows=[0], values=[0])


def test_per_set_stores_finite_non_negative_values_with_the_sign_bit_clear():
    """-0, negatives and NaN store +0 (an unsigned maximum over the words would otherwise let 0x80000000 win), +inf the
    largest float: the maximum scalar and the chunk sums stay finite, and the draw still finds the rows with mass."""
    ops = _ops()
    st, sums, vmax = _storage(8)
    big = np.finfo(np.float32).max
    vals = np.array([-0.0, -3.0, np.nan, 2.0, np.inf, -np.inf, 0.0, -0.0], dtype=np.float32)
    rows = np.array([0, 1, 2, 3, 4, 5, 3, 3], dtype=np.int64)  # row 3: the maximum of 2, +0 and -0
    ops.per_set(st, sums, vmax, 8, rows=_dev(rows), values=_dev(vals))
    got = st.cpu().numpy()
    assert np.array_equal(got, np.array([0, 0, 0, 2, big, 0, 0, 0], dtype=np.float32))
    assert not np.signbit(got).any() and vmax.item() == big
    assert sums.item() == 2.0 + float(big) and np.isfinite(sums.item())
    ops.per_set(st, sums, vmax, 2, rows=_dev(np.array([4, 6], dtype=np.int64)), values=_dev(np.array([-0.0, -0.0], dtype=np.float32)))
    assert st[4].item() == 0.0 and not np.signbit(st.cpu().numpy()).any() and sums.item() == 2.0 and vmax.item() == big


def test_a_ring_without_mass_draws_row_0_with_weight_0():
    ops = _ops()
    cap, B = 300, 4
    st, sums, vmax = _storage(cap)
    ops.per_set(st, sums, vmax, cap, rows=torch.arange(cap, device="cuda"), values=torch.zeros(cap, device="cuda"))
    block = torch.full((24 * B + 4 * B,), 0x55, dtype=torch.uint8, device="cuda")
    block[16 * B:24 * B].view(torch.float64).copy_(_dev(np.array([0.0, 0.3, 0.6, 0.99])))
    ops.per_sample(st, sums, block, 16 * B, 24 * B, B)
    assert block[:16 * B].view(torch.int64).tolist() == [0] * B + [cap] * B
    prob = block[24 * B:].view(torch.float32)
    assert prob.tolist() == [0.0] * B
    q, t, dq_in = _dev(np.ones((2, B), np.float32)), torch.zeros(B, device="cuda"), np.ones((2, B), np.float32)
    dq, loss, w, val = _dev(dq_in), torch.ones(1, device="cuda"), torch.ones(B, device="cuda"), torch.zeros(B, device="cuda")
    ops.per_td(q, B, t, prob, 0.4, 1e-6, 0.6, B, dq, loss, w, val)
    assert w.tolist() == [0.0] * B and not dq.any() and loss.item() == 0.0  # no 0/0: the samples carry no weight
    assert np.allclose(val.cpu().numpy(), (1.0 + 1e-6) ** 0.6, rtol=TOL, atol=0)


# ------------------------------------------------------------------------------------------------- 3. per_td
@pytest.mark.parametrize("beta", [0.0, 0.4, 1.0])
@pytest.mark.parametrize("B", [1, 7, 64, 512])
def test_per_td_against_float64(B, beta):
    ops = _ops()
    rs = np.random.RandomState(B)
    alpha, eps = 0.6, 1e-6
    for probs in ("random", "equal"):
        q = rs.randn(2, B).astype(np.float32) * 3
        t = rs.randn(B).astype(np.float32) * 3
        t[::5] = q[0, ::5]  # |q1 - t| = 0 on some rows: eps is all that is left of that half
        prob = (rs.uniform(1e-4, 1.0, B) if probs == "random" else np.full(B, 0.37)).astype(np.float32)
        dq_in = rs.randn(2, B).astype(np.float32)
        dq, loss, w, val = _dev(dq_in), torch.zeros(1, device="cuda"), torch.zeros(B, device="cuda"), torch.zeros(B, device="cuda")
        ops.per_td(_dev(q), B, _dev(t), _dev(prob), beta, eps, alpha, B, dq, loss, w, val)
        q64, t64, p64 = q.astype(np.float64), t.astype(np.float64), prob.astype(np.float64)
        w_ref = (p64.min() / p64) ** np.float64(np.float32(beta))
        d = q64 - t64
        loss_ref = (w_ref * (d[0] ** 2 + d[1] ** 2)).sum() / B
        val_ref = (0.5 * (np.abs(d[0]) + np.abs(d[1])) + np.float64(np.float32(eps))) ** np.float64(np.float32(alpha))
        dq_ref = dq_in.astype(np.float64) * w_ref

        def close(name, got, ref):
            got = got.cpu().numpy().astype(np.float64).reshape(np.shape(ref))
            err = np.abs(got - ref) / np.abs(ref)
            print(f"per_td B={B} beta={beta} {probs}: {name} max rel err {err.max():.3e}")
            assert (err <= TOL).all(), (name, err.max())
        close("w", w, w_ref)
        close("dq", dq, dq_ref)
        close("loss", loss, np.array([loss_ref]))
        close("value", val, val_ref)
        if beta == 0.0 or probs == "equal":
            assert torch.equal(w, torch.ones(B, device="cuda"))
            assert torch.equal(dq.cpu(), torch.from_numpy(dq_in))  # bit-identical


# ------------------------------------------------------------------------------------------------- 4. through the buffer
def _stream(n, C, hw, seed):
    """n transitions of one frame-stacked stream (obs[t + 1] = next_obs[t]; ``done`` every 7th step)."""
    rs = np.random.RandomState(seed)
    k = C // 3
    frames = rs.randint(0, 256, (n + k, 3) + hw, dtype=np.uint8)
    stacks = np.stack([frames[t:t + k].reshape((C,) + hw) for t in range(n + 1)])
    return (stacks[:-1], rs.uniform(-1, 1, (n, 2)).astype(np.float32), rs.randn(n).astype(np.float32), stacks[1:],
            np.arange(n) % 7 == 6)


ROUTES = {
    "plain": dict(C=3, hw=(4, 4), crop=(3, 3), cap=300, fill=270, kw=dict()),
    "dedup": dict(C=3, hw=(4, 4), crop=(3, 3), cap=300, fill=270, kw=dict(dedup_frames=True)),
    "two_allocations": dict(C=9, hw=(11, 13), crop=(8, 9), cap=41, fill=30, kw=dict()),
    "n_step": dict(C=3, hw=(4, 4), crop=(3, 3), cap=300, fill=270, kw=dict(n_step=3, discount=0.99)),
}


def _crops(ops, o, B):
    out = torch.empty((B, o.C, o.Hc, o.Wc), dtype=torch.float32, device="cuda")
    ops.crop_nchw(o.src, o.idx, o.h1, o.w1, B, (o.Hc, o.Wc), out_f32=out)
    return out


@pytest.mark.parametrize("route", list(ROUTES))
def test_through_the_buffer(route, tmp_path):
    import curla_amd
    ops = _ops()
    r = ROUTES[route]
    C, hw, cap, fill, B = r["C"], r["hw"], r["cap"], r["fill"], 16
    dev = torch.device("cuda")
    aug = curla_amd.RandomCrop(hw, r["crop"])
    mk = lambda **kw: curla_amd.ReplayBuffer((C,) + hw, (2,), cap, B, dev, aug, **r["kw"], **kw)  # noqa: E731
    per, twin = mk(prioritized=True), mk()
    if route == "two_allocations":
        assert per._both is None
    assert not per.graph_supported()
    ep = _stream(cap + 8, C, hw, 3)
    for rb in (per, twin):
        rb.add_batch(*(a[:fill] for a in ep))
        for t in range(fill, fill + 5):
            rb.add(*(a[t] for a in ep))
    n = fill + 5
    assert np.array_equal(per.priorities(), np.ones(n, dtype=np.float32))
    rs = np.random.RandomState(1)
    m = min(40, n // 2)
    rows_u = np.concatenate([rs.permutation(n)[:m], [7, 7]])
    vals_u = np.concatenate([rs.randint(0, 9, m), [3, 8]]).astype(np.float32)
    per.update_priorities(_dev(rows_u.astype(np.int64)), _dev(vals_u))
    model = _Model(n)
    model.set(np.arange(n))
    model.set(rows_u, vals_u)
    s = per.priorities()
    assert np.array_equal(s, model.s) and per._per_max.item() == 8.0
    assert not per._per_s[n:].any()  # rows never written hold 0
    # an injected (u, offs): the rows of the NumPy rule, their pixels and scalars bit for bit
    np.random.seed(11)
    u, offs = per.draw_indices()
    u[0], u[-1] = 0.0, np.nextafter(1.0, 0.0)
    want, total = numpy_rows(s, u)
    assert (s[want] > 0).all() and len(set(want)) > B // 2
    got = per.sample_cpc_refs(indices=(u, offs))
    ref = twin.sample_cpc_refs(indices=(want, offs))
    assert np.array_equal(got[0].per.rows.cpu().numpy(), want)
    assert np.array_equal(got[0].per.prob.cpu().numpy(), (s[want].astype(np.float64) / total).astype(np.float32))
    for j in (1, 2, 4):
        assert torch.equal(got[j], ref[j]), (route, j)
    for a, b in ((got[0], ref[0]), (got[3], ref[3]), (got[5]["obs_pos"], ref[5]["obs_pos"])):
        assert torch.equal(_crops(ops, a, B), _crops(ops, b, B)), route
    if got[0].pair is not None:
        assert torch.equal(_crops(ops, got[0].pair[0], 2 * B), _crops(ops, ref[0].pair[0], 2 * B))
    got = per.sample_cpc(indices=(u, offs))
    ref = twin.sample_cpc(indices=(want, offs))
    assert np.array_equal(got[0].per.rows.cpu().numpy(), want)
    for j in range(5):
        assert torch.equal(got[j], ref[j]), (route, j)
    assert torch.equal(got[5]["obs_pos"], ref[5]["obs_pos"]) and got[5]["obs_anchor"] is got[0]
    # save (the reference's payload, from the plain twin), then: a wrapped add resets its row to the maximum
    twin.save(str(tmp_path))
    per.add_batch(*(a[n:cap] for a in ep))
    assert per.full and per.idx == 0 and (per.priorities()[n:] == 8.0).all()
    per.update_priorities(_dev(np.array([0, 1], dtype=np.int64)), _dev(np.array([2.0, 3.0], dtype=np.float32)))
    before = per.priorities()
    assert before[0] == 2.0 and before[1] == 3.0
    per.add(*(a[cap] for a in ep))
    after = per.priorities()
    before[0] = 8.0
    assert np.array_equal(after, before)
    # load: every loaded row gets the maximum, the others stay 0
    fresh = mk(prioritized=True)
    fresh._per_max.fill_(4.0)
    fresh.load(str(tmp_path))
    assert fresh.idx == n and np.array_equal(fresh.priorities(), np.full(n, 4.0, dtype=np.float32))
    assert not fresh._per_s[n:].any() and fresh._per_sums.sum().item() == 4.0 * n


# ------------------------------------------------------------------------------------------------- 5. through the agent
AGENT_B, IN_HW, OUT_HW = 32, (40, 44), (32, 36)


def _build(seed=5, B=AGENT_B, **rb_kw):
    import curla_amd
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    np.random.seed(seed)
    dev = torch.device("cuda")
    aug = curla_amd.RandomCrop(IN_HW, OUT_HW)
    agent = curla_amd.CurlSacAgent((9,) + OUT_HW, (2,), dev, aug, hidden_dim=64, **HP)
    rb = curla_amd.ReplayBuffer((9,) + IN_HW, (2,), 512, B, dev, aug, **rb_kw)
    rb.add_batch(*_episode(400, 3, IN_HW, 6))
    return agent, rb


def test_equal_priorities_are_the_plain_update():
    """per_alpha = 0 keeps every stored value at 1, so all w = 1 in every update: three updates of a prioritized agent
    against a plain agent fed the same rows -- they differ only in the unfused loss launch."""
    agent_p, rb_p = _build(prioritized=True, per_alpha=0.0, per_beta=1.0)
    draws, rec_p = [], []
    L = NullLogger()
    for step in range(3):
        s = rb_p.priorities()
        assert (s == 1.0).all()
        u, offs = rb_p.draw_indices()
        rows, _ = numpy_rows(s, u)
        sample = rb_p.sample_cpc_refs(indices=(u, offs))
        assert np.array_equal(sample[0].per.rows.cpu().numpy(), rows)
        agent_p._update_phases(sample, L, step)
        assert torch.equal(agent_p._ws(AGENT_B).per_w, torch.ones(AGENT_B, device="cuda"))
        draws.append((rows, offs))
        rec_p.append((agent_p._critic_gflat.clone(), dict(L.scalars)))
    agent_0, rb_0 = _build()
    L = NullLogger()
    for step in range(3):
        agent_0._update_phases(rb_0.sample_cpc_refs(indices=draws[step]), L, step)
        g, scalars = rec_p[step]
        e = rel_err(g, agent_0._critic_gflat)
        print(f"equal priorities, update {step}: critic gradient rel err {e:.3e}")
        assert e <= RTOL
        losses = [k for k in L.scalars if "loss" in k]
        assert "train_critic/loss" in losses and set(L.scalars) == set(scalars)
        for k in losses:
            print(f"equal priorities, update {step}: {k} {scalars[k]!r} against {L.scalars[k]!r}")
            assert abs(scalars[k] - L.scalars[k]) <= RTOL * abs(L.scalars[k]), (step, k)
    for name in ("_critic_flat", "_target_flat", "_actor_flat"):
        e = rel_err(getattr(agent_p, name), getattr(agent_0, name))
        print(f"equal priorities, after three updates: {name} rel err {e:.3e}")
        assert e <= RTOL, name
    assert agent_0._ws(AGENT_B).per_w is None


def test_unequal_priorities_weight_the_critic_gradient():
    """The critic gradient of a prioritized update against loss.backward() on the weighted loss through the
    differentiable Critic, t and w taken from the update's workspace; the unweighted loss gives another gradient."""
    agent, rb = _build(prioritized=True, per_beta=1.0)
    rs = np.random.RandomState(2)
    rb.update_priorities(torch.arange(400, device="cuda"), _dev(rs.randint(1, 20, 400).astype(np.float32)))
    obs, act, rew, nxt, nd, _ = rb.sample_cpc()
    assert obs.per is not None
    agent.critic_optimizer.step = lambda: None  # gradients before Adam moves the weights
    L = NullLogger()
    agent.update_critic(obs, act, rew, nxt, nd, L, 1)
    ws = agent._ws(AGENT_B)
    got = grads_of(agent.critic)
    t, w = ws.target_q.clone(), ws.per_w.clone().view(-1, 1)
    prob = obs.per.prob.cpu().numpy().astype(np.float64)
    assert (np.abs(w.view(-1).cpu().numpy() - prob.min() / prob) <= TOL * (prob.min() / prob)).all() and w.min() < 0.5

    def grads(weights):
        agent.critic_optimizer.zero_grad()
        q1, q2 = agent.critic(obs, act)
        loss = (weights * (q1 - t) ** 2).mean() + (weights * (q2 - t) ** 2).mean()
        loss.backward()
        return loss.item(), grads_of(agent.critic)
    loss_w, ref = grads(w)
    assert abs(L.scalars["train_critic/loss"] - loss_w) <= RTOL * abs(loss_w)
    _, plain = grads(torch.ones_like(w))
    assert set(got) == set(ref)
    for k in ref:
        e = rel_err(got[k], ref[k])
        print(f"weighted critic gradient {k}: rel err {e:.3e}; the unweighted one is {rel_err(plain[k], ref[k]):.3e} away")
        assert np.isfinite(e) and e <= RTOL, (k, e)
    assert max(rel_err(plain[k], ref[k]) for k in ref) > 1e-2


def _prioritized_run(seed):
    """Three whole updates of a default prioritized buffer; per update the drawn rows, q and t as the critic phase
    left them, and the priorities before and after."""
    agent, rb = _build(seed=seed, prioritized=True)
    ws = agent._ws(AGENT_B)
    inner, seen, records = agent.update_critic, {}, []

    def update_critic(obs, *a, **k):
        inner(obs, *a, **k)
        seen.update(rows=obs.per.rows.cpu().numpy().copy(), q=ws.q.cpu().numpy().reshape(2, -1).astype(np.float64),
                    t=ws.target_q.cpu().numpy().reshape(-1).astype(np.float64))
    agent.update_critic = update_critic
    L = NullLogger()
    for step in range(3):
        before = rb.priorities()
        agent.update(rb, L, step)
        records.append(dict(seen, before=before, after=rb.priorities()))
    torch.cuda.synchronize()
    return records, _state(agent, rb), rb


@pytest.fixture(scope="module")
def two_runs():
    return _prioritized_run(5), _prioritized_run(5)


def test_priorities_after_each_update(two_runs):
    (records, _, rb), _ = two_runs
    alpha, eps = np.float64(np.float32(rb.per_alpha)), np.float64(np.float32(rb.per_eps))
    top = 1.0
    for step, r in enumerate(records):
        cand = (0.5 * (np.abs(r["q"][0] - r["t"]) + np.abs(r["q"][1] - r["t"])) + eps) ** alpha
        want = r["before"].astype(np.float64)
        want[r["rows"]] = 0
        np.maximum.at(want, r["rows"], cand)
        drawn = np.zeros(len(want), dtype=bool)
        drawn[r["rows"]] = True
        assert (r["before"][r["rows"]] > 0).all()
        err = np.abs(r["after"][drawn] - want[drawn]) / want[drawn]
        print(f"priorities after update {step}: {drawn.sum()} rows drawn, max rel err {err.max():.3e}")
        assert (err <= TOL).all(), (step, err.max())
        assert np.array_equal(r["after"][~drawn], r["before"][~drawn]), step  # every other row: untouched
        top = max(top, cand.max())
    assert abs(rb._per_max.item() - top) <= TOL * top  # the largest value ever given, 1.0 included


def test_two_seeded_runs_are_bit_identical(two_runs):
    (rec_a, state_a, rb_a), (rec_b, state_b, rb_b) = two_runs
    assert set(state_a) == set(state_b)
    for k in state_a:
        assert torch.equal(state_a[k], state_b[k]), k  # parameters, optimizer state, the NumPy and torch streams
    for a, b in zip(rec_a, rec_b):
        assert np.array_equal(a["rows"], b["rows"]) and np.array_equal(a["after"], b["after"])
    assert torch.equal(rb_a._per_s, rb_b._per_s) and torch.equal(rb_a._per_sums, rb_b._per_sums)
    assert torch.equal(rb_a._per_max, rb_b._per_max)


# ------------------------------------------------------------------------------------------------- 6. off means off
def _counted_run(**rb_kw):
    import curla_amd.ops as ops_mod
    import curla_amd.optim as optim_mod
    from curla_amd import _lib
    agent, rb = _build(**rb_kw)
    real_call, counter = _lib.call, collections.Counter()

    def traced(name, *a):
        counter[name] += 1
        return real_call(name, *a)
    for m in (ops_mod, optim_mod):
        m.call = traced
    try:
        L = NullLogger()
        for step in range(3):
            agent.update(rb, L, step)
        torch.cuda.synchronize()
    finally:
        for m in (ops_mod, optim_mod):
            m.call = real_call
    return _state(agent, rb), counter, rb, agent


OFF_FIXTURE = os.path.join(GOLDEN, "per_off_state.json")


def off_state_digests():
    """Three whole updates of a buffer constructed WITHOUT the prioritized keywords, from the golden tiny agent (its
    parameters come from the fixture, not from an initialiser) on a seeded stream, and the sha256 of every recorded state
    tensor.  tests/golden/per_off_state.json holds what the commit before prioritized replay gave."""
    import curla_amd
    agent, aug = _tiny_agent(load("tiny.npz"))
    torch.manual_seed(7)
    torch.cuda.manual_seed_all(7)
    np.random.seed(7)
    rb = curla_amd.ReplayBuffer((9, 34, 40), (2,), 64, 8, torch.device("cuda"), aug)
    rb.add_batch(*_episode(48, 3, (34, 40), 6))
    L = NullLogger()
    for step in range(3):
        agent.update(rb, L, step)
    torch.cuda.synchronize()
    return {k: hashlib.sha256(v.contiguous().numpy().tobytes()).hexdigest() for k, v in _state(agent, rb).items()}


def test_off_is_the_parent_commits_update_bit_for_bit():
    with open(OFF_FIXTURE) as f:
        want = json.load(f)
    got = off_state_digests()
    assert set(got) == set(want)
    assert [k for k in sorted(want) if got[k] != want[k]] == []


def test_off_means_off():
    s0, c0, rb0, _ = _counted_run()
    s1, c1, rb1, agent = _counted_run(prioritized=False, per_alpha=0.1, per_beta=1.0, per_eps=0.5)
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k
    assert c0 == c1 and not any(c1[n] for n in NEW)
    assert c1["curla_mlp_out_bwd_loss"] > 0 and c1["curla_critic_td_loss"] == 0  # the fused loss-in-backward launch
    for rb in (rb0, rb1):
        assert not any(k.startswith("_per") for k in vars(rb))
    assert agent._ws(AGENT_B).per_w is None
    on_state, on, rb_on, _ = _counted_run(prioritized=True)
    assert on["curla_per_sample"] == 3 and on["curla_per_td"] == 3 and on["curla_per_set"] == 3
    assert on["curla_critic_td_loss"] == 3 and rb_on._per_s.numel() == 512 and rb_on._h_index_dev is None
