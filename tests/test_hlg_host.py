"""CurlSacAgent(critic_bins=M, critic_value_range=(v_min, v_max), critic_bin_sigma=s) on the host: the
float64 reference of the HL-Gauss losses (tests/_hlg_ref.py) against plain Python loops and against the properties of
the definition, a float32 evaluation of the definition against it, the keywords' defaults and validation, the state-dict
contract and what a seed reproduces, the two C entry points (declared, bound, exported, argument checks) and the launch
list of an update under the trace hook.  No GPU: nothing here launches a kernel."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import _hlg_ref as R
from tests._util import RTOL, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("curla_hlg_critic_loss", "curla_hlg_actor_loss")
F_, A_, H_ = 50, 2, 96
RANGE = (-4.0, 6.0)


def make_agent(seed=1, hidden=H_, **kw):
    import curla_amd
    torch.manual_seed(seed)
    return curla_amd.CurlSacAgent((9, 32, 36), (A_,), torch.device("cpu"), None, hidden_dim=hidden, num_layers=2,
                                  num_filters=8, **kw)


def _inputs(B, M, seed=0, bin_sigma=0.75, v=RANGE):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return dict(q=2.0 * r(2, B, M), tq=2.0 * r(2, B, M), log_pi=r(B), reward=2.0 * r(B),
                not_done=(torch.arange(B) % 3 != 1).float(), log_alpha=torch.tensor(np.log(0.3)), discount=0.97,
                v_min=v[0], v_max=v[1], sigma=bin_sigma * (v[1] - v[0]) / M)


# ------------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("views", [False, True])
@pytest.mark.parametrize("M,bin_sigma", [(2, 0.75), (3, 0.3), (5, 2.0), (17, 0.75)])
def test_reference_against_plain_loops(M, bin_sigma, views):
    x = _inputs(6, M, seed=M, bin_sigma=bin_sigma)
    ref = R.critic_loss(views=views, **x)
    loss, dq, rows, t = R.critic_loss_loops(views=views, **x)
    assert abs(float(ref["loss"]) - loss) <= 1e-12 * abs(loss)
    assert np.abs(ref["dq"].numpy() - dq).max() <= 1e-12 * np.abs(dq).max()
    assert np.abs(ref["row_loss"].numpy() - rows).max() <= 1e-12 * np.abs(rows).max()
    assert np.abs(ref["t"].numpy() - t).max() <= 1e-12
    if views:
        assert torch.equal(ref["target_q"][:3], ref["target_q"][3:])
    a = R.actor_loss(x["q"], x["log_pi"], torch.zeros(6, A_), x["log_alpha"], -2.0, *RANGE)
    a_loss, a_dq = R.actor_loss_loops(x["q"], x["log_pi"], x["log_alpha"], *RANGE)
    assert abs(float(a["actor_loss"]) - a_loss) <= 1e-12 * abs(a_loss)
    assert np.abs(a["dq"].numpy() - a_dq).max() <= 1e-12 * np.abs(a_dq).max()


@pytest.mark.parametrize("M", [2, 3, 51, 64, 65, 255, 256])
@pytest.mark.parametrize("bin_sigma", [0.3, 0.75, 2.0])
def test_target_rows_sum_to_one_and_keep_the_mean(M, bin_sigma):
    """Every t row sums to 1; for y at least 3 sigma inside the range the histogram's mean sum_j t_j c_j is within one
    bin width of y (the bins' quantisation: the Gaussian's own mean is y, what the range cuts off is below 0.3 %)."""
    w, _, c = R.grid(M, *RANGE)
    sigma = bin_sigma * w
    y = torch.linspace(RANGE[0], RANGE[1], 41, dtype=torch.float64)
    t = R.target_probs(y, M, *RANGE, sigma)
    assert float((t.sum(1) - 1).abs().max()) <= 1e-12 and float(t.min()) >= 0
    inside = (y >= RANGE[0] + 3 * sigma) & (y <= RANGE[1] - 3 * sigma)
    if inside.any():
        assert float(((t * c).sum(1) - y)[inside].abs().max()) <= w
    assert inside.any() or 6 * sigma > RANGE[1] - RANGE[0]


def test_the_tie_splits_the_actor_gradient_and_the_critic_gradient_sums_to_zero():
    x = _inputs(4, 5, seed=3)
    q = x["q"].clone()
    q[1, 2] = q[0, 2]  # row 2: both networks hold the same logits
    a = R.actor_loss(q, x["log_pi"], torch.zeros(4, A_), x["log_alpha"], -2.0, *RANGE)
    assert torch.equal(a["dq"][0, 2], a["dq"][1, 2]) and float(a["dq"][0, 2].abs().max()) > 0
    for b in (0, 1, 3):  # elsewhere the larger network gets nothing
        big = int(a["q_values"][1, b] > a["q_values"][0, b])
        assert not a["dq"][big, b].any() and a["dq"][1 - big, b].any()
    assert float(a["dq"].sum(-1).abs().max()) <= 1e-15  # (through a softmax: every row sums to 0)
    ref = R.critic_loss(**x)
    assert float(ref["dq"].sum(-1).abs().max()) <= 1e-15


@pytest.mark.parametrize("M", [2, 51, 256])
@pytest.mark.parametrize("bin_sigma", [0.3, 0.75, 2.0])
def test_a_float32_evaluation_stays_far_inside_rtol(M, bin_sigma):
    """The definition evaluated by torch in float32 (erf, exp, log in single precision, as the kernels') against float64:
    the errors are printed; RTOL has to hold with a wide margin for the GPU tests to need no tolerance of their own."""
    x = _inputs(16, M, seed=M, bin_sigma=bin_sigma)
    ref = R.critic_loss(**x)
    f = lambda t: torch.as_tensor(t, dtype=torch.float32)  # noqa: E731
    v_min, v_max, sigma = (f(x[k]) for k in ("v_min", "v_max", "sigma"))
    w = (v_max - v_min) / M
    j = torch.arange(M + 1, dtype=torch.float32)
    e, c = v_min + j * w, v_min + (j[:M] + 0.5) * w
    qt = (torch.softmax(x["tq"], -1) * c).sum(-1)
    alpha = torch.tensor(np.float32(np.exp(float(x["log_alpha"]))))
    y = x["reward"] + x["not_done"] * f(x["discount"]) * (torch.minimum(qt[0], qt[1]) - alpha * x["log_pi"])
    y = y.clamp(float(v_min), float(v_max))
    er = torch.erf((e[None] - y[:, None]) * (f(0.70710678118654752) / sigma))
    t = (er[:, 1:] - er[:, :-1]) / (er[:, -1:] - er[:, :1])
    logp = torch.log_softmax(x["q"], -1)
    rows = -(t[None] * logp).sum(dim=(0, 2))
    dq = (logp.exp() - t[None]) / 16
    errs = dict(loss=rel_err(rows.sum().reshape(1) / 16, ref["loss"].reshape(1)), row_loss=rel_err(rows, ref["row_loss"]),
                t=rel_err(t, ref["t"]), dq=rel_err(dq, ref["dq"]))
    print(f"M{M} bin_sigma {bin_sigma}:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= RTOL / 10


# ------------------------------------------------------------------------------------------------ keywords, validation
def test_keywords_and_defaults():
    import curla_amd
    from curla_amd import ops
    from curla_amd.curl_sac import Critic, QFunction
    assert ops.HLG_MAX == 256
    init = list(inspect.signature(curla_amd.CurlSacAgent.__init__).parameters)
    assert init[-1] == "pixel_sac" and not any(k.startswith("critic_bin") or k == "critic_value_range" for k in init)
    call = inspect.signature(curla_amd.CurlSacAgent).parameters
    for k, default in (("critic_bins", 0), ("critic_value_range", None), ("critic_bin_sigma", 0.75)):
        assert call[k].default == default and call[k].kind is inspect.Parameter.KEYWORD_ONLY
    for cls in (Critic, QFunction):
        p = inspect.signature(cls).parameters["bins"]
        assert p.default == 0 and p.kind is inspect.Parameter.KEYWORD_ONLY
        assert "bins" not in inspect.signature(cls.__init__).parameters
    off = make_agent()
    assert off.critic_bins == 0 and off.critic_value_range is None and off.critic.bins == 0 and off.critic.out_dim == 1
    on = make_agent(critic_bins=np.int64(51), critic_value_range=[-4, np.float32(6)])
    assert type(on.critic_bins) is int and on.critic_bins == 51 and on.critic_value_range == (-4.0, 6.0)
    assert on.critic_bin_sigma == 0.75 and on.critic.out_dim == on.critic_target.out_dim == 51
    assert on.critic.Q2.bins == 51 and on.critic.quantiles == 0
    for text in (curla_amd.CurlSacAgent.__doc__, open(os.path.join(ROOT, "README.md")).read()):
        assert all(k in text for k in ("critic_bins", "critic_value_range", "critic_bin_sigma"))
    assert "7l" in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_an_agent_with_bins_off_is_the_agent_without_the_keyword():
    plain, off = make_agent(), make_agent(critic_bins=0)
    assert sorted(plain.__dict__) == sorted(off.__dict__)
    assert sorted(plain.critic.__dict__) == sorted(off.critic.__dict__)
    assert sorted(plain.critic.Q1.__dict__) == sorted(off.critic.Q1.__dict__)
    assert plain._graph_key() == off._graph_key()
    on = make_agent(critic_bins=5, critic_value_range=RANGE)
    assert set(on.__dict__) - set(plain.__dict__) == {"critic_bins", "critic_value_range", "critic_bin_sigma"}
    k = on._graph_key()
    assert k[-1] == ("bins", 5, -4.0, 6.0, 0.75) and k[:-1] == plain._graph_key()
    on.critic_bin_sigma = 1.5
    on.critic_value_range = (-1, 1)
    assert on._graph_key()[-1] == ("bins", 5, -1.0, 1.0, 1.5)


@pytest.mark.parametrize("bad", [-1, 1, 257, 2.0, True, "5", None])
def test_bins_validation(bad):
    from curla_amd.curl_sac import Critic, QFunction
    with pytest.raises(ValueError, match="bins"):
        make_agent(critic_bins=bad, critic_value_range=RANGE)
    with pytest.raises(ValueError, match="bins"):
        Critic((9, 32, 36), (A_,), H_, F_, 2, 8, bins=bad)
    with pytest.raises(ValueError, match="bins"):
        QFunction(F_, A_, H_, bins=bad)


@pytest.mark.parametrize("bad", [None, (1.0, 1.0), (2.0, 1.0), (0.0, float("inf")), (float("nan"), 1.0), (1.0,), 3.0, "ab",
                                 (0.0, 1.0, 2.0)])
def test_value_range_validation(bad):
    with pytest.raises(ValueError, match="critic_value_range"):
        make_agent(critic_bins=5, critic_value_range=bad)


@pytest.mark.parametrize("bad", [0, 0.0, -0.5, float("inf"), float("nan"), "0.75", None, True])
def test_bin_sigma_validation(bad):
    with pytest.raises(ValueError, match="critic_bin_sigma"):
        make_agent(critic_bins=5, critic_value_range=RANGE, critic_bin_sigma=bad)


def test_exclusive_keywords_and_a_range_without_bins():
    from curla_amd.curl_sac import Critic, QFunction
    with pytest.raises(ValueError, match="critic_quantiles"):
        make_agent(critic_bins=5, critic_value_range=RANGE, critic_quantiles=5)
    with pytest.raises(ValueError, match="critic_value_range"):
        make_agent(critic_value_range=RANGE)
    with pytest.raises(ValueError, match="quantiles"):
        Critic((9, 32, 36), (A_,), H_, F_, 2, 8, bins=5, quantiles=5)
    with pytest.raises(ValueError, match="quantiles"):
        QFunction(F_, A_, H_, bins=5, quantiles=5)
    assert make_agent(critic_bins=5, critic_value_range=RANGE, aug_views=2).aug_views == 2  # (where TQC refuses)


def test_limits_build():
    assert make_agent(critic_bins=256, critic_value_range=RANGE).critic.Q1.trunk[-1].out_features == 256
    assert make_agent(critic_bins=2, critic_value_range=RANGE).critic.Q1.trunk[-1].out_features == 2


def test_edited_attributes_are_checked_by_update_critic_before_anything_runs():
    x = torch.zeros(4, 9, 32, 36)
    for edit in (dict(critic_value_range=(1.0, 1.0)), dict(critic_bin_sigma=0.0), dict(critic_bin_sigma=float("nan"))):
        agent = make_agent(critic_bins=5, critic_value_range=RANGE)
        for k, v in edit.items():
            setattr(agent, k, v)
        with pytest.raises(ValueError, match=next(iter(edit))):
            agent.update_critic(x, torch.zeros(4, A_), torch.zeros(4, 1), x, torch.ones(4, 1), None, 1)


def test_bin_centres_and_expected():
    from curla_amd.curl_sac import Critic
    agent = make_agent(critic_bins=5, critic_value_range=RANGE)
    c = agent.critic.bin_centres()
    assert c.dtype == torch.float32 and c.shape == (5,)
    assert torch.equal(c, torch.tensor([-3.0, -1.0, 1.0, 3.0, 5.0]))
    logits = torch.randn(3, 5, generator=torch.Generator().manual_seed(0), requires_grad=True)
    q = agent.critic.expected(logits)
    assert q.shape == (3, 1)
    assert rel_err(q.detach().reshape(3), R.expected(logits.detach(), 5, *RANGE)) <= 1e-6
    q.sum().backward()
    p = torch.softmax(logits.detach().double(), -1)
    want = p * (c.double() - (p * c.double()).sum(-1, keepdim=True))
    assert rel_err(logits.grad, want) <= 1e-5
    agent.critic_value_range = (0.0, 10.0)  # an edit reaches the critics with the next phase's check
    agent._hlg_params()
    assert torch.equal(agent.critic_target.bin_centres(), torch.tensor([1.0, 3.0, 5.0, 7.0, 9.0]))
    with pytest.raises(RuntimeError, match="bins"):
        make_agent().critic.bin_centres()
    with pytest.raises(RuntimeError, match="value_range"):
        Critic((9, 32, 36), (A_,), H_, F_, 2, 8, bins=5).bin_centres()
    with pytest.raises(RuntimeError, match="critic_bins"):
        make_agent().target_clip_fraction()
    with pytest.raises(RuntimeError, match="no critic phase"):
        agent.target_clip_fraction()


# --------------------------------------------------------------------------------------------------------- state dicts
@pytest.mark.parametrize("ln", [False, True])
def test_state_dict_keys_are_unchanged_and_the_last_layers_have_m_rows(ln):
    M = 51
    off, on = make_agent(critic_layer_norm=ln), make_agent(critic_layer_norm=ln, critic_bins=M, critic_value_range=RANGE)
    last = "trunk.6." if ln else "trunk.4."
    for name in ("critic", "critic_target"):
        a, b = getattr(off, name).state_dict(), getattr(on, name).state_dict()
        assert list(a) == list(b)
        for k in a:
            if last in k:
                assert tuple(b[k].shape) == ((M, H_) if k.endswith("weight") else (M,))
            else:
                assert torch.equal(a[k], b[k]), (name, k)  # the same seed: the same other tensors
    for k, v in on.critic.state_dict().items():
        assert torch.equal(v, on.critic_target.state_dict()[k]), k
    a, b = off.actor.state_dict(), on.actor.state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert torch.equal(off.CURL.W, on.CURL.W) and torch.equal(off.log_alpha, on.log_alpha)
    torch.manual_seed(1)
    make_agent(critic_bins=M, critic_value_range=RANGE)
    after_on = torch.rand(3)
    torch.manual_seed(1)
    make_agent()
    assert torch.equal(after_on, torch.rand(3))
    with pytest.raises(RuntimeError, match="size mismatch"):
        make_agent(critic_layer_norm=ln, critic_bins=5, critic_value_range=RANGE).critic.load_state_dict(on.critic.state_dict())


def test_reset_networks_draws_critics_of_the_same_width():
    agent = make_agent(critic_bins=7, critic_value_range=RANGE)
    _, critic, _ = agent._draw_fresh()
    assert critic.out_dim == 7 and critic.Q1.trunk[-1].weight.shape == (7, H_) and critic.value_range == RANGE


def test_checkpoint_carries_the_range_and_the_smoothing(tmp_path):
    agent = make_agent(critic_bins=5, critic_value_range=RANGE, critic_bin_sigma=1.25)
    ck = tmp_path / "hlg.pt"
    agent.save_checkpoint(str(ck), 7)
    saved = torch.load(str(ck), map_location="cpu", weights_only=False)
    assert saved["critic_bins"] == 5 and saved["critic_value_range"] == RANGE and saved["critic_bin_sigma"] == 1.25
    other = make_agent(seed=2, critic_bins=5, critic_value_range=(0.0, 1.0))
    assert other.load_checkpoint(str(ck)) == 7
    assert other.critic_value_range == RANGE and other.critic_bin_sigma == 1.25 and other.critic.value_range == RANGE
    with pytest.raises(RuntimeError, match="size mismatch"):
        make_agent(critic_bins=6, critic_value_range=RANGE).load_checkpoint(str(ck))
    plain = tmp_path / "plain.pt"
    make_agent().save_checkpoint(str(plain), 1)
    assert not any(k.startswith("critic_bin") or k == "critic_value_range"
                   for k in torch.load(str(plain), map_location="cpu", weights_only=False))


# -------------------------------------------------------------------------------------------------------- entry points
def test_entry_points_are_declared_bound_and_exported():
    import __graft_entry__ as ge
    ge.build()
    from curla_amd import _lib, ops
    text = open(os.path.join(ROOT, "include", "curla_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int %s\(([^;]*)\);" % name, text, flags=re.S)
        assert m, f"include/curla_hip.h does not declare {name} behind a comment"
        comment = " ".join(m.group(1).replace("*", " ").split())
        assert "Additive: CURLA_ABI_VERSION stays 8" in comment
        params = [p.strip() for p in m.group(2).split(",")]
        assert len(params) == len(_lib.SIGNATURES[name])
        for p, t in zip(params, _lib.SIGNATURES[name]):
            want = (_lib.vp if "*" in p else _lib.c_ll if p.startswith("long long") else _lib.c_float
                    if p.startswith("float") else _lib.c_int)
            assert t is want, (name, p)
        assert hasattr(lib, name)
    assert _lib.ABI_VERSION == 8 and _lib.load().curla_abi_version() == 8
    assert callable(ops.hlg_critic_loss) and callable(ops.hlg_actor_loss)
    kernels = open(os.path.join(ROOT, "curla_amd", "csrc", "hlgauss.h")).read()
    assert "hlg_critic_loss_kernel" in kernels and "atomic" not in kernels.replace("No atomics", "")
    heads = open(os.path.join(ROOT, "curla_amd", "csrc", "heads.hip")).read()
    assert heads.index('#include "reduce.h"') < heads.index('#include "hlgauss.h"')


def test_entry_points_check_their_arguments_before_any_launch():
    """CURLA_ERR_ARG (-1) on a NULL required pointer, B < 1, M outside 2 .. 256, v_min >= v_max or a non-finite bound,
    sigma <= 0 or not finite, twin strides below B M, odd B with views -- all decided on the host, so a machine without
    a GPU sees them too (the pointers are never dereferenced)."""
    from curla_amd import _lib
    lib = _lib.load()
    p = 4096  # a non-NULL, aligned, never dereferenced address
    inf, nan = float("inf"), float("nan")

    def critic(q=p, tq=p, lp=p, r=p, nd=p, la=p, dq=p, t=p, rl=p, B=4, M=5, lo=-1.0, hi=1.0, s=0.3, views=0, sq=None, st=None,
               sd=None):
        dense = B * M
        return lib.curla_hlg_critic_loss(q, dense if sq is None else sq, tq, dense if st is None else st, lp, r, nd, la,
                                         0.99, B, M, lo, hi, s, views, dq, dense if sd is None else sd, t, rl, None, None)

    def actor(q=p, lp=p, ls=p, la=p, rq=p, sc=p, dq=p, B=4, M=5, A=2, lo=-1.0, hi=1.0, sq=None, sd=None):
        dense = B * M
        return lib.curla_hlg_actor_loss(q, dense if sq is None else sq, lp, ls, A, la, -2.0, B, M, lo, hi, rq, sc, dq,
                                        dense if sd is None else sd, None, None)
    for bad in (dict(q=None), dict(tq=None), dict(lp=None), dict(r=None), dict(nd=None), dict(la=None), dict(dq=None),
                dict(t=None), dict(rl=None), dict(B=0), dict(M=0), dict(M=1), dict(M=257), dict(lo=1.0), dict(lo=2.0),
                dict(hi=inf), dict(lo=-inf), dict(lo=nan), dict(hi=nan), dict(s=0.0), dict(s=-1.0), dict(s=inf), dict(s=nan),
                dict(sq=19), dict(st=19), dict(sd=19), dict(B=5, views=1), dict(views=2)):
        assert critic(**bad) == -1, bad
    for bad in (dict(q=None), dict(lp=None), dict(ls=None), dict(la=None), dict(rq=None), dict(sc=None), dict(dq=None),
                dict(B=0), dict(M=1), dict(M=257), dict(A=0), dict(lo=1.0), dict(hi=nan), dict(lo=-inf), dict(sq=19),
                dict(sd=19)):
        assert actor(**bad) == -1, bad


# --------------------------------------------------------------------------------------------------------- launch list
def _traced_update(step, views=1, prioritized=False, **kw):
    """The launch list of one update() of a CPU agent under the trace hook (nothing is computed)."""
    import curla_amd
    from curla_amd import _lib
    aug = curla_amd.RandomCrop((34, 40), (28, 34))
    curla_amd.set_seed_everywhere(1)
    v = dict(aug_views=2) if views == 2 else {}
    agent = curla_amd.CurlSacAgent((9, 28, 34), (2,), "cpu", aug, hidden_dim=64, log_interval=100, **v, **kw)
    rb = curla_amd.ReplayBuffer((9, 34, 40), (2,), 32, 8, "cpu", aug, **v, **(dict(prioritized=True) if prioritized else {}))
    for _ in range(12):
        rb.add(np.zeros((9, 34, 40), np.uint8), [0, 0], 0.0, np.zeros((9, 34, 40), np.uint8), False)

    class Log:
        def log(self, *a, **k):
            pass
    calls = []
    _lib.set_trace_hook(lambda name, args: calls.append((name, args)))
    try:
        agent.update(rb, Log(), step)
    finally:
        _lib.set_trace_hook(None)
    return agent, calls


@pytest.mark.parametrize("step", [2, 1])
@pytest.mark.parametrize("M,views", [(5, 1), (51, 1), (5, 2)])
def test_launch_list_contains_the_bins_losses(step, M, views):
    """The critic phase launches the HL-Gauss loss in place of the fused loss-in-backward launch (of the views loss with
    aug_views = 2), the actor phase (even steps) its own, and every other launch is the one of a TQC agent of the same
    width; with the keyword off the launch list is the one of an agent without it."""
    _, off = _traced_update(step, views=views)
    _, off0 = _traced_update(step, views=views, critic_bins=0)
    assert [n for n, _ in off] == [n for n, _ in off0]
    agent, on = _traced_update(step, views=views, critic_bins=M, critic_value_range=RANGE, critic_bin_sigma=0.5)
    names_off, names_on = [n for n, _ in off], [n for n, _ in on]
    assert not any(n in ENTRY_POINTS for n in names_off)
    even = step % 2 == 0
    assert names_on.count(ENTRY_POINTS[0]) == 1 and names_on.count(ENTRY_POINTS[1]) == (1 if even else 0)
    assert not any(n in names_on for n in ("curla_mlp_out_bwd_loss", "curla_critic_td_loss", "curla_critic_td_loss_views",
                                           "curla_actor_loss"))
    B = 8
    ws = agent._ws(B)
    assert ws.q2.shape == (2, 2, B, M) and ws.dq.shape == (2, B, M) and ws.q_row_loss.shape == (B,)
    a = dict(on)[ENTRY_POINTS[0]]
    assert a[0] == ws.q.data_ptr() and a[2] == ws.tq.data_ptr() and a[1] == a[3] == a[16] == B * M
    assert a[9:11] == (B, M) and a[11:13] == RANGE and a[13] == 0.5 * (RANGE[1] - RANGE[0]) / M and a[14] == views - 1
    assert a[15] == ws.dq.data_ptr() and a[17] == ws.target_q.data_ptr() and a[18] == ws.q_row_loss.data_ptr()
    assert a[19] == ws.scalars.data_ptr()  # scalars[0]: the logged train_critic/loss
    if even:
        a = dict(on)[ENTRY_POINTS[1]]
        assert a[0] == ws.q.data_ptr() and a[1] == a[14] == B * M and a[7:9] == (B, M) and a[9:11] == RANGE
        assert a[11] == ws.q_row_loss.data_ptr() and a[12] == ws.scalars.data_ptr() + 4 and a[13] == ws.dq.data_ptr()
    if views == 1:  # the other launches: a TQC agent's of the same width (M <= 32 there)
        _, tqc = _traced_update(step, critic_quantiles=5)
        swap = {"curla_tqc_critic_loss": ENTRY_POINTS[0], "curla_tqc_actor_loss": ENTRY_POINTS[1]}
        if M == 5:
            assert [swap.get(n, n) for n, _ in tqc] == names_on
    i = names_on.index(ENTRY_POINTS[0])
    small = M <= 16
    assert names_on[i + 1] == ("curla_mlp_out_bwd" if small else "curla_gemm")


def test_a_prioritized_minibatch_and_quantiles_are_refused_before_any_launch():
    import curla_amd
    from curla_amd import _lib
    with pytest.raises(ValueError, match="prioritized"):
        _traced_update(1, prioritized=True, critic_bins=5, critic_value_range=RANGE)
    aug = curla_amd.RandomCrop((34, 40), (28, 34))
    agent = curla_amd.CurlSacAgent((9, 28, 34), (2,), "cpu", aug, hidden_dim=64, critic_bins=5, critic_value_range=RANGE)

    class Per:
        pass
    obs = torch.zeros(4, 9, 28, 34)

    class Tagged(torch.Tensor):
        pass
    calls = []
    _lib.set_trace_hook(lambda name, args: calls.append(name))
    try:
        o = obs.as_subclass(Tagged)
        o.per = Per()
        with pytest.raises(ValueError, match="prioritized"):
            agent.update_critic(o, torch.zeros(4, 2), torch.zeros(4, 1), obs, torch.ones(4, 1), None, 1)
    finally:
        _lib.set_trace_hook(None)
    assert calls == []


def test_an_agent_with_bins_off_has_no_bins_buffers():
    agent, _ = _traced_update(1, critic_bins=0)
    assert agent._ws(8).q_row_loss is None and agent._ws(8).q2.shape == (2, 2, 8, 1) and agent._hlg_last_B is None
    assert not any(isinstance(k, tuple) and k and k[0] == "bins" for k in agent._graph_key())
    on, _ = _traced_update(1, critic_bins=5, critic_value_range=RANGE)
    assert on._hlg_last_B == 8 and on._ws(8).q_row_loss.shape == (8,)
