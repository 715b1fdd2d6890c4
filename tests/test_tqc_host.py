"""CurlSacAgent(critic_quantiles=M, critic_drop_quantiles=d) on the host: the float64 reference of the quantile loss
(tests/_tqc_ref.py) against plain Python loops and on rows that show the truncation by value, the keywords' positions,
defaults and validation, the state-dict contract and what a seed reproduces, the two C entry points (declared, bound,
exported, argument checks) and the launch list of an update under the trace hook.  No GPU: nothing here launches a
kernel."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import _tqc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("curla_tqc_critic_loss", "curla_tqc_actor_loss")
F_, A_, H_ = 50, 2, 96


def make_agent(seed=1, hidden=H_, **kw):
    import curla_amd
    torch.manual_seed(seed)
    return curla_amd.CurlSacAgent((9, 32, 36), (A_,), torch.device("cpu"), None, hidden_dim=hidden, num_layers=2,
                                  num_filters=8, **kw)


def _inputs(B, M, seed=0, scale=1.5):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return dict(theta=scale * r(2, B, M), z=scale * r(2, B, M), log_pi=r(B), reward=r(B),
                not_done=(torch.arange(B) % 3 != 1).float(), log_alpha=torch.tensor(np.log(0.3)), discount=0.97)


# ------------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("M,d", [(1, 0), (2, 1), (5, 0), (5, 2), (7, 6)])
def test_reference_against_plain_loops(M, d):
    x = _inputs(4, M, seed=M + d)
    ref = R.critic_loss(d=d, **x)
    loss, dq = R.critic_loss_loops(d=d, **x)
    assert abs(float(ref["loss"]) - loss) <= 1e-12 * abs(loss)
    assert np.abs(ref["dq"].numpy() - dq).max() <= 1e-12 * np.abs(dq).max()
    assert abs(float(ref["row_loss"].mean()) - loss) <= 1e-12 * abs(loss)
    assert ref["y"].shape == (4, 2 * (M - d))


def test_truncation_by_value():
    """d > 0: the 2d largest pooled atoms are dropped whatever their values -- 1e6 or 0 in their places (0 makes them
    the smallest, so the 2d largest of the REST are dropped instead: drop those by hand to compare).  d = 0: they count."""
    B, M, d = 3, 5, 2
    x = _inputs(B, M, seed=5)
    pooled = x["z"].permute(1, 0, 2).reshape(B, 2 * M)
    top = pooled.argsort(dim=1)[:, -2 * d:]
    huge = pooled.clone().scatter_(1, top, 1e6)
    unpool = lambda p: p.reshape(B, 2, M).permute(1, 0, 2).contiguous()  # noqa: E731
    base = R.critic_loss(d=d, **x)
    big = R.critic_loss(d=d, **{**x, "z": unpool(huge)})
    assert float(big["loss"]) == float(base["loss"]) and torch.equal(big["dq"], base["dq"])
    # the kept atoms alone, as a d = 0 problem of K = 2 (M - d) atoms: same targets
    kept = pooled.sort(dim=1).values[:, :2 * (M - d)]
    assert torch.equal(base["y"], R.critic_loss(d=0, **{**x, "theta": x["theta"][:, :, :M - d],
                                                      "z": kept.reshape(B, 2, M - d).permute(1, 0, 2)})["y"])
    full = R.critic_loss(d=0, **x)
    big0 = R.critic_loss(d=0, **{**x, "z": unpool(huge)})
    assert float(big0["loss"]) > 1e3 * float(full["loss"]) and float(full["loss"]) != float(base["loss"])


def test_reference_is_continuous_at_its_seams():
    """u = 0 and |u| = 1 exactly, and ties among the pooled atoms: the loss and the gradient do not jump there."""
    M, d = 2, 0
    x = dict(log_pi=torch.zeros(1), reward=torch.zeros(1), not_done=torch.ones(1), log_alpha=torch.tensor(0.0), discount=1.0)
    z = torch.tensor([[[0.0, 1.0]], [[1.0, 2.0]]])      # pooled 0, 1, 1, 2 (a tie across the networks)
    theta = torch.tensor([[[0.0, 1.0]], [[2.0, 3.0]]])  # u in {0, +-1, +-2, ...}
    at = R.critic_loss(theta, z, d=d, **x)
    for eps in (1e-9, -1e-9):
        near = R.critic_loss(theta.double() + eps, z, d=d, **x)
        assert abs(float(near["loss"]) - float(at["loss"])) < 1e-8
        assert (near["dq"] - at["dq"]).abs().max() < 1e-8
    swapped = R.critic_loss(theta, z.flip(0), d=d, **x)  # the pooled multiset is the same
    assert float(swapped["loss"]) == float(at["loss"]) and torch.equal(swapped["dq"], at["dq"])


def test_actor_reference():
    B, M, A = 5, 3, 2
    x = _inputs(B, M, seed=2)
    log_std = torch.randn(B, A, generator=torch.Generator().manual_seed(3))
    ref = R.actor_loss(x["theta"], x["log_pi"], log_std, x["log_alpha"], -2.0)
    alpha = float(np.float32(np.exp(float(x["log_alpha"]))))
    want = np.mean([alpha * float(x["log_pi"][b]) - float(x["theta"][:, b].double().mean()) for b in range(B)])
    assert abs(float(ref["scalars"][0]) - want) < 1e-12
    assert torch.allclose(ref["dq"], torch.full((2, B, M), -1.0 / (2 * M * B), dtype=torch.float64), rtol=1e-14, atol=0)
    assert abs(float(ref["dlog_alpha"]) - alpha * float((-x["log_pi"].double() + 2.0).mean())) < 1e-12
    assert float(ref["scalars"][3]) == alpha


# ------------------------------------------------------------------------------------------------ keywords, validation
def test_keyword_positions_and_defaults():
    import curla_amd
    from curla_amd.curl_sac import Critic, QFunction
    init = list(inspect.signature(curla_amd.CurlSacAgent.__init__).parameters)
    assert init[-1] == "pixel_sac" and "critic_quantiles" not in init and "critic_drop_quantiles" not in init
    call = inspect.signature(curla_amd.CurlSacAgent).parameters
    names = list(call)
    for k in ("critic_quantiles", "critic_drop_quantiles"):
        assert call[k].default == 0 and call[k].kind is inspect.Parameter.KEYWORD_ONLY
        assert names.index(k) < names.index("weight_decay")
    assert names[-2] == "critic_layer_norm" and names[-3] == "critic_dropout"
    assert list(inspect.signature(Critic.__init__).parameters)[-1] == "layer_norm"
    assert list(inspect.signature(QFunction.__init__).parameters)[-1] == "dropout"
    for cls in (Critic, QFunction):  # the width: a keyword of the class call, as Critic's dropout is
        p = inspect.signature(cls).parameters["quantiles"]
        assert p.default == 0 and p.kind is inspect.Parameter.KEYWORD_ONLY
        assert "quantiles" not in inspect.signature(cls.__init__).parameters
    off = make_agent()
    assert off.critic_quantiles == 0 and off.critic_drop_quantiles == 0 and off.critic.quantiles == 0
    assert off.critic.out_dim == 1 and off.critic.Q1.quantiles == 0
    on = make_agent(critic_quantiles=np.int64(5), critic_drop_quantiles=2)
    assert type(on.critic_quantiles) is int and on.critic_quantiles == 5 and on.critic_drop_quantiles == 2
    assert on.critic.out_dim == on.critic_target.out_dim == 5 and on.critic.Q2.quantiles == 5


@pytest.mark.parametrize("bad", [-1, 33, 2.0, True, "5", None])
def test_quantiles_validation(bad):
    from curla_amd.curl_sac import Critic, QFunction
    with pytest.raises(ValueError, match="quantiles"):
        make_agent(critic_quantiles=bad)
    with pytest.raises(ValueError, match="quantiles"):
        Critic((9, 32, 36), (A_,), H_, F_, 2, 8, quantiles=bad)
    with pytest.raises(ValueError, match="quantiles"):
        QFunction(F_, A_, H_, quantiles=bad)


@pytest.mark.parametrize("M,bad", [(5, 5), (5, -1), (5, 1.0), (5, True), (5, "1"), (0, 1), (1, 1)])
def test_drop_quantiles_validation(M, bad):
    with pytest.raises(ValueError, match="critic_drop_quantiles"):
        make_agent(critic_quantiles=M, critic_drop_quantiles=bad)


def test_limits_build():
    assert make_agent(critic_quantiles=32, critic_drop_quantiles=31).critic.Q1.trunk[-1].out_features == 32
    assert make_agent(critic_quantiles=1).critic.Q1.trunk[-1].out_features == 1


def test_an_edited_drop_count_is_checked_by_update_critic():
    agent = make_agent(critic_quantiles=5, critic_drop_quantiles=1)
    agent.critic_drop_quantiles = 5
    x = torch.zeros(4, 9, 32, 36)
    with pytest.raises(ValueError, match="critic_drop_quantiles"):
        agent.update_critic(x, torch.zeros(4, A_), torch.zeros(4, 1), x, torch.ones(4, 1), None, 1)


# --------------------------------------------------------------------------------------------------------- state dicts
@pytest.mark.parametrize("ln", [False, True])
def test_state_dict_keys_are_unchanged_and_the_last_layers_have_m_rows(ln):
    M = 7
    off, on = make_agent(critic_layer_norm=ln), make_agent(critic_layer_norm=ln, critic_quantiles=M)
    last = "trunk.6." if ln else "trunk.4."
    for name in ("critic", "critic_target"):
        a, b = getattr(off, name).state_dict(), getattr(on, name).state_dict()
        assert list(a) == list(b)
        for k in a:
            if last in k:
                assert tuple(a[k].shape) == ((1, H_) if k.endswith("weight") else (1,))
                assert tuple(b[k].shape) == ((M, H_) if k.endswith("weight") else (M,))
            else:
                assert torch.equal(a[k], b[k]), (name, k)  # the same seed: the same other tensors
    for q in (on.critic.Q1, on.critic.Q2):  # initialised as every Linear is: orthogonal rows, zero bias
        w = q.trunk[-1].weight.detach().double()
        assert torch.allclose(w @ w.T, torch.eye(M, dtype=torch.float64), atol=1e-5) and not q.trunk[-1].bias.any()
    assert not torch.equal(on.critic.Q1.trunk[-1].weight, on.critic.Q2.trunk[-1].weight)
    for k, v in on.critic.state_dict().items():
        assert torch.equal(v, on.critic_target.state_dict()[k]), k
    assert all(not p.requires_grad for p in on.critic_target.parameters())
    a, b = off.actor.state_dict(), on.actor.state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert torch.equal(off.CURL.W, on.CURL.W) and torch.equal(off.log_alpha, on.log_alpha)
    # ... and the generator is left where an agent without the keyword leaves it
    torch.manual_seed(1)
    make_agent(critic_quantiles=M)
    after_on = torch.rand(3)
    torch.manual_seed(1)
    make_agent()
    assert torch.equal(after_on, torch.rand(3))


def test_another_width_does_not_load():
    five, seven = make_agent(critic_quantiles=5), make_agent(critic_quantiles=7)
    with pytest.raises(RuntimeError, match="size mismatch"):
        five.critic.load_state_dict(seven.critic.state_dict())
    with pytest.raises(RuntimeError, match="size mismatch"):
        make_agent().critic.load_state_dict(five.critic.state_dict())


def test_flat_layout_holds_the_wider_last_layers():
    off, on = make_agent(), make_agent(critic_quantiles=6)
    assert on._lay["qblock"] - off._lay["qblock"] == 5 * H_ + 8 - 4  # weights [6, H] for [1, H]; bias slots 8 for 4 floats
    for critic in (on.critic, on.critic_target):
        w1, w2 = critic.Q1.trunk[-1].weight, critic.Q2.trunk[-1].weight
        assert (w2.data_ptr() - w1.data_ptr()) // 4 == critic.twin_stride
    assert on.critic.Q1.trunk[-1].weight.grad.shape == (6, H_)


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
    assert callable(ops.tqc_critic_loss) and callable(ops.tqc_actor_loss) and ops.TQC_MAX == 32
    kernels = open(os.path.join(ROOT, "curla_amd", "csrc", "tqc.h")).read()
    assert "tqc_critic_loss_kernel" in kernels and "tqc_actor_loss_kernel" in kernels and "asm" not in kernels
    heads = open(os.path.join(ROOT, "curla_amd", "csrc", "heads.hip")).read()
    assert heads.index('#include "reduce.h"') < heads.index('#include "tqc.h"')


def test_entry_points_check_their_arguments_before_any_launch():
    """CURLA_ERR_ARG (-1) on a NULL required pointer, B < 1, M < 1, M > 32, d < 0, d >= M and twin strides below B M --
    all decided on the host, so a machine without a GPU sees them too (the pointers are never dereferenced)."""
    from curla_amd import _lib
    lib = _lib.load()
    p = 4096  # a non-NULL, aligned, never dereferenced address

    def critic(q=p, tq=p, lp=p, r=p, nd=p, la=p, dq=p, rl=p, B=4, M=5, d=2, sq=None, st=None, sd=None):
        dense = B * M
        return lib.curla_tqc_critic_loss(q, dense if sq is None else sq, tq, dense if st is None else st, lp, r, nd, la,
                                         0.99, B, M, d, dq, dense if sd is None else sd, rl, None, None)

    def actor(q=p, lp=p, ls=p, la=p, sc=p, dq=p, B=4, M=5, A=2, sq=None, sd=None):
        dense = B * M
        return lib.curla_tqc_actor_loss(q, dense if sq is None else sq, lp, ls, A, la, -2.0, B, M, sc, dq,
                                        dense if sd is None else sd, None, None)
    for bad in (dict(q=None), dict(tq=None), dict(lp=None), dict(r=None), dict(nd=None), dict(la=None), dict(dq=None),
                dict(rl=None), dict(B=0), dict(M=0), dict(M=33, d=0), dict(d=-1), dict(d=5), dict(M=1, d=1), dict(sq=19),
                dict(st=19), dict(sd=19)):
        assert critic(**bad) == -1, bad
    for bad in (dict(q=None), dict(lp=None), dict(ls=None), dict(la=None), dict(sc=None), dict(dq=None), dict(B=0),
                dict(M=0), dict(M=33), dict(A=0), dict(sq=19), dict(sd=19)):
        assert actor(**bad) == -1, bad


# --------------------------------------------------------------------------------------------------------- launch list
def _traced_update(step, **kw):
    """The launch list of one update() of a CPU agent under the trace hook (nothing is computed)."""
    import curla_amd
    from curla_amd import _lib
    aug = curla_amd.RandomCrop((34, 40), (28, 34))
    curla_amd.set_seed_everywhere(1)
    agent = curla_amd.CurlSacAgent((9, 28, 34), (2,), "cpu", aug, hidden_dim=64, log_interval=100, **kw)
    rb = curla_amd.ReplayBuffer((9, 34, 40), (2,), 32, 8, "cpu", aug)
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
@pytest.mark.parametrize("M,d", [(5, 2), (25, 3)])
def test_launch_list_contains_the_quantile_losses(step, M, d):
    """The critic phase launches the quantile loss in place of the fused loss-in-backward launch, the actor phase (even
    steps) its own; M <= 16 keeps the last layer's small forms, above that the GEMM forms take over.  With the keyword
    off neither launch appears."""
    _, off = _traced_update(step)
    agent, on = _traced_update(step, critic_quantiles=M, critic_drop_quantiles=d)
    names_off, names_on = [n for n, _ in off], [n for n, _ in on]
    assert not any(n in ENTRY_POINTS for n in names_off) and "curla_mlp_out_bwd_loss" in names_off
    even = step % 2 == 0
    assert names_on.count(ENTRY_POINTS[0]) == 1 and names_on.count(ENTRY_POINTS[1]) == (1 if even else 0)
    assert "curla_mlp_out_bwd_loss" not in names_on and "curla_critic_td_loss" not in names_on
    assert "curla_actor_loss" not in names_on
    B = 8
    ws = agent._ws(B)
    assert ws.q2.shape == (2, 2, B, M) and ws.dq.shape == (2, B, M) and ws.q_row_loss.shape == (B,)
    a = dict(on)[ENTRY_POINTS[0]]
    assert a[0] == ws.q.data_ptr() and a[2] == ws.tq.data_ptr() and a[1] == a[3] == a[13] == B * M
    assert a[9:12] == (B, M, d) and a[12] == ws.dq.data_ptr() and a[14] == ws.q_row_loss.data_ptr()
    assert a[15] == ws.scalars.data_ptr()  # scalars[0]: the logged train_critic/loss
    if even:
        a = dict(on)[ENTRY_POINTS[1]]
        assert a[0] == ws.q.data_ptr() and a[1] == a[11] == B * M and a[7:9] == (B, M) and a[10] == ws.dq.data_ptr()
        assert a[9] == ws.scalars.data_ptr() + 4
    # the loss launch sits in front of the last layer's backward
    i = names_on.index(ENTRY_POINTS[0])
    small = M <= 16
    assert names_on[i - 1] == ("curla_mlp_out_fwd_nested" if small else "curla_gemm_nested")  # (the four Q functions)
    assert names_on[i + 1] == ("curla_mlp_out_bwd" if small else "curla_gemm")
    assert ("curla_mlp_out_fwd_nested" in names_on) == small and "curla_colsum3" in names_on
    if even:
        j = names_on.index(ENTRY_POINTS[1])
        assert names_on[j - 1] == ("curla_mlp_out_fwd" if small else "curla_gemm")
        assert names_on[j + 1] == ("curla_mlp_out_bwd" if small else "curla_gemm")


def test_default_agent_has_no_quantile_buffers_and_the_old_graph_key():
    agent, _ = _traced_update(1)
    assert agent._ws(8).q_row_loss is None and agent._ws(8).q2.shape == (2, 2, 8, 1)
    key = agent._graph_key()
    assert not any(isinstance(k, tuple) and k and k[0] == "quantiles" for k in key)
    on, _ = _traced_update(1, critic_quantiles=5, critic_drop_quantiles=1)
    k1 = on._graph_key()
    assert k1[-1] == ("quantiles", 5, 1) and k1[:-1] == key
    on.critic_drop_quantiles = 2
    assert on._graph_key()[-1] == ("quantiles", 5, 2)
