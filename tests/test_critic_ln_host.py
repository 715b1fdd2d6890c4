"""CurlSacAgent(critic_layer_norm=True) on the host: the state-dict contract (key numbering, initial values, what a
seed reproduces), the width limit, the launch list of an update under the trace hook, and the two C entry points of the
critics' LayerNorm (declared, bound, exported, argument checks).  No GPU: nothing here launches a kernel."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("curla_mlp_ln_relu_fwd", "curla_mlp_ln_bwd")
F_, A_, H_ = 50, 2, 96


def make_agent(seed=1, hidden=H_, **kw):
    import curla_amd
    torch.manual_seed(seed)
    return curla_amd.CurlSacAgent((9, 32, 36), (A_,), torch.device("cpu"), None, hidden_dim=hidden, num_layers=2,
                                  num_filters=8, **kw)


@pytest.fixture(scope="module")
def agents():
    return make_agent(), make_agent(critic_layer_norm=True)


def test_default_critic_keys_are_unchanged(agents):
    off, _ = agents
    for critic in (off.critic, off.critic_target):
        keys = [k for k in critic.state_dict() if k.startswith("Q")]
        assert keys == [f"Q{q}.trunk.{i}.{t}" for q in (1, 2) for i in (0, 2, 4) for t in ("weight", "bias")]
        assert not any(f".trunk.{i}." in k for k in keys for i in (1, 3, 6))  # (no LayerNorm numbering)
        assert all(sd_v.dim() == 2 for k, sd_v in critic.state_dict().items() if ".trunk.4.weight" in k)
        assert not critic.layer_norm
    assert off.critic_layer_norm is False


def test_keyword_comes_last_and_init_keeps_the_reference_parameter_list():
    """``critic_layer_norm`` is a keyword of the class call, behind everything the reference takes and off by default;
    ``__init__``'s own parameter list stays the reference's (the drop-in contract pins it name for name)."""
    import inspect

    import curla_amd
    from curla_amd.curl_sac import Critic
    init = list(inspect.signature(curla_amd.CurlSacAgent.__init__).parameters)
    assert init[-1] == "pixel_sac" and "critic_layer_norm" not in init
    call = inspect.signature(curla_amd.CurlSacAgent).parameters
    assert list(call)[-2] == "critic_layer_norm" and call["critic_layer_norm"].default is False
    assert call["critic_layer_norm"].kind is inspect.Parameter.KEYWORD_ONLY
    critic = inspect.signature(Critic.__init__).parameters
    assert list(critic)[-1] == "layer_norm" and critic["layer_norm"].default is False
    with pytest.raises(TypeError):
        make_agent(critic_layer_norms=True)  # (a misspelt keyword still reaches __init__ and is refused there)


def test_layer_norm_critic_keys_shapes_and_initial_values(agents):
    _, on = agents
    shapes = {0: (H_, F_ + A_), 1: (H_,), 3: (H_, H_), 4: (H_,), 6: (1, H_)}
    for critic in (on.critic, on.critic_target):
        sd = critic.state_dict()
        keys = [k for k in sd if k.startswith("Q")]
        assert keys == [f"Q{q}.trunk.{i}.{t}" for q in (1, 2) for i in (0, 1, 3, 4, 6) for t in ("weight", "bias")]
        for q in (1, 2):
            trunk = getattr(critic, f"Q{q}").trunk
            assert [type(m).__name__ for m in trunk] == ["Linear", "LayerNorm", "ReLU", "Linear", "LayerNorm", "ReLU",
                                                         "Linear"]
            for i, shape in shapes.items():
                assert tuple(sd[f"Q{q}.trunk.{i}.weight"].shape) == shape
                assert tuple(sd[f"Q{q}.trunk.{i}.bias"].shape) == shape[:1]
            for i in (1, 4):
                assert trunk[i].eps == 1e-5 and trunk[i].elementwise_affine
                assert torch.equal(sd[f"Q{q}.trunk.{i}.weight"], torch.ones(H_))
                assert torch.equal(sd[f"Q{q}.trunk.{i}.bias"], torch.zeros(H_))
    assert all(not p.requires_grad for p in on.critic_target.parameters())


def test_same_seed_gives_the_same_linears_encoders_actor_and_curl_w(agents):
    off, on = agents
    renumber = {0: 0, 2: 3, 4: 6}
    for name in ("critic", "critic_target"):
        a, b = getattr(off, name).state_dict(), getattr(on, name).state_dict()
        for k, v in a.items():
            m = re.match(r"(Q[12]\.trunk\.)(\d)(\..*)", k)
            kb = k if m is None else m.group(1) + str(renumber[int(m.group(2))]) + m.group(3)
            assert torch.equal(v, b[kb]), (name, k)
        assert len(b) == len(a) + 8
    a, b = off.actor.state_dict(), on.actor.state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert torch.equal(off.CURL.W, on.CURL.W)
    assert torch.equal(off.log_alpha, on.log_alpha)


def test_width_limit_is_checked_at_construction():
    import curla_amd
    with pytest.raises(ValueError, match="1024"):
        make_agent(hidden=1025, critic_layer_norm=True)
    with pytest.raises(ValueError, match="1024"):
        curla_amd.curl_sac.Critic((9, 32, 36), (A_,), 1025, F_, 2, 8, layer_norm=True)
    on = make_agent(hidden=1024, critic_layer_norm=True)
    assert on.critic.Q1.trunk[1].weight.shape == (1024,)
    assert make_agent(hidden=1025).hidden_dim == 1025  # (without the flag the MLP path's own limits apply)


def test_flag_mismatch_does_not_load_silently(agents):
    off, on = agents
    with pytest.raises(RuntimeError, match="Missing key") as e:
        off.critic.load_state_dict(on.critic.state_dict())
    assert "Unexpected key" in str(e.value)
    with pytest.raises(RuntimeError, match="Missing key") as e:
        on.critic.load_state_dict(off.critic.state_dict())
    assert "Unexpected key" in str(e.value)


def test_critic_log_histograms_the_three_linears(agents):
    class Log:
        params = []

        def log_histogram(self, *a, **k):
            pass

        def log_param(self, key, module, step):
            self.params.append((key, module))
    for agent in agents:
        Log.params = []
        agent.critic.log(Log(), 0)
        assert [k for k, _ in Log.params] == [f"train_critic/q{q}_fc{i}" for i in range(3) for q in (1, 2)]
        assert all(isinstance(m, torch.nn.Linear) for _, m in Log.params)
        assert Log.params[-1][1] is agent.critic.Q2.trunk[-1]


def _traced_update(flag, step):
    """The launch list of one update() of a CPU agent under the trace hook (nothing is computed)."""
    import numpy as np

    import curla_amd
    from curla_amd import _lib
    aug = curla_amd.RandomCrop((34, 40), (28, 34))
    curla_amd.set_seed_everywhere(1)
    agent = curla_amd.CurlSacAgent((9, 28, 34), (2,), "cpu", aug, hidden_dim=64, log_interval=100, critic_layer_norm=flag)
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
def test_launch_list_is_the_default_one_plus_the_layer_norm_launches(step):
    """An even update gains 2 four-Q forward launches and 2 backward calls with parameter gradients (critic phase), then
    2 twin forward launches and 2 backward calls for the data gradient alone (actor phase); an odd one the critic
    phase's.  Everything else is the flag-off list, except that the critic's three-way bias column sum shrinks to the
    last layer's (the hidden Linears' bias gradients now come out of the LayerNorm backward)."""
    _, off = _traced_update(False, step)
    agent, on = _traced_update(True, step)
    ln = ("curla_mlp_ln_relu_fwd", "curla_mlp_ln_bwd")
    assert not any(n in ln for n, _ in off)
    fwd = [a for n, a in on if n == ln[0]]
    bwd = [a for n, a in on if n == ln[1]]
    even = step % 2 == 0
    assert len(fwd) == len(bwd) == (4 if even else 2)
    B, H = 8, 64
    # critic phase: the target's and the critic's twins in ONE launch per hidden layer, saving from group 1 on
    for a in fwd[:2]:
        assert a[7] is not None and a[8] is not None and a[9:14] == (1, B, H, 2, 2) and a[2] == 2 * B * H
        assert a[6] == agent._twin_outer == agent._lay["total"] and a[5] == agent.critic.twin_stride
    # ... its backward leaves parameter gradients, the actor phase's does not (and saves for its own backward)
    assert all(a[9] is not None and a[10] is not None and a[11] is not None and a[12] is not None for a in bwd[:2])
    if even:
        assert all(a[7] is not None and a[9:14] == (0, B, H, 2, 1) for a in fwd[2:])
        assert all(a[9] is None and a[10] is None and a[11] is None and a[12] is None for a in bwd[2:])
    # the bias folds into the neighbouring launches are off
    for n, a in on:
        if n == "curla_mlp_out_bwd_loss":
            assert a[12] is None  # db_hidden
    rest = [n for n, _ in on if n not in ln]
    names_off = [n for n, _ in off]
    assert len(rest) == len(names_off)
    differ = [(a, b) for a, b in zip(rest, names_off) if a != b]
    assert differ in ([], [("curla_colsum", "curla_colsum3")]), differ


def test_entry_points_are_declared_bound_and_exported():
    import __graft_entry__ as ge
    ge.build()
    from curla_amd import _lib
    text = open(os.path.join(ROOT, "include", "curla_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int %s\(([^;]*)\);" % name, text, flags=re.S)
        assert m, f"include/curla_hip.h does not declare {name} behind a comment"
        comment = " ".join(m.group(1).replace("*", " ").split())
        assert "Additive: CURLA_ABI_VERSION stays 8" in comment and "curl_sac.py:129-139" in comment
        params = [p.strip() for p in m.group(2).split(",")]
        assert len(params) == len(_lib.SIGNATURES[name])
        for p, t in zip(params, _lib.SIGNATURES[name]):
            want = (_lib.vp if "*" in p else _lib.c_ll if p.startswith("long long") else _lib.c_float
                    if p.startswith("float") else _lib.c_int)
            assert t is want, (name, p)
        assert hasattr(lib, name)
    assert _lib.ABI_VERSION == 8 and _lib.load().curla_abi_version() == 8


def test_entry_points_check_their_arguments_before_any_launch():
    """CURLA_ERR_ARG (-1) on a NULL required pointer, B < 1, H < 1; CURLA_ERR_UNSUPPORTED (-3) on H > 1024 -- all
    decided on the host, so a machine without a GPU sees them too (the pointers are never dereferenced)."""
    from curla_amd import _lib
    lib = _lib.load()
    p = 4096  # a non-NULL, aligned, never dereferenced address
    fwd = lambda h=p, g=p, b=p, xh=None, rs=None, first=0, B=4, H=64, nb=2, n2=1: lib.curla_mlp_ln_relu_fwd(  # noqa: E731
        h, B * H, 0, g, b, H, 0, xh, rs, first, B, H, nb, n2, 1e-5, None)
    bwd = lambda dh=p, xh=p, rs=p, g=p, B=4, H=64, nb=2, part=None, dg=None, db=None, dbias=None: lib.curla_mlp_ln_bwd(  # noqa: E731
        dh, B * H, xh, rs, g, H, B, H, nb, part, dg, db, dbias, H, None)
    for bad in (dict(h=None), dict(g=None), dict(b=None), dict(B=0), dict(H=0), dict(nb=0), dict(n2=0),
                dict(xh=p), dict(rs=p), dict(xh=p, rs=p, first=1), dict(xh=p, rs=p, first=-1)):
        assert fwd(**bad) == -1, bad
    for bad in (dict(dh=None), dict(xh=None), dict(rs=None), dict(g=None), dict(B=0), dict(H=0), dict(nb=0),
                dict(part=p), dict(dg=p, db=p, dbias=p), dict(part=p, dg=p, db=p)):
        assert bwd(**bad) == -1, bad
    assert fwd(H=1025) == -3 and bwd(H=1025) == -3
    assert fwd(H=1025, h=None) == -1 and bwd(H=1025, dh=None) == -1  # (an argument error comes first)
