"""CurlSacAgent(critic_layer_norm=True, critic_dropout=p) on the host: the NumPy restatement of the masks' stream
(tests/_dropout_ref.py) against Random123's known answers, its keep fractions and the independence of its masks; the
keyword's validation; keys, flat layout and graph fingerprint against a LayerNorm agent's; the two C entry points
(declared, bound, exported, argument checks) and the launch list of an update under the trace hook.  No GPU: nothing
here launches a kernel."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import _dropout_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("curla_mlp_drop_ln_relu_fwd", "curla_mlp_drop_ln_bwd")
A_, H_ = 2, 96
SEED, COUNTER = 0x1234ABCD5678, 7


def make_agent(seed=1, hidden=H_, **kw):
    import curla_amd
    torch.manual_seed(seed)
    return curla_amd.CurlSacAgent((9, 32, 36), (A_,), torch.device("cpu"), None, hidden_dim=hidden, num_layers=2,
                                  num_filters=8, **kw)


# ------------------------------------------------------------------------------------------------------- the reference
def test_numpy_philox_reproduces_the_random123_vectors():
    zero = [np.zeros(1, np.uint64)] * 4
    assert [int(w[0]) for w in R.philox4x32_10(zero, (0, 0))] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    ones = [np.full(1, 0xFFFFFFFF, np.uint64)] * 4
    assert [int(w[0]) for w in R.philox4x32_10(ones, (0xFFFFFFFF, 0xFFFFFFFF))] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6,
                                                                                  0x6D5451FD]


def test_keep_fractions_of_the_reference():
    """96 cases; the dropped share of each within 4 binomial sigmas of p."""
    worst = 0.0
    for p in (0.01, 0.1, 0.5):
        for H in (64, 100, 513, 1024):
            for B in (3, 5):
                for tag in (1, 2, 3, 4):
                    m = R.keep_mask(SEED, COUNTER, tag, 2, B, H, p)
                    assert m.shape == (2, B, H) and m.dtype == np.bool_
                    n = m.size
                    sig = abs((1.0 - m.mean()) - p) / np.sqrt(p * (1 - p) / n)
                    worst = max(worst, sig)
                    assert sig <= 4.0, (p, H, B, tag, sig)
    print(f"worst dropped share: {worst:.2f} sigma")


def test_masks_that_differ_in_one_coordinate_are_independent():
    p, H, B = 0.5, 1024, 5
    base = R.keep_mask(SEED, COUNTER, 1, 2, B, H, p)
    others = {"tag": R.keep_mask(SEED, COUNTER, 2, 2, B, H, p)[0], "counter": R.keep_mask(SEED, COUNTER + 1, 1, 2, B, H, p)[0],
              "seed": R.keep_mask(SEED + 1, COUNTER, 1, 2, B, H, p)[0], "twin": base[1]}
    n = B * H
    for what, m in others.items():
        agree = float((m == base[0]).mean())
        print(f"agreement with a mask of another {what}: {agree:.4f}")
        assert abs(agree - 0.5) <= 4 * 0.5 / np.sqrt(n), (what, agree)


# ------------------------------------------------------------------------------------------------- keyword, validation
def test_keyword_sits_next_to_critic_layer_norm_and_defaults_to_zero():
    import curla_amd
    from curla_amd.curl_sac import Critic, QFunction
    init = list(inspect.signature(curla_amd.CurlSacAgent.__init__).parameters)
    assert init[-1] == "pixel_sac" and "critic_dropout" not in init
    call = inspect.signature(curla_amd.CurlSacAgent).parameters
    assert call["critic_dropout"].default == 0.0 and call["critic_dropout"].kind is inspect.Parameter.KEYWORD_ONLY
    assert abs(list(call).index("critic_dropout") - list(call).index("critic_layer_norm")) == 1
    params = inspect.signature(QFunction.__init__).parameters
    assert list(params)[-1] == "dropout" and params["dropout"].default == 0.0
    # Critic takes it as a keyword of the class call, like the agent: its __init__ keeps layer_norm last
    params = inspect.signature(Critic).parameters
    assert params["dropout"].default == 0.0 and params["dropout"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(Critic.__init__).parameters)[-1] == "layer_norm"
    off = make_agent()
    assert off.critic_dropout == 0.0 and off.critic.dropout == 0.0 and off.critic.Q1.dropout == 0.0
    on = make_agent(critic_layer_norm=True, critic_dropout=0.01)
    assert on.critic_dropout == on.critic.dropout == on.critic_target.dropout == on.critic.Q2.dropout == 0.01


def test_validation():
    from curla_amd.curl_sac import Critic, QFunction
    for p in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"\[0, 1\)"):
            make_agent(critic_layer_norm=True, critic_dropout=p)
        with pytest.raises(ValueError, match=r"\[0, 1\)"):
            Critic((9, 32, 36), (A_,), H_, 50, 2, 8, True, dropout=p)
        with pytest.raises(ValueError, match=r"\[0, 1\)"):
            QFunction(50, A_, H_, True, p)
    with pytest.raises(ValueError, match="LayerNorm"):
        make_agent(critic_dropout=0.01)
    with pytest.raises(ValueError, match="LayerNorm"):
        Critic((9, 32, 36), (A_,), H_, 50, 2, 8, dropout=0.01)
    with pytest.raises(ValueError, match="LayerNorm"):
        QFunction(50, A_, H_, dropout=0.01)
    with pytest.raises(ValueError, match="1024"):
        make_agent(hidden=1025, critic_layer_norm=True, critic_dropout=0.01)
    assert make_agent(hidden=1024, critic_layer_norm=True, critic_dropout=0.01).critic.hidden_dim == 1024
    assert make_agent(critic_dropout=0.0).critic_dropout == 0.0  # (p = 0 needs no LayerNorm: it is today's critic)


# ------------------------------------------------------------------------------------------------------------ structure
def test_keys_layout_and_graph_key_are_a_layer_norm_agents():
    ln, drop = make_agent(critic_layer_norm=True), make_agent(critic_layer_norm=True, critic_dropout=0.1)
    for name in ("critic", "critic_target", "actor", "CURL"):
        a, b = getattr(ln, name).state_dict(), getattr(drop, name).state_dict()
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a), name  # (dropout draws nothing at init)
    assert [type(m).__name__ for m in drop.critic.Q1.trunk] == [type(m).__name__ for m in ln.critic.Q1.trunk]
    assert not any(isinstance(m, torch.nn.Dropout) for m in drop.critic.modules())
    assert ln._lay == drop._lay and ln.critic.twin_stride == drop.critic.twin_stride
    assert ln._critic_flat.numel() == drop._critic_flat.numel()
    # state dicts are interchangeable, both ways, and p stays the module's own
    with torch.no_grad():
        drop.critic.Q1.trunk[1].weight.add_(0.5)
    ln.critic.load_state_dict(drop.critic.state_dict())
    assert torch.equal(ln.critic.Q1.trunk[1].weight, drop.critic.Q1.trunk[1].weight) and ln.critic.dropout == 0.0
    drop.critic_target.load_state_dict(ln.critic_target.state_dict())
    assert drop.critic_target.dropout == 0.1
    # the graph fingerprint: p = 0 is an agent without the keyword, p > 0 enters it
    plain, zero = make_agent(), make_agent(critic_dropout=0.0)
    assert zero._graph_key() == plain._graph_key()
    assert make_agent(critic_layer_norm=True, critic_dropout=0.0)._graph_key() == ln._graph_key()
    assert len(ln._graph_key()) == len(plain._graph_key())
    assert drop._graph_key() != ln._graph_key() and 0.1 in drop._graph_key()
    drop.critic_dropout = 0.2
    assert 0.2 in drop._graph_key() and 0.1 not in drop._graph_key()


def test_checkpoint_records_p_and_a_mismatch_warns(tmp_path):
    ln, drop = make_agent(critic_layer_norm=True), make_agent(critic_layer_norm=True, critic_dropout=0.1)
    f_ln, f_drop = str(tmp_path / "ln.pt"), str(tmp_path / "drop.pt")
    ln.save_checkpoint(f_ln, 3)
    drop.save_checkpoint(f_drop, 4)
    assert torch.load(f_drop, weights_only=False)["critic_dropout"] == 0.1
    assert torch.load(f_ln, weights_only=False)["critic_dropout"] == 0.0
    with pytest.warns(RuntimeWarning, match="critic_dropout"):
        assert drop.load_checkpoint(f_ln) == 3  # a LayerNorm file loads into a dropout agent ...
    assert drop.critic_dropout == 0.1           # ... which keeps its own p
    with pytest.warns(RuntimeWarning, match="critic_dropout"):
        assert ln.load_checkpoint(f_drop) == 4
    assert ln.critic_dropout == 0.0


# --------------------------------------------------------------------------------------------------------- entry points
def test_entry_points_are_declared_bound_and_exported():
    import __graft_entry__ as ge
    ge.build()
    from curla_amd import _lib
    text = open(os.path.join(ROOT, "include", "curla_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, base in zip(ENTRY_POINTS, ("curla_mlp_ln_relu_fwd", "curla_mlp_ln_bwd")):
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int %s\(([^;]*)\);" % name, text, flags=re.S)
        assert m, f"include/curla_hip.h does not declare {name} behind a comment"
        comment = " ".join(m.group(1).replace("*", " ").split())
        assert "Additive: CURLA_ABI_VERSION stays 8" in comment and "curl_sac.py:129-139" in comment
        params = [p.strip() for p in m.group(2).split(",")]
        sig = _lib.SIGNATURES[name]
        assert len(params) == len(sig)
        for p, t in zip(params, sig):
            want = (_lib.vp if "*" in p else _lib.c_u64 if p.startswith("unsigned long long") else _lib.c_ll
                    if p.startswith("long long") else _lib.c_float if p.startswith("float") else _lib.c_int)
            assert t is want, (name, p)
        # the LayerNorm counterpart's arguments, then p, seed, counter, rng_dev, tag, then the stream
        assert sig[:-6] == _lib.SIGNATURES[base][:-1]
        assert sig[-6:] == [_lib.c_float, _lib.c_u64, _lib.c_u64, _lib.vp, _lib.c_int, _lib.vp]
        assert [p.split()[-1].lstrip("*") for p in params[-6:]] == ["p", "seed", "counter", "rng_dev", "tag", "stream"]
        assert hasattr(lib, name)
    assert _lib.ABI_VERSION == 8 and _lib.load().curla_abi_version() == 8


def test_entry_points_check_their_arguments_before_any_launch():
    """CURLA_ERR_ARG (-1) / CURLA_ERR_UNSUPPORTED (-3), decided on the host: the pointers are never dereferenced."""
    from curla_amd import _lib
    lib = _lib.load()
    P = 4096  # a non-NULL, aligned, never dereferenced address

    def fwd(h=P, g=P, b=P, xh=None, rs=None, first=0, B=4, H=64, nb=2, n2=1, p=0.1, dev=None, tag=1):
        return lib.curla_mlp_drop_ln_relu_fwd(h, B * H, 0, g, b, H, 0, xh, rs, first, B, H, nb, n2, 1e-5, p, SEED, COUNTER,
                                              dev, tag, None)

    def bwd(dh=P, xh=P, rs=P, g=P, B=4, H=64, nb=2, part=None, dg=None, db=None, dbias=None, p=0.1, dev=None, tag=1):
        return lib.curla_mlp_drop_ln_bwd(dh, B * H, xh, rs, g, H, B, H, nb, part, dg, db, dbias, H, p, SEED, COUNTER, dev,
                                         tag, None)
    drop_bad = (dict(p=-0.01), dict(p=1.0), dict(p=float("nan")), dict(tag=0), dict(tag=256), dict(tag=-1), dict(dev=P + 4))
    for bad in (dict(h=None), dict(g=None), dict(b=None), dict(B=0), dict(H=0), dict(nb=0), dict(n2=0),
                dict(xh=P), dict(rs=P), dict(xh=P, rs=P, first=1), dict(xh=P, rs=P, first=-1),
                dict(tag=254, n2=2), dict(tag=2, n2=128)) + drop_bad:
        assert fwd(**bad) == -1, bad
    for bad in (dict(dh=None), dict(xh=None), dict(rs=None), dict(g=None), dict(B=0), dict(H=0), dict(nb=0),
                dict(part=P), dict(dg=P, db=P, dbias=P), dict(part=P, dg=P, db=P)) + drop_bad:
        assert bwd(**bad) == -1, bad
    assert fwd(H=1025) == -3 and bwd(H=1025) == -3
    assert fwd(H=1025, tag=255, n2=1) == -3 and fwd(H=1025, tag=253, n2=2) == -3 and fwd(H=1025, p=0.0, dev=P + 8) == -3
    for bad in (dict(h=None), dict(p=1.0), dict(tag=0), dict(dev=P + 2), dict(tag=254, n2=2)):
        assert fwd(H=1025, **bad) == -1, bad  # (an argument error comes first)
    for bad in (dict(dh=None), dict(p=-1.0), dict(tag=256), dict(dev=P + 1)):
        assert bwd(H=1025, **bad) == -1, bad


# --------------------------------------------------------------------------------------------------------- launch lists
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


def _shape(args):
    """A traced call's arguments with the addresses reduced to given / NULL (two agents' buffers differ)."""
    return tuple(a if a is None or isinstance(a, float) or abs(a) < 2 ** 20 else "ptr" for a in args)


@pytest.mark.parametrize("step", [2, 1])
def test_launch_lists(step):
    _, ln = _traced_update(step, critic_layer_norm=True)
    _, zero = _traced_update(step, critic_layer_norm=True, critic_dropout=0.0)
    assert [(n, _shape(a)) for n, a in zero] == [(n, _shape(a)) for n, a in ln]  # p = 0: exactly the LayerNorm agent's
    agent, on = _traced_update(step, critic_layer_norm=True, critic_dropout=0.01)
    twin = {"curla_mlp_ln_relu_fwd": ENTRY_POINTS[0], "curla_mlp_ln_bwd": ENTRY_POINTS[1]}
    assert len(on) == len(ln)
    assert not any(n in twin for n, _ in on)
    fwd_tags, bwd_tags = [], []
    for (n0, a0), (n1, a1) in zip(ln, on):
        if n0 not in twin:
            assert n1 == n0 and _shape(a1) == _shape(a0), (n0, n1)  # nothing else differs
            continue
        assert n1 == twin[n0]
        assert _shape(a1[:len(a0) - 1]) == _shape(a0[:-1]) and len(a1) == len(a0) + 5
        p, seed, counter, dev, tag, stream = a1[-6:]
        assert p == 0.01 and dev is None and stream == a0[-1]
        assert (seed, counter) == (torch.initial_seed(), 0)  # (a CPU agent's stream position: it launches nothing)
        (fwd_tags if n1 == ENTRY_POINTS[0] else bwd_tags).append(tag)
    even = step % 2 == 0
    # the four-Q call (groups under tag, tag + 2), the critic's backward (layer 1 first), then the actor phase's pair
    assert fwd_tags == ([1, 2, 5, 6] if even else [1, 2])
    assert bwd_tags == ([4, 3, 6, 5] if even else [4, 3])
