"""Decoupled weight decay (AdamW) in the flat Adam launches, host side (no GPU): the launch schedule of a decaying
``FlatAdam`` seen through the launch trace (nothing computes), the validation of ``weight_decay``, the ``state_dict()``
format, the additive C ABI, ``CurlSacAgent(weight_decay=...)`` / ``set_weight_decay`` and the captured graphs'
fingerprint -- and the CPU identity the feature is specified by: ``torch.optim.AdamW`` is, bit for bit,
``param *= float32(1 - lr * weight_decay)`` followed by a plain ``torch.optim.Adam`` step."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests.test_grad_clip_host import _cpu_agent, _flat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADAMW_NAMES = ["curla_adamw_step", "curla_adamw_step_lerp", "curla_adamw_step_scalar64", "curla_adamw_step2"]
NO_CLIP = (0, 0, 0.0, 0)  # (partials, n_partials, max_norm, stats) of an unclipped curla_adamw_* launch


@pytest.fixture
def trace():
    from curla_amd import _lib
    calls = []
    _lib.set_trace_hook(lambda name, args: calls.append((name, args)))
    yield calls
    _lib.set_trace_hook(None)


class _Scalar:
    """What FlatAdam.step_with_scalar asks of log_alpha: a float64 one-element device parameter with a gradient (the
    trace computes nothing, so the addresses only have to exist)."""

    def __init__(self):
        self.t, self.grad = torch.zeros((), dtype=torch.float64), torch.zeros((), dtype=torch.float64)
        self.dtype, self.is_cuda = torch.float64, True

    def numel(self):
        return 1

    def data_ptr(self):
        return self.t.data_ptr()


def _four_forms(max_grad_norm=None, **decay):
    """The launches of step, step_pair, step_with_lerp and step_with_scalar over the layout of test_grad_clip_host, each
    on fresh optimizers: {form: [(name, args)]}, and the objects the argument tuples are checked against."""
    from curla_amd import _lib
    from curla_amd.optim import FlatAdam
    calls = []
    _lib.set_trace_hook(lambda name, args: calls.append((name, args)))
    out = {}
    try:
        flat, gflat, params, off = _flat()
        kw = dict(lr=3e-4, betas=(0.5, 0.999), max_grad_norm=max_grad_norm)
        opt = FlatAdam(params, flat, gflat, **kw, **decay)
        opt.step()
        out["step"], calls[:] = list(calls), []
        enc = FlatAdam(params[1:], flat, gflat, **kw, **decay)
        cpc = FlatAdam(params, flat, gflat, lr=1e-3, max_grad_norm=max_grad_norm, **decay)
        FlatAdam.step_pair(enc, cpc)
        out["step_pair"], calls[:] = list(calls), []
        lerp = FlatAdam(params, flat, gflat, **kw, **decay)
        target = torch.zeros_like(flat)
        assert FlatAdam.step_with_lerp(lerp, target, 0, off, 40, 0.05, 0.01)
        out["step_with_lerp"], calls[:] = list(calls), []
        first = FlatAdam(params, flat, gflat, **kw, **decay)
        a = torch.nn.Parameter(torch.zeros((), dtype=torch.float64))
        sopt = torch.optim.Adam([a], lr=1e-4, betas=(0.5, 0.999), foreach=False)
        fake = _Scalar()
        sopt.param_groups[0]["params"][0] = fake  # (a CPU parameter would send the step to the two separate ones)
        sopt.state[fake] = {"step": torch.tensor(0.0), "exp_avg": torch.zeros((), dtype=torch.float64),
                            "exp_avg_sq": torch.zeros((), dtype=torch.float64)}
        FlatAdam.step_with_scalar(first, sopt)
        out["step_with_scalar"], calls[:] = list(calls), []
    finally:
        _lib.set_trace_hook(None)
    keep = dict(flat=flat, gflat=gflat, off=off, opt=opt, enc=enc, cpc=cpc, lerp=lerp, first=first, target=target)
    return out, keep


PLAIN = {"step": "curla_adam_step", "step_pair": "curla_adam_step2", "step_with_lerp": "curla_adam_step_lerp",
         "step_with_scalar": "curla_adam_step_scalar64"}
ADAMW = {"step": "curla_adamw_step", "step_pair": "curla_adamw_step2", "step_with_lerp": "curla_adamw_step_lerp",
         "step_with_scalar": "curla_adamw_step_scalar64"}
# where weight_decay stands in a curla_adamw_* argument tuple (right behind each eps of the flat run), and where the four
# clip arguments begin
WD_AT = {"step": (9,), "step_pair": (12, 18), "step_with_lerp": (9,), "step_with_scalar": (9,)}
CLIP_AT = {"step": 12, "step_pair": 21, "step_with_lerp": 18, "step_with_scalar": 22}


def _without(args, positions):
    return tuple(a for i, a in enumerate(args) if i not in positions)


@pytest.mark.parametrize("max_grad_norm", [None, 2.5])
def test_zero_weight_decay_is_todays_launch_list_and_arguments(max_grad_norm):
    """weight_decay = 0 -- by default, spelled out, and with the decoupled flag on -- launches the plain family with the
    argument tuples it has always had (the literal tuples of the unclipped forms are written out here)."""
    base, k = _four_forms(max_grad_norm)
    suffix = "" if max_grad_norm is None else "_clip"
    for form, calls in base.items():
        names = [c[0] for c in calls]
        assert names == ([] if max_grad_norm is None else ["curla_grad_sqsum"]) + [PLAIN[form] + suffix], (form, names)
    if max_grad_norm is None:
        f, g, n = k["flat"].data_ptr(), k["gflat"].data_ptr(), k["off"] - 3
        opt, enc, cpc = k["opt"], k["enc"], k["cpc"]
        hyper = (3e-4, 0.5, 0.999, 1e-8, 1)
        assert base["step"][0][1] == (f, g, opt._m.data_ptr(), opt._v.data_ptr(), n) + hyper + (None, 0)
        e0 = enc._lo
        assert base["step_pair"][0][1] == (f, g, enc._m.data_ptr(), enc._v.data_ptr(), cpc._m.data_ptr(),
                                           cpc._v.data_ptr(), n, e0) + hyper + (1e-3, 0.9, 0.999, 1e-8, 1) + (None, 0)
        lerp = k["lerp"]
        assert base["step_with_lerp"][0][1] == (f, g, lerp._m.data_ptr(), lerp._v.data_ptr(), n) + hyper + \
            (None, k["target"].data_ptr(), 40, 0.05, 1.0 - 0.05, 0.01, 1.0 - 0.01, 0)
        sc = base["step_with_scalar"][0][1]
        first = k["first"]
        assert sc[:11] == (f, g, first._m.data_ptr(), first._v.data_ptr(), n) + hyper + (None,)
        assert sc[15:] == (1e-4, 0.5, 0.999, 1e-8, 1, None, 0) and len(sc) == 22
    for decay in (dict(weight_decay=0.0), dict(weight_decay=0, decoupled_weight_decay=True)):
        again, _ = _four_forms(max_grad_norm, **decay)
        for form in base:
            assert [c[0] for c in again[form]] == [c[0] for c in base[form]]
            assert [len(c[1]) for c in again[form]] == [len(c[1]) for c in base[form]]
            # (fresh buffers: the addresses differ, everything that is not an address is equal)
            small = lambda args: tuple(a for a in args if a is None or isinstance(a, float) or abs(a) < 4096)  # noqa: E731
            assert [small(c[1]) for c in again[form]] == [small(c[1]) for c in base[form]]


@pytest.mark.parametrize("max_grad_norm", [None, 2.5])
def test_decaying_forms_launch_their_adamw_namesake_once(max_grad_norm):
    """Each of the four forms: ONE curla_adamw_* launch (behind the square-sum when clipping), no fall-back to separate
    steps; weight_decay behind each eps of the flat run, the clip arguments (0, 0, 0.0, 0) when unclipped, and every
    other argument where the plain launch has it."""
    plain, _ = _four_forms(max_grad_norm)
    got, k = _four_forms(max_grad_norm, weight_decay=1e-2, decoupled_weight_decay=True)
    for form, calls in got.items():
        names = [c[0] for c in calls]
        assert names == ([] if max_grad_norm is None else ["curla_grad_sqsum"]) + [ADAMW[form]], (form, names)
        args, old = calls[-1][1], plain[form][-1][1]
        assert all(args[i] == 1e-2 and type(args[i]) is float for i in WD_AT[form]), (form, args)
        c = CLIP_AT[form]
        if max_grad_norm is None:
            assert args[c:c + 4] == NO_CLIP and len(args) == c + 5, (form, args)
            rest = _without(args, WD_AT[form] + tuple(range(c, c + 4)))
        else:
            assert args[c + 1:c + 3] == (1, 2.5) and args[c] != 0 and args[c + 3] != 0 and len(args) == c + 5
            assert calls[0][1][2] == args[c]  # the partials the square-sum launch wrote
            rest = _without(args, WD_AT[form])
        assert len(rest) == len(old)
        small = lambda a: tuple(x for x in a if x is None or isinstance(x, float) or abs(x) < 4096)  # noqa: E731
        assert small(rest) == small(old), form
    # step_pair: the two optimizers' own decays, 0 included, in the order (first, second)
    from curla_amd import _lib
    from curla_amd.optim import FlatAdam
    flat, gflat, params, off = _flat()
    enc = FlatAdam(params[1:], flat, gflat, weight_decay=0.0)
    cpc = FlatAdam(params, flat, gflat, lr=2e-3, weight_decay=0.25, decoupled_weight_decay=True)
    calls = []
    _lib.set_trace_hook(lambda name, args: calls.append((name, args)))
    try:
        FlatAdam.step_pair(enc, cpc)
    finally:
        _lib.set_trace_hook(None)
    assert [c[0] for c in calls] == ["curla_adamw_step2"]
    assert calls[0][1][8:20] == (1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 2e-3, 0.9, 0.999, 1e-8, 0.25, 1)


def test_every_run_and_piece_of_a_decaying_step_is_an_adamw_launch(trace):
    """step() over several runs (a parameter without a gradient; a parameter with a step count of its own) and
    step_pair's two separate steps, where the second steps over runs the first has clipped already: every launch is
    curla_adamw_step, clipped or not; the decay is read from the group at step time."""
    from curla_amd.optim import FlatAdam
    flat, gflat, params, off = _flat()
    opt = FlatAdam(params, flat, gflat, weight_decay=0.5, decoupled_weight_decay=True)
    g2 = params[2].grad
    params[2].grad = None
    opt.step()
    assert [(c[0], c[1][4], c[1][9]) for c in trace] == [("curla_adamw_step", 48, 0.5), ("curla_adamw_step", 65, 0.5)]
    assert all(c[1][12:16] == NO_CLIP for c in trace)
    trace.clear()
    params[2].grad = g2
    opt.param_groups[0]["weight_decay"] = 0.125  # edited as with torch: read at step time
    opt.step()
    assert [(c[0], c[1][4], c[1][9], c[1][10]) for c in trace] == \
        [("curla_adamw_step", 48, 0.125, 2), ("curla_adamw_step", 3, 0.125, 1), ("curla_adamw_step", 65, 0.125, 2)]
    trace.clear()
    opt.param_groups[0]["weight_decay"] = 0  # ... and switched off: the plain launches
    opt.step()
    assert [c[0] for c in trace] == ["curla_adam_step"] * 3
    trace.clear()
    enc = FlatAdam(params[1:], flat, gflat, max_grad_norm=3.0, weight_decay=0.5, decoupled_weight_decay=True)
    cpc = FlatAdam(params, flat, gflat, max_grad_norm=3.0, weight_decay=0.25, decoupled_weight_decay=True)
    enc._steps[0] += 1  # unequal step counts: the two separate steps, ONE norm
    FlatAdam.step_pair(enc, cpc)
    names = [c[0] for c in trace]
    assert names.count("curla_grad_sqsum") == 1 and set(names[1:]) == {"curla_adamw_step"} and len(names) == 6
    steps = [c[1] for c in trace[1:]]
    assert [a[9] for a in steps] == [0.5, 0.5, 0.25, 0.25, 0.25]
    clipped = [a[12] != 0 for a in steps]
    assert clipped == [True, True, True, False, False]  # cpc clips CURL.W only: the encoder's runs are scaled already
    assert all(a[12:16] == NO_CLIP for a, c in zip(steps, clipped) if not c)


def test_coupled_decay_and_other_options_stay_refused(trace):
    from curla_amd.optim import FlatAdam
    flat, gflat, params, off = _flat()
    with pytest.raises(NotImplementedError, match="decoupled"):
        FlatAdam(params, flat, gflat, weight_decay=1e-2)
    opt = FlatAdam(params, flat, gflat)
    opt.param_groups[0]["weight_decay"] = 1e-2  # coupled: the flag is off
    with pytest.raises(NotImplementedError, match="decoupled"):
        opt.step()
    assert opt._single_run() is None and trace == []
    opt.param_groups[0]["decoupled_weight_decay"] = True
    assert opt._single_run() is not None  # a decaying group keeps the fused launches
    opt.step()
    assert [c[0] for c in trace] == ["curla_adamw_step"]
    for option in ("amsgrad", "maximize"):
        bad = FlatAdam(params, flat, gflat, weight_decay=1e-2, decoupled_weight_decay=True)
        bad.param_groups[0][option] = True
        with pytest.raises(NotImplementedError):
            bad.step()


@pytest.mark.parametrize("bad", [True, False, -1e-3, float("nan"), float("inf"), -float("inf"), "0.01", [0.01], None])
def test_bad_weight_decays_are_refused(bad):
    from curla_amd.optim import FlatAdam
    flat, gflat, params, _ = _flat()
    with pytest.raises(ValueError):
        FlatAdam(params, flat, gflat, weight_decay=bad, decoupled_weight_decay=True)
    agent, _ = _cpu_agent()
    with pytest.raises(ValueError):
        agent.set_weight_decay(bad)
    assert agent.weight_decay == 0.0
    import curla_amd
    with pytest.raises(ValueError):
        curla_amd.CurlSacAgent((9, 28, 34), (2,), "cpu", curla_amd.RandomCrop((34, 40), (28, 34)), weight_decay=bad)


def test_the_two_arguments_are_keyword_only():
    from curla_amd.optim import FlatAdam
    flat, gflat, params, _ = _flat()
    with pytest.raises(TypeError):
        FlatAdam(params, flat, gflat, 1e-3, (0.9, 0.999), 1e-8, 1e-2)
    with pytest.raises(TypeError):
        FlatAdam(params, flat, gflat, 1e-3, (0.9, 0.999), 1e-8, 1e-2, True)
    sig = inspect.signature(FlatAdam.__init__).parameters
    assert sig["weight_decay"].kind is sig["decoupled_weight_decay"].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig["weight_decay"].default == 0.0 and sig["decoupled_weight_decay"].default is False


def test_state_dict_is_torchs_with_the_decay_in_the_group(trace):
    from curla_amd.optim import FlatAdam
    sizes = [(8, 5), (8,), (3,), (16, 4), (1,)]
    flat, gflat, params, _ = _flat(sizes)
    kw = dict(lr=3e-4, betas=(0.5, 0.999), eps=1e-7, weight_decay=1e-2, decoupled_weight_decay=True)
    opt = FlatAdam(params, flat, gflat, **kw)
    opt.step()
    ref = torch.optim.Adam([torch.nn.Parameter(torch.zeros(n)) for n in sizes], **kw)
    for p in ref.param_groups[0]["params"]:
        p.grad = torch.zeros_like(p)
    ref.step()
    sd, rsd = opt.state_dict(), ref.state_dict()
    assert sd["param_groups"][0] == rsd["param_groups"][0]  # the same keys and, for the same arguments, the same values
    assert sd["param_groups"][0]["weight_decay"] == 1e-2 and sd["param_groups"][0]["decoupled_weight_decay"] is True
    assert set(sd) == set(rsd) and set(sd["state"][0]) == set(rsd["state"][0])
    plain = FlatAdam(params, flat, gflat)
    assert plain.state_dict()["param_groups"][0] == \
        torch.optim.Adam([torch.nn.Parameter(torch.zeros(n)) for n in sizes]).state_dict()["param_groups"][0]
    plain.load_state_dict(sd)  # the round trip: the group's decay comes back, and the next step is the decaying one
    assert plain.state_dict()["param_groups"][0] == sd["param_groups"][0] and plain._steps == [1] * len(sizes)
    trace.clear()
    plain.step()
    assert [(c[0], c[1][9], c[1][10]) for c in trace] == [("curla_adamw_step", 1e-2, 2)]
    ref.load_state_dict(sd)  # ... and torch's own Adam takes FlatAdam's state_dict()
    assert ref.param_groups[0]["weight_decay"] == 1e-2 and ref.param_groups[0]["decoupled_weight_decay"] is True


def test_abi_is_additive():
    from curla_amd import _lib
    text = open(os.path.join(ROOT, "include", "curla_hip.h")).read()
    assert re.search(r"#define\s+CURLA_ABI_VERSION\s+8\b", text) and _lib.ABI_VERSION == 8
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(curla_[a-z0-9_]+)\s*\(", code))
    assert set(ADAMW_NAMES) <= declared and set(ADAMW_NAMES) <= set(_lib.SIGNATURES)
    assert set(_lib.SIGNATURES) == declared
    d = _lib.c_double
    for name, eps_at in (("step", (8,)), ("step_lerp", (8,)), ("step_scalar64", (8,)), ("step2", (11, 16))):
        old, new = list(_lib.SIGNATURES["curla_adam_" + name + "_clip"]), _lib.SIGNATURES["curla_adamw_" + name]
        assert all(old[i] is d for i in eps_at)
        for i in reversed(eps_at):  # a c_double right behind each eps of the flat run (the scalar's eps64 gets none)
            old.insert(i + 1, d)
        assert new == old, name
    # ... and the C declarations say the same: `double weight_decay` follows `double eps`, the gradient is not const
    for name in ADAMW_NAMES:
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", code).group(1)
        names = [a.split()[-1].lstrip("*") for a in decl.split(",")]
        types = [" ".join(a.split()[:-1]) for a in decl.split(",")]
        assert len(names) == len(_lib.SIGNATURES[name])
        for i, n in enumerate(names):
            if n in ("eps", "eps1", "eps2"):
                assert names[i + 1].startswith("weight_decay") and types[i + 1] == "double"
        assert names.count("eps64") <= 1 and (("eps64" not in names) or names[names.index("eps64") + 1] == "step64")
        assert types[names.index("grad")] == "float*"


def _groups(agent):
    return {n: getattr(agent, n + "_optimizer").param_groups for n in ("critic", "actor", "encoder", "cpc", "log_alpha")}


def test_agent_keyword_setter_and_graph_key():
    import curla_amd
    assert "weight_decay" not in inspect.signature(curla_amd.CurlSacAgent.__init__).parameters
    agent, rb = _cpu_agent()
    assert agent.weight_decay == 0.0
    with pytest.raises(AttributeError):
        agent.weight_decay = 1e-2  # read-only: set_weight_decay
    before = {n: [dict((k, v) for k, v in g.items() if k != "params") for g in gs] for n, gs in _groups(agent).items()}
    key0 = agent._graph_key()
    agent.critic_optimizer.param_groups[0]["lr"] = 5e-4
    assert agent._graph_key() == key0            # without decay lr travels as data: not in the key
    agent.set_weight_decay(1e-2)
    assert agent.weight_decay == 1e-2 and type(agent.weight_decay) is float
    key1 = agent._graph_key()
    assert key1 != key0
    agent.critic_optimizer.param_groups[0]["lr"] = 7e-4
    key2 = agent._graph_key()
    assert key2 != key1                          # a decaying optimizer's launch holds 1 - lr * wd by value
    agent.set_weight_decay(2e-2)
    key3 = agent._graph_key()
    assert key3 not in (key0, key1, key2)        # ... and the decay itself is in the key
    for n, gs in _groups(agent).items():
        for g in gs:
            if n == "log_alpha":                 # log_alpha's optimizer is its own: plain Adam
                assert g["weight_decay"] == 0 and g["decoupled_weight_decay"] is False
            else:
                assert g["weight_decay"] == 2e-2 and g["decoupled_weight_decay"] is True
    agent.set_weight_decay(0)
    assert agent._graph_key() == key0 and agent.weight_decay == 0.0
    agent.critic_optimizer.param_groups[0]["lr"] = 1e-3
    after = {n: [dict((k, v) for k, v in g.items() if k != "params") for g in gs] for n, gs in _groups(agent).items()}
    assert after == before                       # switched off: the groups are what the constructor left
    # the keyword of the class call: the same groups as the setter leaves, on an agent built like _cpu_agent's
    aug = curla_amd.RandomCrop((34, 40), (28, 34))
    curla_amd.set_seed_everywhere(1)
    kw_agent = curla_amd.CurlSacAgent((9, 28, 34), (2,), "cpu", aug, hidden_dim=64, log_interval=1, weight_decay=0.05)
    assert kw_agent.weight_decay == 0.05
    for n, gs in _groups(kw_agent).items():
        for g in gs:
            assert (g["weight_decay"], g["decoupled_weight_decay"]) == ((0, False) if n == "log_alpha" else (0.05, True))
    plain_key = agent._graph_key()
    assert kw_agent._graph_key() != plain_key
    kw_agent.set_weight_decay(0.0)
    assert kw_agent._graph_key() == plain_key
    kw_agent.set_weight_decay(0.05)
    # one update of the CPU agent runs (torch's own Adam honours the group's flag)
    from curla_amd import _lib

    class Log:
        def log(self, *a, **k):
            pass
    _lib.set_trace_hook(lambda n, a: None)
    try:
        kw_agent.update(rb, Log(), 0)
    finally:
        _lib.set_trace_hook(None)
    steps = [float(s["step"]) for s in kw_agent.critic_optimizer.state.values()]
    assert steps and set(steps) == {1.0}


def test_flat_optimizers_of_an_agent_take_the_decay_from_their_groups(trace):
    """The four flat optimizers of an agent, stood in for by FlatAdams put in place of a CPU agent's torch ones: the
    setter reaches their groups, and their next steps are the decaying launches."""
    from curla_amd.optim import FlatAdam
    agent, _ = _cpu_agent()
    for name, sizes in (("critic", [(4, 4)]), ("actor", [(5,)]), ("encoder", [(3,)]), ("cpc", [(2, 2), (3,)])):
        flat, gflat, params, _ = _flat(sizes)
        setattr(agent, name + "_optimizer", FlatAdam(params, flat, gflat))
    agent.set_weight_decay(0.03)
    for name in ("critic", "actor", "encoder", "cpc"):
        getattr(agent, name + "_optimizer").step()
    assert [(c[0], c[1][9]) for c in trace] == [("curla_adamw_step", 0.03)] * 4
    assert agent.weight_decay == 0.03


@pytest.mark.parametrize("wd,lr", [(1e-2, 1e-3), (1e-4, 3e-4), (0.1, 1e-3)])
@pytest.mark.parametrize("foreach", [False, True])
def test_adamw_is_one_float32_multiply_in_front_of_adam(wd, lr, foreach):
    """The specification of the kernels, pinned to the installed torch: over 6 steps, torch.optim.AdamW on the CPU
    equals BIT FOR BIT ``param *= float32(1 - lr * weight_decay)`` (the factor formed in double, rounded to float once)
    followed by a plain torch.optim.Adam step -- and so does torch.optim.Adam(decoupled_weight_decay=True)."""
    gen = torch.Generator().manual_seed(3)
    shapes = [(32, 9, 3, 3), (50, 1203), (1,), (7,)]
    init = [torch.randn(s, generator=gen) for s in shapes]
    a = [torch.nn.Parameter(t.clone()) for t in init]
    b = [torch.nn.Parameter(t.clone()) for t in init]
    c = [torch.nn.Parameter(t.clone()) for t in init]
    betas = (0.5, 0.999)
    adamw = torch.optim.AdamW(a, lr=lr, betas=betas, weight_decay=wd, foreach=foreach)
    adam = torch.optim.Adam(b, lr=lr, betas=betas, foreach=foreach)
    flagged = torch.optim.Adam(c, lr=lr, betas=betas, weight_decay=wd, decoupled_weight_decay=True, foreach=foreach)
    d = float(np.float32(1.0 - lr * wd))
    assert d != 1.0
    for step in range(6):
        for i, (pa, pb, pc) in enumerate(zip(a, b, c)):
            g = torch.randn(pa.shape, generator=gen) * 10.0 ** (i % 3 - 2)
            pa.grad, pb.grad, pc.grad = g.clone(), g.clone(), g.clone()
        adamw.step()
        flagged.step()
        with torch.no_grad():
            for pb in b:
                pb.mul_(d)
        adam.step()
        for pa, pb, pc in zip(a, b, c):
            assert torch.equal(pa, pb) and torch.equal(pa, pc), step
    for pa, pb in zip(a, b):
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(adamw.state[pa][k], adam.state[pb][k])
    assert not torch.equal(a[0], init[0])
