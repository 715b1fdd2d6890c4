"""Clipping by the global gradient norm, host side (no GPU): the launch schedule of a clipped ``FlatAdam`` step seen
through the launch trace (nothing computes), the validation of ``max_grad_norm``, the unchanged ``state_dict()`` format,
the additive C ABI, and the captured graphs' fingerprint."""
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(8, 5), (8,), (3,), (16, 4), (1,)]  # the layout of test_host_logic.test_flat_adam_plan_and_state_format
CLIP_NAMES = ["curla_grad_sqsum", "curla_adam_step_clip", "curla_adam_step_lerp_clip", "curla_adam_step_scalar64_clip",
              "curla_adam_step2_clip"]


def _flat(sizes=SIZES):
    offs, off = [], 0
    for n in sizes:
        offs.append(off)
        off += (int(np.prod(n)) + 3) & ~3
    flat, gflat = torch.zeros(off), torch.zeros(off)
    params = []
    for n, o in zip(sizes, offs):
        p = torch.nn.Parameter(flat[o:o + int(np.prod(n))].view(n))
        p.grad = gflat[o:o + int(np.prod(n))].view(n)
        params.append(p)
    return flat, gflat, params, off


@pytest.fixture
def trace():
    from curla_amd import _lib
    calls = []
    _lib.set_trace_hook(lambda name, args: calls.append((name, args)))
    yield calls
    _lib.set_trace_hook(None)


def test_unset_is_todays_launch_list(trace):
    from curla_amd.optim import FlatAdam
    flat, gflat, params, off = _flat()
    opt = FlatAdam(params, flat, gflat, lr=3e-4, betas=(0.5, 0.999))
    assert opt.max_grad_norm is None
    opt.step()
    assert [c[0] for c in trace] == ["curla_adam_step"]
    trace.clear()
    opt.max_grad_norm = 1.0
    opt.max_grad_norm = None  # switched off again: the same list
    opt.step()
    assert [c[0] for c in trace] == ["curla_adam_step"]


def test_clipped_step_is_one_sqsum_per_run_then_the_clipped_steps(trace):
    from curla_amd.optim import FlatAdam
    flat, gflat, params, off = _flat()
    opt = FlatAdam(params, flat, gflat, lr=3e-4, betas=(0.5, 0.999), max_grad_norm=2.5)
    gbase, pbase = gflat.data_ptr(), opt._clip_partials.data_ptr()
    assert opt._clip_partials.dtype == torch.float64 and opt._clip_partials.numel() == 256
    opt.step()
    assert [c[0] for c in trace] == ["curla_grad_sqsum", "curla_adam_step_clip"]
    sq, st = trace[0][1], trace[1][1]
    assert sq[:4] == (gbase, off - 3, pbase, 1)          # one run over everything, one block (n <= 1024)
    assert st[4] == off - 3 and st[9] == 1               # ... stepped as the unclipped launch would
    assert st[11:15] == (pbase, 1, 2.5, opt.clip_stats.data_ptr())
    trace.clear()
    g2 = params[2].grad
    params[2].grad = None  # a hole in the middle: two runs, ONE norm over both
    opt.step()
    assert [c[0] for c in trace] == ["curla_grad_sqsum"] * 2 + ["curla_adam_step_clip"] * 2
    assert [c[1][1] for c in trace[:2]] == [48, 65] and [c[1][4] for c in trace[2:]] == [48, 65]
    assert [c[1][2] for c in trace[:2]] == [pbase, pbase + 8]
    assert all(c[1][11:13] == (pbase, 2) for c in trace[2:])
    trace.clear()
    params[2].grad = g2    # back with a step count of its own: three runs (the existing host test's layout)
    opt.step()
    assert [c[0] for c in trace] == ["curla_grad_sqsum"] * 3 + ["curla_adam_step_clip"] * 3
    sq, st = [c[1] for c in trace[:3]], [c[1] for c in trace[3:]]
    assert [(a[0] - gbase) // 4 for a in sq] == [0, 48, 52] and [a[1] for a in sq] == [48, 3, 65]
    # one partials buffer, disjoint slots: each run's slot starts where the previous one's ends
    slots = [((a[2] - pbase) // 8, a[3]) for a in sq]
    assert slots[0][0] == 0 and all(slots[i + 1][0] == slots[i][0] + slots[i][1] for i in range(2))
    total = sum(n for _, n in slots)
    assert 3 <= total <= 256
    assert [(a[4], a[9]) for a in st] == [(48, 3), (3, 2), (65, 3)]
    assert all(a[11:15] == (pbase, total, 2.5, opt.clip_stats.data_ptr()) for a in st)  # every step: the total count


def test_partial_counts_stay_within_one_adam_block(trace):
    """The block count is a function of the run's length alone, capped at 256 over all runs of a step."""
    from curla_amd.optim import FlatAdam
    flat, gflat, params, _ = _flat([(300001,), (5,), (1027,)])
    opt = FlatAdam(params, flat, gflat, max_grad_norm=1.0)
    opt.step()
    assert [c[1][3] for c in trace if c[0] == "curla_grad_sqsum"] == [256]  # one run (padding bridged), capped
    trace.clear()
    params[1].grad = None
    opt.step()
    assert [c[1][3] for c in trace if c[0] == "curla_grad_sqsum"] == [128, 2]  # two runs: 256 // 2 each at the most
    assert all(c[1][12] == 130 for c in trace if c[0] == "curla_adam_step_clip")


def test_fused_steps_take_the_norm_over_their_run(trace):
    from curla_amd.optim import FlatAdam
    flat, gflat, params, off = _flat()
    enc = FlatAdam(params[1:], flat, gflat, max_grad_norm=3.0)
    cpc = FlatAdam(params, flat, gflat, max_grad_norm=3.0)
    FlatAdam.step_pair(enc, cpc)
    assert [c[0] for c in trace] == ["curla_grad_sqsum", "curla_adam_step2_clip"]
    assert trace[0][1][:2] == (gflat.data_ptr(), off - 3)  # the norm is the SECOND optimizer's run's, [W | encoder]
    assert trace[0][1][2] == cpc._clip_partials.data_ptr() and trace[1][1][19:23] == \
        (cpc._clip_partials.data_ptr(), 1, 3.0, cpc.clip_stats.data_ptr())
    trace.clear()
    enc.max_grad_norm = 4.0   # a mismatch: the two separate steps, each with its own norm
    FlatAdam.step_pair(enc, cpc)
    assert [c[0] for c in trace] == ["curla_grad_sqsum", "curla_adam_step_clip"] * 2
    trace.clear()
    enc.max_grad_norm = 3.0
    enc._steps[0] += 1        # unequal step counts: the separate steps, but ONE norm and no element scaled twice
    FlatAdam.step_pair(enc, cpc)
    names = [c[0] for c in trace]
    assert names.count("curla_grad_sqsum") == 1 and trace[0][1][1] == off - 3
    e0 = (params[1].data_ptr() - flat.data_ptr()) // 4
    clipped = [((c[1][0] - flat.data_ptr()) // 4, c[1][4]) for c in trace if c[0] == "curla_adam_step_clip"]
    plain = [((c[1][0] - flat.data_ptr()) // 4, c[1][4]) for c in trace if c[0] == "curla_adam_step"]
    # encoder_optimizer clips its two runs (the odd step count splits them); cpc_optimizer clips only CURL.W in front
    # and steps over the encoder's runs with the unclipped launch: the gradient there is clipped already
    assert clipped == [(e0, 8), (e0 + 8, off - 3 - e0 - 8), (0, e0)]
    assert sorted(plain) == [(e0, 8), (e0 + 8, off - 3 - e0 - 8)]
    trace.clear()
    opt = FlatAdam(params, flat, gflat, max_grad_norm=3.0)
    target = torch.zeros_like(flat)
    assert FlatAdam.step_with_lerp(opt, target, 0, off, 40, 0.05, 0.01)
    assert [c[0] for c in trace] == ["curla_grad_sqsum", "curla_adam_step_lerp_clip"]
    assert trace[1][1][17:21] == (opt._clip_partials.data_ptr(), 1, 3.0, opt.clip_stats.data_ptr())


@pytest.mark.parametrize("bad", [True, False, 0, 0.0, -1.0, float("nan"), "1.0", [1.0], -float("inf")])
def test_bad_thresholds_are_refused(bad):
    from curla_amd.optim import FlatAdam
    flat, gflat, params, _ = _flat()
    with pytest.raises(ValueError):
        FlatAdam(params, flat, gflat, max_grad_norm=bad)
    opt = FlatAdam(params, flat, gflat, max_grad_norm=1.0)
    with pytest.raises(ValueError):
        opt.max_grad_norm = bad
    assert opt.max_grad_norm == 1.0


@pytest.mark.parametrize("good", [None, 1, 0.5, np.float32(2.0), float("inf")])
def test_good_thresholds(good):
    from curla_amd.optim import FlatAdam
    flat, gflat, params, _ = _flat()
    opt = FlatAdam(params, flat, gflat, max_grad_norm=good)
    assert opt.max_grad_norm == good and (good is None or type(opt.max_grad_norm) is float)
    with pytest.raises(TypeError):
        FlatAdam(params, flat, gflat, 1e-3, (0.9, 0.999), 1e-8, 1.0)  # keyword-only


def test_state_dict_keeps_torchs_format_with_clipping_on(trace):
    from curla_amd.optim import FlatAdam
    flat, gflat, params, _ = _flat()
    opt = FlatAdam(params, flat, gflat, lr=3e-4, betas=(0.5, 0.999), max_grad_norm=1.0)
    opt.step()
    ref = torch.optim.Adam([torch.nn.Parameter(torch.zeros(n)) for n in SIZES], lr=3e-4, betas=(0.5, 0.999))
    for p in ref.param_groups[0]["params"]:
        p.grad = torch.zeros_like(p)
    ref.step()
    sd, rsd = opt.state_dict(), ref.state_dict()
    assert sd["param_groups"][0].keys() == rsd["param_groups"][0].keys()
    assert "max_grad_norm" not in opt.param_groups[0]
    assert set(sd) == set(rsd) and set(sd["state"][0]) == set(rsd["state"][0])


def test_abi_is_additive():
    from curla_amd import _lib
    text = open(os.path.join(ROOT, "include", "curla_hip.h")).read()
    assert re.search(r"#define\s+CURLA_ABI_VERSION\s+8\b", text) and _lib.ABI_VERSION == 8
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(curla_[a-z0-9_]+)\s*\(", code))
    assert set(CLIP_NAMES) <= declared
    assert set(_lib.SIGNATURES) == declared
    for name in ("curla_adam_step", "curla_adam_step_lerp", "curla_adam_step_scalar64", "curla_adam_step2"):
        # a clipped entry point is its namesake plus (partials, n_partials, max_norm, stats) in front of the stream
        old, new = _lib.SIGNATURES[name], _lib.SIGNATURES[name + "_clip"]
        assert new == old[:-1] + [_lib.vp, _lib.c_int, _lib.c_double, _lib.vp] + old[-1:]


def _cpu_agent():
    import curla_amd
    aug = curla_amd.RandomCrop((34, 40), (28, 34))
    curla_amd.set_seed_everywhere(1)
    agent = curla_amd.CurlSacAgent((9, 28, 34), (2,), "cpu", aug, hidden_dim=64, log_interval=1)
    rb = curla_amd.ReplayBuffer((9, 34, 40), (2,), 32, 8, "cpu", aug)
    for _ in range(12):
        rb.add(np.zeros((9, 34, 40), np.uint8), [0, 0], 0.0, np.zeros((9, 34, 40), np.uint8), False)
    return agent, rb


def test_agent_setter_and_graph_key():
    """The setter validates, allocates the stats, and the value is part of what a captured graph is fingerprinted by."""
    agent, _ = _cpu_agent()
    assert agent.max_grad_norm is None and agent.grad_clip_stats is None
    with pytest.raises(AttributeError):
        agent.max_grad_norm = 1.0  # read-only: set_max_grad_norm
    keys = [agent._graph_key()]
    for m in (10.0, 5.0, float("inf"), None):
        agent.set_max_grad_norm(m)
        assert agent.max_grad_norm == m
        keys.append(agent._graph_key())
    assert len(set(keys[:4])) == 4 and keys[4] == keys[0]
    assert agent.grad_clip_stats.shape == (3, 2) and agent.grad_clip_stats.dtype == torch.float32
    for bad in (True, 0, -2.0, float("nan"), "3"):
        with pytest.raises(ValueError):
            agent.set_max_grad_norm(bad)
    assert agent.max_grad_norm is None
    import inspect
    import curla_amd
    assert "max_grad_norm" not in inspect.signature(curla_amd.CurlSacAgent.__init__).parameters


def test_flat_optimizers_share_the_agents_value_and_stats_rows():
    """The four flat optimizers of an agent, stood in for by FlatAdams put in place of a CPU agent's torch ones: the
    setter hands each the value and its row of grad_clip_stats (encoder and cpc share the CURL phase's)."""
    from curla_amd.optim import FlatAdam
    agent, _ = _cpu_agent()
    for name, sizes in (("critic", [(4, 4)]), ("actor", [(5,)]), ("encoder", [(3,)]), ("cpc", [(2, 2), (3,)])):
        flat, gflat, params, _ = _flat(sizes)
        setattr(agent, name + "_optimizer", FlatAdam(params, flat, gflat))
    agent.set_max_grad_norm(7)
    st = agent.grad_clip_stats
    rows = dict(critic=0, actor=1, encoder=2, cpc=2)
    for name, row in rows.items():
        opt = getattr(agent, name + "_optimizer")
        assert opt.max_grad_norm == 7.0 and opt.clip_stats.data_ptr() == st[row].data_ptr()
    agent.set_max_grad_norm(None)
    assert all(getattr(agent, n + "_optimizer").max_grad_norm is None for n in rows)


def test_torch_optimizers_clip_at_the_same_call_sites():
    """With torch's own optimizers (a CPU agent) the phases call torch.nn.utils.clip_grad_norm_ on their live
    parameters and fill the stats from its result; a traced update computes nothing, so every gradient is zero:
    norm 0, coefficient 1 in all three rows, and the three norms are logged."""
    from curla_amd import _lib
    agent, rb = _cpu_agent()
    seen = []
    real = torch.nn.utils.clip_grad_norm_

    def spy(params, max_norm, *a, **k):
        seen.append((sum(p.numel() for p in params), max_norm))
        return real(params, max_norm, *a, **k)

    class Log:
        keys = []

        def log(self, key, *a, **k):
            self.keys.append(key)
    _lib.set_trace_hook(lambda n, a: None)
    torch.nn.utils.clip_grad_norm_ = spy
    try:
        agent.update(rb, Log(), 0)
        assert seen == [] and not any("grad_norm" in k for k in Log.keys)  # off by default
        agent.set_max_grad_norm(0.5)
        agent.grad_clip_stats.fill_(-1.0)
        agent.update(rb, Log(), 2)
    finally:
        torch.nn.utils.clip_grad_norm_ = real
        _lib.set_trace_hook(None)
    n_critic = sum(p.numel() for p in agent.critic.parameters())
    n_actor = sum(p.numel() for g in agent.actor_optimizer.param_groups for p in g["params"])
    n_cpc = agent.CURL.W.numel() + sum(p.numel() for p in agent.critic.encoder.parameters())
    assert seen == [(n_critic, 0.5), (n_actor, 0.5), (n_cpc, 0.5)]
    assert agent.grad_clip_stats.tolist() == [[0.0, 1.0]] * 3
    assert {"train_critic/grad_norm", "train_actor/grad_norm", "train/curl_grad_norm"} <= set(Log.keys)
    assert math.isfinite(float(agent.grad_clip_stats.sum()))
