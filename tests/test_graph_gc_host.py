"""The cyclic collector around an update-graph capture (agent_graphs._collector_held_off): off inside the captured
region, back as it was behind it -- when the body ends, when it raises, when the caller had it off already, and around a
capture of update() that raises half way.
The capture is the host stand-in of tests/test_graph_aug_host.py (a CPU agent under the trace hook); no GPU."""
import contextlib
import gc

import numpy as np
import pytest
import torch

import curla_amd
from curla_amd import _lib
from curla_amd.agent_graphs import _collector_held_off

HW, C = (28, 34), 9


class _Log:
    def log(self, *a, **k):
        pass


def test_the_context_manager_restores_the_collector():
    assert gc.isenabled()
    with _collector_held_off():
        assert not gc.isenabled()
    assert gc.isenabled()
    with pytest.raises(RuntimeError, match="inside"):
        with _collector_held_off():
            raise RuntimeError("inside")
    assert gc.isenabled()
    gc.disable()
    try:
        with _collector_held_off():
            assert not gc.isenabled()
        assert not gc.isenabled()  # (a caller that runs without the collector keeps running without it)
    finally:
        gc.enable()


def test_a_capture_that_raises_ran_without_the_collector_and_gives_it_back(monkeypatch):
    fails = True
    aug = curla_amd.RandomCrop((34, 40), HW)
    curla_amd.set_seed_everywhere(1)
    agent = curla_amd.CurlSacAgent((C,) + HW, (2,), "cpu", aug, hidden_dim=64, log_interval=1000)
    rb = curla_amd.ReplayBuffer((C, 34, 40), (2,), 32, 8, "cpu", aug)
    for _ in range(12):
        rb.add(np.zeros((C, 34, 40), np.uint8), [0, 0], 0.0, np.zeros((C, 34, 40), np.uint8), False)

    class FakeGraph:
        replays = 0

        def replay(self):
            FakeGraph.replays += 1
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    monkeypatch.setattr(torch.cuda, "CUDAGraph", FakeGraph)
    monkeypatch.setattr(torch.cuda, "graph", lambda *a, **k: contextlib.nullcontext())
    # what enable_update_graphs sets up (it refuses a CPU agent before anything else)
    agent._graphs, agent._graph_rb, agent._graph_warm, agent._graph_depth = {}, rb, 0, 2
    agent._graph_seen, agent._graph_key_at_capture = {}, None
    seen = dict(in_capture=[], outside=[])

    def hook(name, args):
        inside = agent._graph_cap is not None
        seen["in_capture" if inside else "outside"].append(gc.isenabled())
        if fails and inside and len(seen["in_capture"]) == 5:
            raise RuntimeError("injected capture failure")
    _lib.set_trace_hook(hook)
    try:
        assert gc.isenabled()
        with pytest.warns(RuntimeWarning, match="injected capture failure"):
            agent.update(rb, _Log(), 1)
    finally:
        _lib.set_trace_hook(None)
    assert gc.isenabled()
    assert seen["in_capture"] and not any(seen["in_capture"])  # every launch of the capture: collector off
    assert len(seen["in_capture"]) == 5 and seen["outside"] and all(seen["outside"])  # the eager update: on again
    assert FakeGraph.replays == 0
