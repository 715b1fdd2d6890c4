"""Same library calls, in the same order, with the same arguments: every launch and every collective of
``CurlSacAgent.update()`` on CPU agents and CPU buffers under the launch-trace hook (which computes nothing), over the
agent's options, against lists recorded on the commit BEFORE the three phase methods were rebuilt from shared building
blocks (``tests/update_launches.json``: per case and step the entry points in clear text and a SHA-256 of the canonical
JSON of the full list; ``python -m tests.test_update_launches_host`` prints the full lists, ``--write`` stores the table).

Scalars are recorded as they are.  An address is recorded as (named region, byte offset): the agent's flat and gradient
buffers, ``log_alpha`` and its gradient, the deterministic policy's device scalars, every tensor of the workspace by its storage (views resolve to one name), the
encoders' partial buffers, ``grad_clip_stats``, the flat optimizers' moment and partials buffers, the redo buffers and
the replay buffer's tensors by attribute.  An address in none of them is named by the order of its first appearance
(``ext0``, ...).  The small host arrays and structs some entry points take by address are recorded by content.
Data parallel: ``_allreduce`` / ``_allreduce_wait`` are replaced on the instance by recorders that append to the same
list, so the place of every collective among the launches is part of the record.

Behind the lists: the error path.  After an ``update()`` in which a phase raised the agent is in the state of a fresh
call -- every hand-over attribute idle, no pending collective, and the next ``update()`` launches what a fresh agent's
launches."""
import contextlib
import copy
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import curla_amd
from curla_amd import _lib, ops
from curla_amd.networks import LOG_FREQ
from curla_amd.optim import FlatAdam

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "update_launches.json")
C, IN_HW, OUT_HW, A, CAP = 9, (34, 40), (28, 34), 2, 32
# b8: the shape of tests/test_utd_host.py.  b128: the fused CURL head and the streaming fc forward apply (B % 128 == 0,
# F = 50, flat_dim = 11 * 14 * 16 a multiple of 32).  f68: F > 64, ops.fc_bwd_streams is false.
SHAPES = {"b8": (8, dict(num_filters=8)), "b128": (128, dict(num_filters=16, encoder_feature_dim=50)),
          "f68": (8, dict(num_filters=8, encoder_feature_dim=68))}
# actor and CURL phase every 4th step, a soft update every 2nd: (step, only_cpc) of the four kinds of update
FREQ = dict(actor_update_freq=4, cpc_update_freq=4)
STEPS = {"full": (4, False), "critic_soft": (2, False), "critic": (1, False), "only_cpc": (4, True)}
HIST_STEPS = {"full": (4 * LOG_FREQ, False), "critic_soft": (2 * LOG_FREQ, False), "critic": (LOG_FREQ, False),
              "only_cpc": (4 * LOG_FREQ, True)}
CASES = {
    "default": {},
    "b128": dict(shape="b128"),
    "f68": dict(shape="f68"),
    "detach_encoder": dict(agent=dict(detach_encoder=True)),
    "pixel_sac": dict(agent=dict(pixel_sac=True)),
    "layer_norm": dict(agent=dict(critic_layer_norm=True)),
    "layer_norm_dropout": dict(agent=dict(critic_layer_norm=True, critic_dropout=0.1)),
    "quantiles": dict(agent=dict(critic_quantiles=5, critic_drop_quantiles=1)),
    "prioritized": dict(rb=dict(prioritized=True)),
    "utd3": dict(agent=dict(utd_ratio=3)),
    "clip": dict(clip=1.0),
    "weight_decay": dict(agent=dict(weight_decay=0.01)),
    "four_q_off": dict(env=dict(CURLA_FOUR_Q="0")),
    "curl_unfused": dict(shape="b128", env=dict(CURLA_CURL_HEAD="unfused")),
    "hist": dict(agent=dict(log_param_hist_imgs=True), steps=HIST_STEPS),
    "logging": dict(agent=dict(log_interval=1)),
    "reference_buffer": dict(reference_buffer=True),
    "reference_buffer_f68": dict(shape="f68", reference_buffer=True),
    "noise": dict(noise=True, steps={k: STEPS[k] for k in ("full", "critic")}),
    "flat": dict(flat=True),
    "flat_b128": dict(shape="b128", flat=True),
    "flat_clip": dict(flat=True, clip=1.0),
    "flat_weight_decay": dict(flat=True, agent=dict(weight_decay=0.01)),
    "flat_detach_encoder": dict(flat=True, agent=dict(detach_encoder=True)),
    "dp_blocking": dict(dp="blocking"),
    "dp_overlap": dict(dp="overlap"),
    "dp_overlap_b128": dict(shape="b128", dp="overlap"),
    "dp_overlap_hist": dict(dp="overlap", agent=dict(log_param_hist_imgs=True)),
    "redo": dict(agent=dict(redo_recycle=False), redo=True, steps={}),
    "aug_views": dict(agent=dict(aug_views=2), rb=dict(aug_views=2)),
    "bins": dict(agent=dict(critic_bins=5, critic_value_range=(-4.0, 6.0))),
    "bins_views": dict(agent=dict(critic_bins=5, critic_value_range=(-4.0, 6.0), aug_views=2), rb=dict(aug_views=2)),
    "deterministic": dict(agent=dict(policy="deterministic")),
    "deterministic_schedule": dict(agent=dict(policy="deterministic", policy_std_schedule=(1.0, 0.1, 8.0))),
    "deterministic_flat": dict(flat=True, agent=dict(policy="deterministic")),
    "quantiles_flat": dict(flat=True, agent=dict(critic_quantiles=5, critic_drop_quantiles=1)),
    "bins_logging": dict(agent=dict(critic_bins=5, critic_value_range=(-4.0, 6.0), log_interval=1)),
    "deterministic_logging": dict(agent=dict(policy="deterministic", log_interval=1)),
}


# ---------------------------------------------------------------------------------------------------- agents and buffers
class Log:
    def log(self, *a, **k):
        pass

    log_histogram = log_param = log_image = log


class ReferenceBuffer:
    """A buffer that only offers the reference's ``sample_cpc()``: float tensors, no handles (the unmerged route)."""

    def __init__(self, B):
        f = lambda *s: torch.zeros(s)  # noqa: E731
        self.obs, self.next_obs, self.pos = (f(B, C, *OUT_HW) for _ in range(3))
        self.action, self.reward, self.not_done = f(B, A), f(B, 1), f(B, 1)

    def sample_cpc(self):
        kw = dict(obs_anchor=self.obs, obs_pos=self.pos, time_anchor=None, time_pos=None)
        return self.obs, self.action, self.reward, self.next_obs, self.not_done, kw


@contextlib.contextmanager
def _environ(values):
    old = {k: os.environ.get(k) for k in values}
    os.environ.update(values)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _flat_optimizers(agent):
    """FlatAdams over the agent's own flat buffers in place of the CPU agent's torch optimizers: the parameter lists
    of CurlSacAgent.__init__, each with the hyper-parameters of the optimizer it replaces."""
    actor_own = [p for n, p in agent.actor.named_parameters() if ".convs." not in n]
    enc = list(agent.critic.encoder.parameters())
    cf, cg = agent._critic_flat, agent._critic_gflat
    for name, params, flat, gflat in (("actor", actor_own, agent._actor_flat, agent._actor_gflat),
                                      ("critic", list(agent.critic.parameters()), cf, cg), ("encoder", enc, cf, cg),
                                      ("cpc", [agent.CURL.W] + enc, cf, cg)):
        g = getattr(agent, name + "_optimizer").param_groups[0]
        setattr(agent, name + "_optimizer", FlatAdam(params, flat, gflat, lr=g["lr"], betas=g["betas"], eps=g["eps"]))


def make(case, seed=1):
    """(agent, buffer) of a case of CASES, or of a case's description."""
    spec = CASES[case] if isinstance(case, str) else case
    B, shape_kw = SHAPES[spec.get("shape", "b8")]
    aug = curla_amd.RandomCrop(IN_HW, OUT_HW)
    curla_amd.set_seed_everywhere(seed)
    kw = {**dict(hidden_dim=64, num_layers=2, log_interval=1000), **FREQ, **shape_kw, **spec.get("agent", {})}
    with _environ(spec.get("env", {})):
        agent = curla_amd.CurlSacAgent((C,) + OUT_HW, (A,), "cpu", aug, **kw)
    if spec.get("flat"):
        _flat_optimizers(agent)
        if "weight_decay" in kw:
            agent.set_weight_decay(kw["weight_decay"])
    if spec.get("clip"):
        agent.set_max_grad_norm(spec["clip"])
    if spec.get("reference_buffer"):
        rb = ReferenceBuffer(B)
    else:
        rb = curla_amd.ReplayBuffer((C,) + IN_HW, (A,), max(CAP, 2 * B), B, "cpu", aug, **spec.get("rb", {}))
        rs = np.random.RandomState(3)
        for _ in range(12):
            f = rs.randint(0, 256, (C,) + IN_HW, dtype=np.uint8)
            rb.add(f, [0.1, -0.2], 0.5, f, False)
    curla_amd.set_seed_everywhere(seed + 10)
    return agent, rb


# ------------------------------------------------------------------------------------------------------------ recording
_OUT_INT = {"curla_conv3x3_s1_wgrad_slabs": 7, "curla_conv3x3_s1_bwd_slabs": 9, "curla_conv1_wgrad_slabs": 15,
            "curla_ln_bwd_partial": 10, "curla_curl_head": 12}  # the argument that is the address of a host int


def _host_arguments(name, args):
    """The arguments with every address of a host array or struct (they live as long as the call) replaced by
    ["host", content]; the addresses inside are resolved like any other."""
    args = list(args)

    def array(i, ctype, n):
        if args[i] is not None:
            args[i] = ["host", list((ctype * n).from_address(args[i]))]

    def structs(i, cls, n):
        items = (cls * n).from_address(args[i])
        args[i] = ["host", [[getattr(s, f) for f, _ in cls._fields_] for s in items]]
    P, I = ctypes.c_void_p, ctypes.c_int
    if name == "curla_conv3x3_s1_fwd_stack":
        for i in (2, 3, 4, 7, 8, 9):
            array(i, P, args[0])
    elif name == "curla_wgrad_reduce_multi":
        for i, t in ((1, P), (2, I), (3, I), (4, I), (5, P), (6, P)):
            array(i, t, args[0])
    elif name in ("curla_gemm_multi", "curla_fc_fwd_multi"):
        for i in (1, 2, 3):
            array(i, P, args[0])
    elif name == "curla_mlp_out_bwd_loss":
        structs(0, ops._LossArgs, 1)
    elif name == "curla_fc_ln_fwd_multi":
        structs(1, ops._FcLnJob, args[0])
    elif name == "curla_redo_recycle":
        structs(6, ops._RedoSeg, args[7])
    elif name in _OUT_INT:
        array(_OUT_INT[name], I, 1)
    return args


class FakeWork:
    def wait(self):
        pass


class Recorder:
    """The raw list of one or more calls: launches from the trace hook, collectives from the stand-ins of
    ``_allreduce`` / ``_allreduce_wait`` (an asynchronous one leaves a pending entry, as the real one does)."""

    def __init__(self, agent, rb):
        self.agent, self.rb, self.raw = agent, rb, []

    def hook(self, name, args):
        self.raw.append([name, _host_arguments(name, args)])

    def data_parallel(self, overlap):
        agent = self.agent
        agent._dp_active, agent._dp_overlap = True, overlap

        def allreduce(*buckets, async_op=False, f64_rider=None):
            for t in buckets:
                self.raw.append(["allreduce", [t.data_ptr(), t.numel(), bool(async_op), f64_rider is not None]])
                if async_op:
                    agent._dp_pending.append((FakeWork(), []))

        def wait():
            self.raw.append(["wait", []])
            agent._dp_pending = []
        agent._allreduce, agent._allreduce_wait = allreduce, wait

    def run(self, fn):
        start = len(self.raw)
        _lib.set_trace_hook(self.hook)
        try:
            fn()
        finally:
            _lib.set_trace_hook(None)
        return _resolve(self.raw[start:], _regions(self.agent, self.rb))


def _regions(agent, rb):
    """[(first byte, bytes, name)] of every allocation a launch of this agent on this buffer may address."""
    out, seen = [], set()

    def walk(name, obj):
        if torch.is_tensor(obj):
            s = obj.untyped_storage()
            if s.nbytes() and s.data_ptr() not in seen:
                seen.add(s.data_ptr())
                out.append((s.data_ptr(), s.nbytes(), name))
        elif isinstance(obj, (list, tuple)):
            for i, x in enumerate(obj):
                walk("%s[%d]" % (name, i), x)
        elif isinstance(obj, dict):
            for k, x in obj.items():
                if isinstance(k, (str, int)):
                    walk("%s[%s]" % (name, k), x)
    for name in ("_target_flat", "_critic_gflat", "_actor_flat", "_actor_gbucket", "log_alpha", "grad_clip_stats"):
        walk("flat" if name == "_target_flat" else name, getattr(agent, name))  # (one allocation: [target | critic])
    walk("log_alpha.grad", agent.log_alpha.grad)
    walk("actor.std", getattr(agent.actor, "std", None))  # (the deterministic policy's two device scalars)
    walk("_dla_scratch", getattr(agent, "_dla_scratch", None))
    for name, opt in agent._optimizers().items():
        if isinstance(opt, FlatAdam):
            for attr in ("_m", "_v", "_clip_partials", "clip_stats"):
                walk("%s_optimizer.%s" % (name, attr), getattr(opt, attr))
    for B, ws in agent._workspaces.items():
        for attr, value in vars(ws).items():
            walk("ws.%s" % attr, value)
    for name, enc in (("actor", agent.actor.encoder), ("critic", agent.critic.encoder),
                      ("critic_target", agent.critic_target.encoder)):
        walk("%s.encoder.partial" % name, enc._partial)
    walk("_redo_buf", agent._redo_buf)
    for attr, value in vars(rb).items():
        walk("rb.%s" % attr, value)
    return out


def _resolve(raw, regions):
    ext = {}

    def norm(x):
        if isinstance(x, (list, tuple)):
            return [norm(y) for y in x]
        if isinstance(x, np.generic):
            x = x.item()
        if isinstance(x, bool) or not isinstance(x, int):
            return x
        for lo, size, name in regions:
            if lo <= x < lo + size:
                return [name, x - lo]
        if abs(x) >= 1 << 24:
            return ["ext%d" % ext.setdefault(x, len(ext)), 0]
        return x
    return [[name, norm(args)] for name, args in raw]


def record(case):
    """{step kind: full list} of one case: the four kinds of update one after the other on ONE agent, so what a call
    leaves for the next (the encoder caches, the ring of index slots) is part of the record."""
    spec = CASES[case]
    agent, rb = make(case)
    rec = Recorder(agent, rb)
    if spec.get("dp"):
        rec.data_parallel(spec["dp"] == "overlap")
    out = {}
    for kind, (step, only_cpc) in spec.get("steps", STEPS).items():
        B = SHAPES[spec.get("shape", "b8")][0]
        noise = (torch.zeros(B, A), torch.zeros(B, A)) if spec.get("noise") else None
        out[kind] = rec.run(lambda: agent.update(rb, Log(), step, only_cpc=only_cpc, noise=noise))
    if spec.get("redo"):
        sample = []
        out["sample"] = rec.run(lambda: sample.append(rb.sample_cpc_refs()))
        out["redo_pass"] = rec.run(lambda: agent.redo_pass(sample[0][0], sample[0][1]))
    return out


def digest(calls):
    return hashlib.sha256(json.dumps(calls, sort_keys=True, separators=(",", ":")).encode()).hexdigest()


def summary(lists):
    return {kind: dict(names=[n for n, _ in calls], sha256=digest(calls)) for kind, calls in lists.items()}


_RECORDED = {}


def recorded(case):
    if case not in _RECORDED:
        _RECORDED[case] = record(case)
    return _RECORDED[case]


# ---------------------------------------------------------------------------------------------------------- launch lists
def expected():
    with open(TABLE) as f:
        return json.load(f)


def test_the_table_holds_exactly_the_cases():
    assert sorted(expected()) == sorted(CASES)


@pytest.mark.parametrize("case", sorted(CASES))
def test_update_launches_what_it_launched(case):
    EXPECTED = expected()
    got = summary(recorded(case))
    assert sorted(got) == sorted(EXPECTED[case])
    for kind in got:
        assert got[kind]["names"] == EXPECTED[case][kind]["names"], (case, kind)
        assert got[kind]["sha256"] == EXPECTED[case][kind]["sha256"], (case, kind)


def test_only_the_recording_steps_address_anything_unnamed():
    """Every address falls into a named region -- but for the copies a histogram step makes for the logger (tensors made
    during the call, named by the order of their first appearance): nothing else in the record depends on where a
    temporary happened to lie."""
    for case in CASES:
        for kind, calls in recorded(case).items():
            assert ('"ext' in json.dumps(calls)) == _has(calls, "curla_nhwc_to_nchw"), (case, kind)


def _has(calls, name, where=lambda args: True):
    return any(n == name and where(args) for n, args in calls)


def _pending_wait_order(calls):
    """Is there an asynchronous all-reduce of the actor's bucket that an optimizer launch does not follow directly?"""
    at = [i for i, (n, a) in enumerate(calls) if n == "allreduce" and a[0][0] == "_actor_gbucket" and a[2]]
    return bool(at) and calls[at[0] + 1][0] != "wait"


def _names(calls):
    return [n for n, _ in calls]


ROUTES = {
    # the critic phase's three forward routes: four Q functions in one batch; merged convs with separate Q passes (the
    # three fc products in one launch, no nested GEMM); fully separate passes (first-layer launches of one minibatch)
    "four_q": lambda c: _has(c, "curla_gemm_nested") and _has(c, "curla_fc_ln_fwd_multi", lambda a: a[0] == 3),
    "merged": lambda c: _has(c, "curla_gemm_multi", lambda a: a[0] == 3) and not _has(c, "curla_gemm_nested")
    and _names(c).count("curla_fc_ln_fwd") == 3 and _has(c, "curla_conv1_fwd2"),
    "unmerged": lambda c: _names(c).count("curla_conv1_fwd") >= 3 and _names(c).count("curla_fc_ln_fwd") == 3
    and not _has(c, "curla_conv1_fwd2"),
    "curl_head_fused": lambda c: _has(c, "curla_curl_head") and _has(c, "curla_fc_bwd_ln2"),
    "curl_head_unfused": lambda c: _has(c, "curla_curl_ce"),
    "fc_forward_streaming": lambda c: _has(c, "curla_fc_fwd_multi"),
    "fc_forward_not_streaming": lambda c: _has(c, "curla_gemm_multi"),
    "fc_backward_streaming": lambda c: _has(c, "curla_fc_bwd_ln") and _has(c, "curla_fc_dw_ln"),
    "fc_backward_not_streaming": lambda c: _has(c, "curla_ln_bwd_twin") and _has(c, "curla_ln_bwd")
    and not _has(c, "curla_fc_bwd_ln") and not _has(c, "curla_fc_dw_ln"),
    "deferred_actor_step": _pending_wait_order,
    "actor_step_not_deferred": lambda c: any(n == "allreduce" and a[3] and a[2] and c[i + 1][0] == "wait"
                                             for i, (n, a) in enumerate(c)),
    "step_with_lerp": lambda c: any(n.endswith("_step_lerp") or n.endswith("_step_lerp_clip") for n in _names(c)),
    "step_pair": lambda c: any("_step2" in n for n in _names(c)),
    "soft_update_launch": lambda c: _has(c, "curla_soft_update2"),
    "quantile_losses": lambda c: _has(c, "curla_tqc_critic_loss") and _has(c, "curla_tqc_actor_loss"),
    "prioritized": lambda c: _has(c, "curla_critic_td_loss") and _has(c, "curla_per_td"),
    "fused_loss": lambda c: _has(c, "curla_mlp_out_bwd_loss"),
    "layer_norm": lambda c: _has(c, "curla_mlp_ln_relu_fwd") and _has(c, "curla_mlp_ln_bwd"),
    "dropout": lambda c: _has(c, "curla_mlp_drop_ln_relu_fwd") and _has(c, "curla_mlp_drop_ln_bwd"),
    "records": lambda c: _has(c, "curla_nhwc_to_nchw"),
    "collective_blocking": lambda c: _has(c, "allreduce", lambda a: not a[2]),
    "collective_overlapped": lambda c: _has(c, "allreduce", lambda a: a[2]) and _has(c, "wait"),
    "redo_pass": lambda c: _has(c, "curla_dormant_mask"),
}


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_every_route_occurs_in_some_case(route):
    hits = [(case, kind) for case in CASES for kind, calls in recorded(case).items() if ROUTES[route](calls)]
    assert hits, route


# ------------------------------------------------------------------------------------------------------------ error path
HANDOVER_IDLE = dict(_soft_update_hint=False, _soft_update_done=False, _pos_hint=None, _pos_fc_done=False,
                     _anchor_cache=None, _pos_cache=None, _defer_actor_step=False, _actor_step_pending=False,
                     _actor_norm_log=None, _utd_leading=False)


def _raising(agent, phase, after=True):
    """Replace ``phase`` on the instance by one that runs the real phase first (``after``) and then raises."""
    real = getattr(agent, phase)

    def boom(*a, **k):
        if after:
            real(*a, **k)
        raise RuntimeError("injected")
    setattr(agent, phase, boom)
    return lambda: delattr(agent, phase)


def _failed_then_next(phase, step=4, utd=1, after=True):
    """The recorded overlapped data-parallel setup with ``phase`` raising during update(step) -- at once, or ``after``
    the real phase has run.  Returns (the hand-over attributes behind the failed call, its pending collectives, what it
    recorded, the next update's list, a fresh agent's list for that update on a copy of the buffer, the calls of
    _reset_handover)."""
    spec = dict(dp="overlap", agent=dict(utd_ratio=utd))
    (agent, rb), (fresh_agent, _) = make(spec), make(spec)
    rec = Recorder(agent, rb)
    rec.data_parallel(True)
    resets = []
    real_reset = agent._reset_handover

    def counted(*a, **k):
        resets.append((a, k))
        return real_reset(*a, **k)
    agent._reset_handover = counted
    undo = _raising(agent, phase, after)
    with pytest.raises(RuntimeError, match="injected"):
        rec.run(lambda: agent.update(rb, Log(), step))
    failed = list(rec.raw)
    undo()
    state = {k: getattr(agent, k) for k in HANDOVER_IDLE}
    pending = list(agent._dp_pending)
    fresh_rb = copy.deepcopy(rb)
    nxt = rec.run(lambda: agent.update(rb, Log(), step))
    fresh = Recorder(fresh_agent, fresh_rb)
    fresh.data_parallel(True)
    want = fresh.run(lambda: fresh_agent.update(fresh_rb, Log(), step))
    return state, pending, failed, nxt, want, resets


def test_update_cpc_raising_under_a_deferred_actor_step_loses_nothing():
    state, pending, failed, nxt, want, resets = _failed_then_next("update_cpc", after=False)
    assert state == HANDOVER_IDLE and pending == []
    # the actor's bucket went out asynchronously, its step was deferred -- and the reset waited for it
    names = [n for n, _ in failed]
    bucket = [i for i, (n, a) in enumerate(failed) if n == "allreduce" and a[3]]
    assert len(bucket) == 1 and "wait" in names[bucket[0] + 1:]
    assert len(resets) == 1
    assert nxt == want and _pending_wait_order(nxt)


@pytest.mark.parametrize("phase", ["update_critic", "update_actor_and_alpha", "update_cpc"])
@pytest.mark.parametrize("after", [False, True], ids=["at_once", "at_its_end"])
def test_a_phase_that_raises_leaves_the_agent_as_a_fresh_call_finds_it(phase, after):
    state, pending, failed, nxt, want, resets = _failed_then_next(phase, after=after)
    assert state == HANDOVER_IDLE and pending == []
    assert len(resets) == 1
    assert nxt == want


def test_a_leading_sub_step_that_raises_takes_the_same_reset():
    state, pending, failed, nxt, want, resets = _failed_then_next("update_critic", utd=3)
    assert state == HANDOVER_IDLE and pending == []
    assert len(resets) == 1  # the one method, once: from the leading sub-step's error path
    assert [n for n, _ in failed].count("curla_conv1_fwd2") == 1  # one sub-step ran and nothing followed
    assert nxt == want
    # ... and from _update_phases' own, for a final sub-step: the same method, once
    assert len(_failed_then_next("update_actor_and_alpha", utd=3)[5]) == 1


if __name__ == "__main__":
    import sys
    table = {case: record(case) for case in sorted(CASES)}
    if "--write" in sys.argv:
        with open(TABLE, "w") as f:
            f.write("{\n" + ",\n".join('"%s": %s' % (case, json.dumps(summary(lists), separators=(",", ":")))
                                       for case, lists in table.items()) + "\n}\n")
    else:
        for case, lists in table.items():
            for kind, calls in lists.items():
                print("==", case, kind, digest(calls))
                for name, args in calls:
                    print(name, json.dumps(args, separators=(",", ":")))
