"""CurlSacAgent(utd_ratio=G) on the host, under the launch-trace hook: nothing is computed on a device.
The keyword and its validation; that G = 1 is the agent without the keyword; the launch list of a G = 3 call as two
critic-only updates and the ordinary one; what ``ReplayBuffer.sample_cpc_refs(want_pos=False)`` leaves out and that it
draws what it draws otherwise; the checkpoint entry; ``only_cpc``; one set of log lines per call."""
import collections
import inspect
import warnings

import numpy as np
import pytest
import torch

import curla_amd
from curla_amd import _lib

C, IN_HW, B, CAP = 9, (34, 40), 8, 32
# actor and CURL phase every 4th step: steps 1, 2, 3 are critic-only updates, with (2) or without (1, 3) a soft update
# under critic_target_update_freq = 2
FREQ = dict(actor_update_freq=4, cpc_update_freq=4)
FULL_STEP, CRITIC_ONLY_STEP = 4, 2


def _augmentor(name):
    if name == "crop":
        return curla_amd.RandomCrop(IN_HW, (28, 34)), (28, 34)
    cls = dict(jiggle=curla_amd.ColorJiggle, conv=curla_amd.RandomConv, shift=curla_amd.RandomShift)[name]
    return cls(IN_HW), IN_HW


def make(aug_name="crop", rb_kw=None, seed=1, **kw):
    aug, out_hw = _augmentor(aug_name)
    curla_amd.set_seed_everywhere(seed)
    agent = curla_amd.CurlSacAgent((C,) + out_hw, (2,), "cpu", aug, hidden_dim=64, num_layers=2, num_filters=8,
                                   **{**dict(log_interval=1000), **kw})
    rb = curla_amd.ReplayBuffer((C,) + IN_HW, (2,), CAP, B, "cpu", aug, **(rb_kw or {}))
    rs = np.random.RandomState(3)
    for _ in range(12):
        f = rs.randint(0, 256, (C,) + IN_HW, dtype=np.uint8)
        rb.add(f, [0.1, -0.2], 0.5, f, False)
    curla_amd.set_seed_everywhere(seed + 10)
    return agent, rb


class Log:
    def __init__(self):
        self.keys = collections.Counter()

    def log(self, key, *a, **k):
        self.keys[key] += 1


def _shape(args):
    """A traced call's arguments with the addresses reduced to given / NULL (two agents' buffers differ)."""
    return tuple(a if a is None or isinstance(a, float) or abs(a) < 2 ** 20 else "ptr" for a in args)


def traced(fn):
    calls = []
    _lib.set_trace_hook(lambda name, args: calls.append((name, _shape(args))))
    try:
        fn()
    finally:
        _lib.set_trace_hook(None)
    return calls


def traced_update(step, aug_name="crop", rb_kw=None, only_cpc=False, log=None, **kw):
    agent, rb = make(aug_name, rb_kw, **kw)
    return traced(lambda: agent.update(rb, log or Log(), step, only_cpc=only_cpc))


def _states():
    s = np.random.get_state()
    return torch.get_rng_state().clone(), (s[1].copy(), s[2], s[3], s[4])


def _same(a, b):
    return torch.equal(a[0], b[0]) and np.array_equal(a[1][0], b[1][0]) and a[1][1:] == b[1][1:]


# ------------------------------------------------------------------------------------------------- keyword, validation
def test_keyword_of_the_class_call_beside_the_critic_keywords():
    init = list(inspect.signature(curla_amd.CurlSacAgent.__init__).parameters)
    assert init[-1] == "pixel_sac" and "utd_ratio" not in init
    call = inspect.signature(curla_amd.CurlSacAgent).parameters
    assert call["utd_ratio"].default == 1 and call["utd_ratio"].kind is inspect.Parameter.KEYWORD_ONLY
    names = list(call)
    # not between the two critic keywords, which stay neighbours with critic_layer_norm the last keyword of the call
    assert abs(names.index("critic_dropout") - names.index("critic_layer_norm")) == 1
    assert names.index("utd_ratio") < min(names.index("critic_dropout"), names.index("critic_layer_norm"))
    assert names[-2] == "critic_layer_norm"
    assert make()[0].utd_ratio == 1 and make(utd_ratio=20)[0].utd_ratio == 20
    assert type(make(utd_ratio=np.int64(4))[0].utd_ratio) is int


@pytest.mark.parametrize("bad", [0, -1, 1.5, True, "2"])
def test_validation(bad):
    with pytest.raises(ValueError, match="utd_ratio"):
        make(utd_ratio=bad)
    # edited later: the next update() refuses it before anything is drawn or launched
    agent, rb = make(utd_ratio=2)
    agent.utd_ratio = bad
    before = _states()
    calls = []
    _lib.set_trace_hook(lambda name, args: calls.append(name))
    try:
        with pytest.raises(ValueError, match="utd_ratio"):
            agent.update(rb, Log(), FULL_STEP)
    finally:
        _lib.set_trace_hook(None)
    assert not calls and _same(before, _states())


def test_noise_stands_for_one_minibatch():
    agent, rb = make(utd_ratio=2)
    with pytest.raises(ValueError, match="utd_ratio"):
        agent.update(rb, Log(), FULL_STEP, noise=(torch.zeros(B, 2), torch.zeros(B, 2)))


# ------------------------------------------------------------------------------------------------------------ defaults
def test_ratio_one_is_the_agent_without_the_keyword():
    assert make(utd_ratio=1)[0]._graph_key() == make()[0]._graph_key()
    assert make(utd_ratio=7)[0]._graph_key() == make()[0]._graph_key()  # plain replays: no graph holds the ratio
    for step in (2, 1):
        for hp in ({}, FREQ):
            assert traced_update(step, utd_ratio=1, **hp) == traced_update(step, **hp)


# -------------------------------------------------------------------------------------------------------- launch lists
@pytest.mark.parametrize("freq", [1, 2])
def test_launch_list_of_three_sub_steps(freq):
    """G = 3 at a step with actor and CURL phase = 2 x the critic-only update with the same soft-update decision + the
    ordinary update of that step.  (RandomCrop launches nothing for the positive: the lists are equal as they are.)"""
    hp = dict(FREQ, critic_target_update_freq=freq)
    full, lead = traced_update(FULL_STEP, **hp), traced_update(CRITIC_ONLY_STEP, **hp)
    names = [n for n, _ in lead]
    assert names.count("curla_soft_update2") == 1 and len(full) > len(lead) + 10  # (both softly update; full has more)
    without = traced_update(1, **hp)
    assert [n for n, _ in without].count("curla_soft_update2") == (1 if freq == 1 else 0)
    got = traced_update(FULL_STEP, utd_ratio=3, **hp)
    assert got == lead + lead + full
    # at a step whose own kind is critic-only the final sub-step is that update
    last = traced_update(1, **hp)
    assert traced_update(1, utd_ratio=3, **hp) == last * 3
    # the logging step's extra launch (the batch reward's mean) belongs to the final sub-step alone
    logged = traced_update(FULL_STEP, utd_ratio=3, log_interval=FULL_STEP, **hp)
    assert [n for n, _ in logged].count("curla_mean") == 1 and logged[:2 * len(lead)] == lead + lead


def _drop_nth(calls, name, nth):
    at = [i for i, (n, _) in enumerate(calls) if n == name][nth]
    return calls[:at] + calls[at + 1:]


@pytest.mark.parametrize("aug_name,staged,kernel", [("jiggle", False, "curla_color_jiggle"), ("jiggle", True, "curla_color_jiggle"),
                                                     ("conv", False, "curla_random_conv"), ("conv", True, "curla_random_conv")])
@pytest.mark.parametrize("dedup", [False, True])
def test_leading_sub_steps_lack_exactly_the_positives_float_launch(aug_name, staged, kernel, dedup):
    hp = dict(FREQ, critic_target_update_freq=1)
    rb_kw = dict(staged_aug=staged, dedup_frames=dedup)
    full = traced_update(FULL_STEP, aug_name, rb_kw, **hp)
    lead = traced_update(CRITIC_ONLY_STEP, aug_name, rb_kw, **hp)
    assert [n for n, _ in lead].count(kernel) == 3
    got = traced_update(FULL_STEP, aug_name, rb_kw, utd_ratio=3, **hp)
    lean = _drop_nth(lead, kernel, 2)
    assert got == lean + lean + full


@pytest.mark.parametrize("rb_kw", [{}, dict(dedup_frames=True), dict(pos_offset=2), dict(pos_offset=2, dedup_frames=True)],
                         ids=["plain", "dedup", "pos_offset", "pos_offset, dedup"])
def test_leading_sub_steps_shift_two_tensors_and_gather_two(rb_kw):
    """A scratch augmentation's one launch of n = 3B becomes n = 2B, the positive's gather_stacks and the positive's walk
    (a launch of its own on a buffer that copies its block: this CPU one) are not launched, nothing else differs."""
    hp = dict(FREQ, critic_target_update_freq=1)
    full = traced_update(FULL_STEP, "shift", rb_kw, **hp)
    lead = traced_update(CRITIC_ONLY_STEP, "shift", rb_kw, **hp)
    got = traced_update(FULL_STEP, "shift", rb_kw, utd_ratio=3, **hp)
    assert got[2 * (len(got) - len(full)) // 2:] == full
    sub = got[:(len(got) - len(full)) // 2]
    assert got[len(sub):2 * len(sub)] == sub
    want = list(lead)
    if rb_kw.get("pos_offset"):
        want = _drop_nth(want, "curla_pos_walk", 0)
        if rb_kw.get("dedup_frames"):
            assert [n for n, _ in want].count("curla_gather_stacks") == 3
            want = _drop_nth(want, "curla_gather_stacks", 2)
    assert [n for n, _ in sub] == [n for n, _ in want]
    n_seen = []
    for (n0, a0), (n1, a1) in zip(want, sub):
        if n0 != "curla_random_shift_u8":
            assert a0 == a1, n0
            continue
        n_seen.append((a0[6], a1[6]))
        assert a0[7:] == a1[7:] and a0[3:6] == a1[3:6]  # (rows and period are the obs | next_obs run's with pos_offset)
    assert n_seen == [(3 * B, 2 * B)]


# -------------------------------------------------------------------------------------------------------- the sampler
@pytest.mark.parametrize("aug_name,rb_kw", [("crop", {}), ("jiggle", {}), ("jiggle", dict(staged_aug=True)), ("conv", {}),
                                            ("shift", dict(pos_offset=1))])
def test_want_pos_false_draws_the_same_and_returns_no_positive(aug_name, rb_kw):
    ends, lists = [], []
    for want_pos in (None, True, False):
        _, rb = make(aug_name, rb_kw)
        kw = {} if want_pos is None else dict(want_pos=want_pos)
        out = []
        lists.append(traced(lambda: out.append(rb.sample_cpc_refs(**kw))))
        ends.append(_states())
        pos = out[0][5]["obs_pos"]
        assert (pos is None) == (want_pos is False)
        assert out[0][5]["obs_anchor"] is out[0][0]
    assert _same(ends[0], ends[1]) and _same(ends[0], ends[2])
    assert lists[0] == lists[1]  # without the argument, and with its default: today's launches
    assert len(lists[2]) <= len(lists[0])


def test_draws_of_a_call_are_those_of_its_samples(monkeypatch):
    """After one G = 3 call NumPy's and torch's host streams stand where three ``sample_cpc_refs()`` calls leave them.
    (A HIP agent draws its policy noise from the DEVICE generator; the CPU agent of this test would take it from torch's
    CPU stream, so its draw is switched off here: the host streams then see the sampler alone, as on the device.)"""
    for aug_name in ("crop", "jiggle", "conv"):
        agent, rb = make(aug_name, utd_ratio=3, **FREQ)
        monkeypatch.setattr(agent, "_noise", lambda ws, noise: (ws.noise, None))
        traced(lambda: agent.update(rb, Log(), FULL_STEP))
        after_call = _states()
        _, twin = make(aug_name)
        start = _states()
        traced(lambda: [twin.sample_cpc_refs() for _ in range(3)])
        assert _same(after_call, _states()), aug_name
        assert not _same(start, _states())


# --------------------------------------------------------------------------------------------------------- checkpoints
def test_checkpoint_records_the_ratio_and_a_mismatch_warns(tmp_path):
    one, three = make()[0], make(utd_ratio=3)[0]
    f1, f3, f_old = (str(tmp_path / n) for n in ("one.pt", "three.pt", "old.pt"))
    one.save_checkpoint(f1, 5)
    three.save_checkpoint(f3, 6)
    assert torch.load(f1, weights_only=False)["utd_ratio"] == 1 and torch.load(f3, weights_only=False)["utd_ratio"] == 3
    with pytest.warns(RuntimeWarning, match="utd_ratio"):
        assert one.load_checkpoint(f3) == 6
    assert one.utd_ratio == 1
    with pytest.warns(RuntimeWarning, match="utd_ratio"):
        assert three.load_checkpoint(f1) == 5
    assert three.utd_ratio == 3
    # a file from before the keyword loads as 1: silently into a ratio-1 agent
    ck = torch.load(f1, weights_only=False)
    del ck["utd_ratio"]
    torch.save(ck, f_old)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert one.load_checkpoint(f_old) == 5 and one.load_checkpoint(f1) == 5
    with pytest.warns(RuntimeWarning, match="utd_ratio = 1"):
        three.load_checkpoint(f_old)
    assert three.utd_ratio == 3


# ------------------------------------------------------------------------------------------------- only_cpc and logging
def test_only_cpc_has_no_leading_sub_steps():
    assert traced_update(FULL_STEP, utd_ratio=3, only_cpc=True, **FREQ) == traced_update(FULL_STEP, only_cpc=True, **FREQ)


def test_a_logging_step_logs_every_key_once():
    one, three = Log(), Log()
    traced_update(FULL_STEP, log=one, log_interval=1, **FREQ)
    traced_update(FULL_STEP, log=three, utd_ratio=3, log_interval=1, **FREQ)
    assert three.keys == one.keys and set(one.keys.values()) == {1}
    assert {"train/batch_reward", "train_critic/loss", "train_actor/loss", "train/curl_loss"} <= set(one.keys)
    assert all(k.startswith("train") for k in one.keys)


def test_a_leading_sub_step_that_raises_ends_the_call(monkeypatch):
    agent, rb = make(utd_ratio=3, critic_target_update_freq=1, **FREQ)
    seen = []

    def boom(*a, **k):
        seen.append(agent._soft_update_hint)
        raise RuntimeError("injected")
    monkeypatch.setattr(agent, "update_critic", boom)
    with pytest.raises(RuntimeError, match="injected"):
        traced(lambda: agent.update(rb, Log(), FULL_STEP))
    assert seen == [True]  # one sub-step ran, announced its soft update, and nothing followed
    assert agent._soft_update_hint is False and agent._soft_update_done is False and agent._utd_leading is False
