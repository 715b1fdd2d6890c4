"""Host side of the batched acting calls (CurlSacAgent.select_actions / sample_actions), without a GPU: argument
errors come first and name the accepted shapes, a valid call on a CPU agent raises (no CPU fallback), the C ABI is
at version 8 with curla_stage_frames_u8 in the binding table, and -- on the launch-trace hook, where nothing is
computed -- N frames are staged by ONE curla_stage_frames_u8 launch that carries the centre window."""
import os
import re

import numpy as np
import pytest
import torch

import curla_amd
from curla_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HP = dict(num_layers=4, num_filters=32, encoder_feature_dim=50)


def _agent(aug=None):
    aug = aug or curla_amd.RandomCrop((34, 40), (28, 34))
    torch.manual_seed(1)
    return curla_amd.CurlSacAgent((9, 28, 34), (2,), "cpu", aug, hidden_dim=64, **HP)


def _frames(n, c=9, hw=(34, 40), seed=0):
    return np.random.RandomState(seed).randint(0, 256, (n, c) + hw, dtype=np.uint8)


@pytest.mark.parametrize("method", ["select_actions", "sample_actions"])
def test_argument_errors_name_the_accepted_shapes(method):
    call = getattr(_agent(), method)
    bad = {
        "wrong rank": _frames(1)[0],
        "wrong channel count": _frames(2, c=6),
        "frame size that is neither accepted one": _frames(2, hw=(30, 36)),
        "empty batch": _frames(0),
        "empty list": [],
        "frames of different shapes": [_frames(1)[0], _frames(1, hw=(28, 34))[0]],
        "float array of the wrong size": _frames(2, hw=(30, 36)).astype(np.float32),
    }
    for what, obs in bad.items():
        with pytest.raises(ValueError) as e:
            call(obs)
        msg = str(e.value)
        assert "(28, 34)" in msg and "(34, 40)" in msg and "(N, 9, H, W)" in msg, (what, msg)


def test_noise_of_the_wrong_shape_is_refused():
    agent = _agent()
    for noise in (torch.zeros(2, 2), torch.zeros(3), torch.zeros(3, 3), np.zeros((3, 2), np.float32)):
        with pytest.raises(ValueError) as e:
            agent.sample_actions(_frames(3), noise=noise)
        assert "(N, A) = (3, 2)" in str(e.value)


def test_identity_augmentation_accepts_one_size_only():
    agent = _agent(curla_amd.IdentityAugmentation((28, 34)))
    with pytest.raises(ValueError) as e:
        agent.select_actions(_frames(2))
    assert "(28, 34)" in str(e.value) and "(34, 40)" not in str(e.value)


@pytest.mark.parametrize("obs", [_frames(3), list(_frames(3)), _frames(3, hw=(28, 34)), _frames(3).astype(np.float32),
                                 torch.from_numpy(_frames(3))], ids=["array", "list", "pre-cropped", "float", "tensor"])
def test_valid_call_on_a_cpu_agent_raises_like_update(obs):
    agent = _agent()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        agent.select_actions(obs)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        agent.sample_actions(obs, noise=torch.zeros(3, 2))
    assert not agent._act_batch_stage  # nothing was allocated on the way to the error


def test_abi_is_version_8_and_binds_the_staging_entry_point():
    text = open(os.path.join(ROOT, "include", "curla_hip.h")).read()
    assert re.search(r"#define\s+CURLA_ABI_VERSION\s+8\b", text)
    assert re.search(r"\bint\s+curla_stage_frames_u8\s*\(", text)
    assert _lib.ABI_VERSION == 8
    args = _lib.SIGNATURES["curla_stage_frames_u8"]
    assert len(args) == 12 and args[2] is _lib.c_ll and args[0] is _lib.vp and args[-1] is _lib.vp
    import __graft_entry__ as ge
    ge.build()
    lib = _lib.load()
    assert int(lib.curla_abi_version()) == 8 and hasattr(lib, "curla_stage_frames_u8")


def test_entry_point_refuses_bad_windows_on_the_host():
    """The argument checks run before any launch, so they can be exercised without a device: every refused call
    returns CURLA_ERR_ARG (-1) and touches no memory."""
    import __graft_entry__ as ge
    ge.build()
    fn = _lib.load().curla_stage_frames_u8
    src, ring = np.zeros(3 * 10 * 12, np.uint8), np.zeros(3 * 8 * 8 + 32, np.uint8)
    p, q = src.ctypes.data, ring.ctypes.data
    ok = dict(first_slot=0, N=1, C=3, Hs=10, Ws=12, top=1, left=2, Hd=8, Wd=8)
    for edit in (dict(top=3), dict(left=5), dict(top=-1), dict(left=-1), dict(N=0), dict(C=0), dict(first_slot=-1),
                 dict(Hd=0), dict(Wd=13, left=0), dict(Hd=11, top=0)):
        a = {**ok, **edit}
        rc = fn(p, q, a["first_slot"], a["N"], a["C"], a["Hs"], a["Ws"], a["top"], a["left"], a["Hd"], a["Wd"], None)
        assert rc == -1, edit
    assert fn(None, q, 0, 1, 3, 10, 12, 1, 2, 8, 8, None) == -1 and fn(p, None, 0, 1, 3, 10, 12, 1, 2, 8, 8, None) == -1
    assert not ring.any()


def test_launch_schedule_one_staging_launch_for_n_frames():
    """On the trace hook (nothing is computed): N = 5 pre-crop frames -> exactly one curla_stage_frames_u8 call with
    N = 5 and the centre window, then the conv stack at B = 5 from the ring it wrote; pre-cropped frames give the
    whole-frame window; a float batch stages nothing; a second call allocates nothing new."""
    agent = _agent()
    calls = []
    _lib.set_trace_hook(lambda name, args: calls.append((name, args)))
    try:
        out = agent.select_actions(_frames(5), as_tensor=True)
        assert tuple(out.shape) == (5, 2)
        staged = [a for n, a in calls if n == "curla_stage_frames_u8"]
        assert len(staged) == 1
        _, ring_ptr, first, N, C, Hs, Ws, top, left, Hd, Wd, _ = staged[0]
        assert (first, N, C, Hs, Ws, top, left, Hd, Wd) == (0, 5, 9, 34, 40, 3, 3, 28, 34)
        conv1 = [a for n, a in calls if n == "curla_conv1_fwd"]
        assert len(conv1) == 1 and conv1[0][0] == ring_ptr and conv1[0][1] == 1 and conv1[0][8] == 5
        assert [n for n, _ in calls].index("curla_stage_frames_u8") < [n for n, _ in calls].index("curla_conv1_fwd")
        st = agent._act_batch_stage[(9, 34, 40)]
        blocks = (st["ring"], st["src"], [p[0] for p in st["pins"]])
        del calls[:]
        agent.sample_actions(_frames(3, seed=1), noise=torch.zeros(3, 2))  # fewer frames: same blocks
        st2 = agent._act_batch_stage[(9, 34, 40)]
        assert st2 is st and st2["ring"] is blocks[0] and st2["src"] is blocks[1]
        assert [a[3] for n, a in calls if n == "curla_stage_frames_u8"] == [3]
        del calls[:]
        agent.select_actions(_frames(4, hw=(28, 34)))
        staged = [a for n, a in calls if n == "curla_stage_frames_u8"]
        assert len(staged) == 1 and staged[0][3:11] == (4, 9, 28, 34, 0, 0, 28, 34)
        del calls[:]
        agent.select_actions(_frames(4).astype(np.float32))
        assert not [n for n, _ in calls if n == "curla_stage_frames_u8"]
        assert [a[1] for n, a in calls if n == "curla_conv1_fwd"] == [0]  # the float NCHW source
    finally:
        _lib.set_trace_hook(None)
