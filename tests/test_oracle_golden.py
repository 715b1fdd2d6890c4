"""Pins oracle/curla_oracle.py to the golden vectors generated from the
reference (tests/golden/make_goldens.py).  CPU only."""
import hashlib

import numpy as np
import torch

from oracle import curla_oracle as O
from tests._util import assert_close, like, load, sub, summarize

torch.set_num_threads(1)
HP = dict(num_layers=4, log_std_min=-10, log_std_max=2)


def _f(x):
    return torch.from_numpy(np.asarray(x, dtype=np.float32))


def test_shape_arithmetic_matches_reference_tables():
    # encoder.py:21-29 rows that are well-formed in the reference
    assert O.conv_out_hw(76, 135, 4) == (31, 61)
    assert O.conv_out_hw(90, 160, 4) == (38, 73)
    # the square tables (ints in the reference, encoder.py:21-23)
    assert [O.conv_out_hw(84, 84, n)[0] for n in (2, 4, 6)] == [39, 35, 31]
    assert [O.conv_out_hw(64, 64, n)[0] for n in (2, 4, 6)] == [29, 25, 21]
    g = load("crop84.npz")
    assert tuple(g["default_shape_84"]) == O.random_crop_output_shape((84, 84))
    assert tuple(g["default_shape_90_160"]) == O.random_crop_output_shape((90, 160))


def test_random_crop_bit_exact_84_to_76():
    g = load("crop84.npz")
    imgs = np.random.RandomState(int(g["imgs_seed"])).randint(0, 256, (16, 9, 84, 84), dtype=np.uint8)
    rs = np.random.RandomState(int(g["numpy_seed"]))
    h1 = rs.randint(0, 8, 16)
    w1 = rs.randint(0, 8, 16)
    assert np.array_equal(h1, g["h1"]) and np.array_equal(w1, g["w1"])
    assert h1.max() <= 7  # exclusive upper bound (augmentations.py:66-67)
    out = O.random_crop(imgs, h1, w1, (76, 76))
    assert hashlib.sha256(out.tobytes()).hexdigest() == str(g["out_sha256"])
    assert np.array_equal(out[:2], g["out_first2"])
    assert np.array_equal(O.center_crop(imgs[0], (76, 76)), g["center_crop0"])


def test_crop_fixture_under_the_genuine_skimage():
    """make_goldens.py records crop84.npz with ``sliding_window_view`` standing in for skimage's ``view_as_windows``
    (this interpreter has no scikit-image).  crop84_skimage.npz holds what the reference's RandomCrop gives under the
    GENUINE scikit-image on the same images and seeds (tests/golden/check_crop_with_skimage.py --write): the fixture's
    index stream, bytes and shapes must be those, and so must the oracle's crops of the same images."""
    g, s = load("crop84.npz"), load("crop84_skimage.npz")
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()  # noqa: E731
    assert int(s["imgs_seed"]) == int(g["imgs_seed"]) and int(s["numpy_seed"]) == int(g["numpy_seed"])
    for k in ("default_shape_84", "default_shape_90_160", "h1", "w1"):
        assert np.array_equal(g[k], s[k]), k
    assert str(g["out_sha256"]) == str(s["out_sha256"])
    assert sha(g["out_first2"]) == str(s["out_first2_sha256"])
    assert sha(g["center_crop0"]) == str(s["center_crop0_sha256"])
    imgs = np.random.RandomState(int(s["imgs_seed"])).randint(0, 256, (16, 9, 84, 84), dtype=np.uint8)
    assert sha(O.random_crop(imgs, s["h1"], s["w1"], (76, 76))) == str(s["out_sha256"])
    assert sha(O.center_crop(imgs[0], (76, 76))) == str(s["center_crop0_sha256"])
    assert tuple(s["default_shape_84"]) == O.random_crop_output_shape((84, 84))
    assert tuple(s["default_shape_90_160"]) == O.random_crop_output_shape((90, 160))


def test_sample_cpc_draw_order_bit_exact():
    g = load("tiny.npz")
    rs = np.random.RandomState()
    st = list(rs.get_state())
    st[1], st[2] = g["meta/numpy_state_keys"], int(g["meta/numpy_state_pos"])
    rs.set_state(tuple(st))
    ih, iw = g["meta/in_hw"]
    oh, ow = g["meta/out_hw"]
    idxs, offs = O.draw_sample_cpc_indices(int(g["meta/n_valid"]), 8, ih - oh, iw - ow, rng=rs)
    assert np.array_equal(idxs, g["rng/idxs"])
    for (h1, w1), nm in zip(offs, ("obs", "next_obs", "pos")):
        assert np.array_equal(h1, g[f"rng/h1_{nm}"]) and np.array_equal(w1, g[f"rng/w1_{nm}"])
    # and the cropped bytes the reference fed its networks
    for nm, full in (("obs", "obs_full"), ("next_obs", "next_obs_full"), ("pos", "obs_full")):
        out = O.random_crop(g[f"batch/{full}"], g[f"rng/h1_{nm}"], g[f"rng/w1_{nm}"], (oh, ow))
        assert np.array_equal(out, g[f"batch/{nm}"])


def _state(g):
    return (sub(g, "state0/actor/"), sub(g, "state0/critic/"), sub(g, "state0/critic_target/"),
            torch.from_numpy(g["state0/W"]), torch.from_numpy(g["state0/log_alpha"]))


def test_critic_phase_matches_reference():
    g = load("tiny.npz")
    actor, critic, target, W, la = _state(g)
    r = O.critic_phase(actor, critic, target, la, _f(g["batch/obs"]), _f(g["batch/action"]), _f(g["batch/reward"]),
                       _f(g["batch/next_obs"]), _f(g["batch/not_done"]), _f(g["noise/critic"]), discount=0.99, **HP)
    assert_close(r["policy_action"], g["critic/policy_action"], 1e-5, "policy_action")
    assert_close(r["next_log_pi"], g["critic/next_log_pi"], 1e-5, "next_log_pi")
    assert_close(r["q1"], g["critic/q1"], 1e-5, "q1")
    assert_close(r["q2"], g["critic/q2"], 1e-5, "q2")
    assert_close(r["loss"], g["scalar/train_critic/loss"], 1e-5, "critic loss")
    for k in ("conv1", "conv2", "conv3", "conv4", "fc", "ln"):
        assert_close(r["enc"][k], g[f"critic/enc/{k}"], 1e-5, k)
    n = 0
    for k, v in sub(g, "critic/grad/").items():
        assert_close(r["grads"][k], v, 1e-5, "critic grad " + k)
        n += 1
    assert n == 24  # curl_sac.py:301: all critic tensors get a gradient


def test_actor_phase_matches_reference():
    g = load("tiny.npz")
    actor, _, _, _, la = _state(g)
    critic = sub(g, "critic_after/")  # weights after the critic Adam step (curl_sac.py:368)
    r = O.actor_phase(actor, critic, la, _f(g["batch/obs"]), _f(g["noise/actor"]), target_entropy=-2.0, **HP)
    for k in ("pi", "log_pi", "log_std", "q1", "q2"):
        assert_close(r[k], g[f"actor/{k}"], 1e-5, k)
    assert_close(r["actor_loss"], g["scalar/train_actor/loss"], 1e-5, "actor loss")
    assert_close(r["alpha_loss"], g["scalar/train_alpha/loss"], 1e-5, "alpha loss")
    assert_close(r["entropy"], g["scalar/train_actor/entropy"], 1e-5, "entropy")
    assert_close(r["alpha"], g["scalar/train_alpha/value"], 1e-6, "alpha")
    assert_close(r["log_alpha_grad"], g["alpha/grad/log_alpha"], 1e-5, "log_alpha grad")
    ref = sub(g, "actor/grad/")
    assert len(ref) == 10 and set(ref) == set(r["grads"])  # convs get no actor gradient
    for k, v in ref.items():
        assert_close(r["grads"][k], v, 1e-5, "actor grad " + k)


def test_soft_update_matches_reference():
    g = load("tiny.npz")
    critic, target = sub(g, "critic_after/"), sub(g, "state0/critic_target/")
    O.soft_update(critic, target, 0.01, "Q1.")
    O.soft_update(critic, target, 0.01, "Q2.")
    O.soft_update(critic, target, 0.05, "encoder.")
    for k, v in sub(g, "target_after/").items():
        assert_close(target[k], v, 1e-6, "target " + k)


def test_cpc_phase_matches_reference():
    g = load("tiny.npz")
    critic, target = sub(g, "critic_after/"), sub(g, "target_after/")
    W = torch.from_numpy(g["state0/W"])
    r = O.cpc_phase(critic, target, W, _f(g["batch/obs"]), _f(g["batch/pos"]), num_layers=4)
    for k in ("z_a", "z_pos", "logits"):
        assert_close(r[k], g[f"cpc/{k}"], 1e-5, k)
    assert_close(r["loss"], g["scalar/train/curl_loss"], 1e-5, "curl loss")
    ref = sub(g, "cpc/grad/")
    assert len(ref) == 13
    for k, v in ref.items():
        got = r["W_grad"] if k == "W" else r["grads"][k]
        assert_close(got, v, 2e-5, "cpc grad " + k)


def test_float64_mode_matches_reference_and_reports_hidden_units():
    """The arbiter of tests/test_gpu_fullsize.py: every phase evaluated on float64 casts of the same arguments is the
    same function (the reference's fp32 numbers to 1e-4 -- fp32's own distance from the exact result --, results in
    float64), and the phases hand out the MLPs'
    hidden pre-activations, whose signs are the ReLU branches."""
    g = load("tiny.npz")
    actor, critic, target, W, la = _state(g)
    d = lambda x: O.as_dtype(x, torch.float64)  # noqa: E731
    b = lambda k: d(_f(g[k]))  # noqa: E731
    r = O.critic_phase(d(actor), d(critic), d(target), la, b("batch/obs"), b("batch/action"), b("batch/reward"),
                       b("batch/next_obs"), b("batch/not_done"), b("noise/critic"), discount=0.99, **HP)
    assert r["loss"].dtype == torch.float64 and r["target_Q"].dtype == torch.float64
    assert_close(r["loss"], g["scalar/train_critic/loss"], 1e-4, "critic loss (f64)")
    for k, v in sub(g, "critic/grad/").items():
        assert r["grads"][k].dtype == torch.float64
        assert_close(r["grads"][k], v, 1e-4, "critic grad (f64) " + k)
    B = g["batch/obs"].shape[0]
    assert [tuple(h.shape) for h in r["q_hidden"]] == [(B, critic["Q1.trunk.0.weight"].shape[0])] * 4
    # (the process's FIRST fp32 evaluation of these conv shapes is thrown away: oneDNN may run a primitive's first call
    # through another implementation than the cached one it uses from then on -- seen once in ~6 runs as a 6e-5
    # difference between two otherwise identical evaluations, which the bit-identity checks below would trip over)
    O.critic_phase(actor, critic, target, la, _f(g["batch/obs"]), _f(g["batch/action"]), _f(g["batch/reward"]),
                   _f(g["batch/next_obs"]), _f(g["batch/not_done"]), _f(g["noise/critic"]), discount=0.99, **HP)
    r32 = O.critic_phase(actor, critic, target, la, _f(g["batch/obs"]), _f(g["batch/action"]), _f(g["batch/reward"]),
                         _f(g["batch/next_obs"]), _f(g["batch/not_done"]), _f(g["noise/critic"]), discount=0.99, **HP)
    za = torch.cat([r32["enc"]["ln"], _f(g["batch/action"])], 1)
    want = torch.nn.functional.linear(za, critic["Q2.trunk.0.weight"], critic["Q2.trunk.0.bias"])
    assert_close(r32["q_hidden"][2], want, 1e-6, "Q2 hidden 1 pre-activation")
    critic_after = sub(g, "critic_after/")
    ra = O.actor_phase(d(actor), d(critic_after), la, b("batch/obs"), b("noise/actor"), target_entropy=-2.0, **HP)
    assert_close(ra["actor_loss"], g["scalar/train_actor/loss"], 1e-4, "actor loss (f64)")
    for k, v in sub(g, "actor/grad/").items():
        assert_close(ra["grads"][k], v, 1e-4, "actor grad (f64) " + k)
    assert len(ra["trunk_hidden"]) == 2 and len(ra["q_hidden"]) == 4
    rp = O.cpc_phase(d(critic_after), d(sub(g, "target_after/")), d(W), b("batch/obs"), b("batch/pos"), num_layers=4)
    assert_close(rp["loss"], g["scalar/train/curl_loss"], 1e-4, "curl loss (f64)")
    for k, v in sub(g, "cpc/grad/").items():
        assert_close(rp["W_grad"] if k == "W" else rp["grads"][k], v, 1e-4, "cpc grad (f64) " + k)
    # one forward pass, differentiated again: own branches = the plain gradients, given branches = the phase evaluated
    # along them (values untouched either way)
    args = (actor, critic, target, la, _f(g["batch/obs"]), _f(g["batch/action"]), _f(g["batch/reward"]),
            _f(g["batch/next_obs"]), _f(g["batch/not_done"]), _f(g["noise/critic"]))
    rr = O.critic_phase(*args, discount=0.99, regrad=True, **HP)
    for k, v in r32["grads"].items():
        assert torch.equal(rr["grads"][k], v), k
    again = rr["regrad"]()
    assert all(torch.equal(again[k], v) for k, v in r32["grads"].items())
    gen = torch.Generator().manual_seed(3)
    flip = lambda t: (t > 0) ^ (torch.rand(t.shape, generator=gen) < 0.01)  # noqa: E731
    conv_b = [flip(r32["enc"][f"conv{i + 1}"]) for i in range(4)]
    q_b = [[flip(h) for h in r32["q_hidden"][0:2]], [flip(h) for h in r32["q_hidden"][2:4]]]
    direct = O.critic_phase(*args, discount=0.99, relu_branches=conv_b, q_branches=q_b, **HP)
    swapped = rr["regrad"](relu_branches=conv_b, q_branches=q_b)
    assert float(direct["loss"]) == float(r32["loss"])
    moved = 0
    for k, v in direct["grads"].items():
        assert torch.equal(swapped[k], v), k
        moved += int(not torch.equal(v, r32["grads"][k]))
    assert moved >= 20  # (1 % of the branches flipped: every gradient below the Q heads' last layer moves)
    back = rr["regrad"]()
    assert all(torch.equal(back[k], v) for k, v in r32["grads"].items())
    rp32 = O.cpc_phase(critic_after, sub(g, "target_after/"), W, _f(g["batch/obs"]), _f(g["batch/pos"]), num_layers=4, regrad=True)
    eg, wg = rp32["regrad"]()
    assert torch.equal(wg, rp32["W_grad"]) and all(torch.equal(eg[k], v) for k, v in rp32["grads"].items())
    ra32 = O.actor_phase(actor, critic_after, la, _f(g["batch/obs"]), _f(g["noise/actor"]), target_entropy=-2.0, regrad=True, **HP)
    tb = [flip(h) for h in ra32["trunk_hidden"]]
    direct = O.actor_phase(actor, critic_after, la, _f(g["batch/obs"]), _f(g["noise/actor"]), target_entropy=-2.0,
                           trunk_branches=tb, **HP)
    swapped = ra32["regrad"](trunk_branches=tb)
    assert set(swapped) == set(direct["grads"]) and all(torch.equal(swapped[k], v) for k, v in direct["grads"].items())
    # the batch-chunked float64 conv is the plain one
    x = torch.randn(130, 3, 9, 11, dtype=torch.float64)
    w, bias = torch.randn(4, 3, 3, 3, dtype=torch.float64), torch.randn(4, dtype=torch.float64)
    assert torch.equal(O._conv2d(x, w, bias, 2), torch.nn.functional.conv2d(x, w, bias, stride=2))


def test_acting_path_matches_reference():
    g = load("tiny.npz")
    actor, critic, _, _, _ = _state(g)
    obs = O.center_crop(g["act/obs"], tuple(g["meta/out_hw"]))
    x = _f(obs)[None]
    mu, _, _, _ = O.actor_forward(actor, critic, x, None, compute_pi=False, compute_log_pi=False, **HP)
    assert_close(mu.flatten(), g["act/select"], 1e-5, "select_action")
    _, pi, _, _ = O.actor_forward(actor, critic, x, _f(g["act/noise"]), compute_log_pi=False, **HP)
    assert_close(pi.flatten(), g["act/sample"], 1e-5, "sample_action")


def test_full_shape_update_summaries():
    """84x84 -> 76x76 (BASELINE config-1 geometry): weights regenerated from
    the NumPy recipe, whole update() compared through per-tensor summaries."""
    from tests.golden_recipes import c1shape_inputs
    g = load("c1shape.npz")
    inp = c1shape_inputs(g)
    assert hashlib.sha256(inp["obs"].tobytes()).hexdigest() == str(g["batch/obs_sha256"])
    actor, critic, target, W, la = inp["actor"], inp["critic"], inp["target"], inp["W"], inp["log_alpha"]
    obs, nxt, pos = _f(inp["obs"]), _f(inp["next_obs"]), _f(inp["pos"])
    act, rew, nd = _f(g["batch/action"]), _f(g["batch/reward"]), _f(g["batch/not_done"])
    # One thread, set HERE (another test module imported into the same process may have raised the count since this
    # module's import): PyTorch's threaded fp32 CPU kernels are not run-to-run reproducible at this size -- the critic
    # loss, a mean of cancelling squares, moved by 2e-5 between two threaded runs -- while one thread is what the
    # fixture was recorded with.  So the bounds stay at the oracle's 1e-5 / 2e-5, not widened.
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        r = O.critic_phase(actor, critic, target, la, obs, act, rew, nxt, nd, _f(g["noise/critic"]), discount=0.99, **HP)
        assert_close(r["loss"], g["scalar/train_critic/loss"], 1e-5, "critic loss")
        for k in ("q1", "q2"):
            assert_close(summarize(r[k]), g[f"sum/critic/{k}"], 1e-5, k)
        for k, v in sub(g, "sum/critic/grad/", as_torch=False).items():
            assert_close(summarize(r["grads"][k]), v, 2e-5, "critic grad " + k)
        # chain the optimizer steps exactly as update() does to reach the later phases
        ag = inp["agent"]
        out = ag.update(obs, act, rew, nxt, nd, pos, _f(g["noise/critic"]), _f(g["noise/actor"]), step=0)
        assert_close(out["actor_loss"], g["scalar/train_actor/loss"], 2e-5, "actor loss")
        assert_close(out["alpha_loss"], g["scalar/train_alpha/loss"], 2e-5, "alpha loss")
        assert_close(out["curl_loss"], g["scalar/train/curl_loss"], 2e-5, "curl loss")
    finally:
        torch.set_num_threads(threads)


def _post_check(name, got, want, lr, what):
    """A parameter after the update against the fixture's (first POST_CLIP elements).  Adam's first step moves every
    element by lr * g / (|g| + eps): an element whose gradient is within rounding of zero may land 2 lr away
    (SURVEY.md D11).  So: (nearly) all elements to 1e-5 of the tensor's scale, a handful anywhere within 2.1 lr."""
    got = np.asarray(got.detach() if isinstance(got, torch.Tensor) else got, dtype=np.float64).ravel()[:len(want)]
    want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want)
    tight = 1e-5 * max(np.abs(want).max(), 1e-3)
    off = err > tight
    assert off.sum() <= max(2, 0.002 * err.size), f"{name} {what}: {off.sum()} of {err.size} elements off"
    assert err.max() <= 2.1 * lr + tight, f"{name} {what}: max error {err.max():.3e}"


MODE_NAMES = ("odd", "pixel_sac", "only_cpc", "detach", "l6c12", "thesis", "thesis_odd")


def _mode_case(name):
    from tests.golden_recipes import mode_inputs
    g = load(f"mode_{name}.npz")
    return g, mode_inputs(name, g)


def test_mode_fixtures_draw_order_and_bytes():
    """utils.py:147-182: with RandomCrop the draws are idxs, then (h1, w1) for obs, next_obs, pos; any other
    augmentation draws the indices only and ``pos`` is a copy of ``obs``."""
    import pytest  # noqa: F401
    for name in MODE_NAMES:
        g, inp = _mode_case(name)
        m = inp["m"]
        rs = np.random.RandomState(m["numpy_seed"])
        (ih, iw), (oh, ow) = m["in_hw"], m["out_hw"]
        idxs, offs = O.draw_sample_cpc_indices(m["n_fill"], m["batch"], ih - oh, iw - ow, random_crop=m["crop"], rng=rs)
        assert np.array_equal(idxs, g["rng/idxs"]), name
        assert int(g["rng/n_draws"]) == (7 if m["crop"] else 1)
        for (h1, w1), nm in zip(offs, ("obs", "next_obs", "pos")):
            assert np.array_equal(h1, g[f"rng/h1_{nm}"]) and np.array_equal(w1, g[f"rng/w1_{nm}"]), (name, nm)
        for nm in ("obs", "next_obs", "pos"):
            key = f"batch/{nm}_sha256"
            if key in g:
                assert hashlib.sha256(inp[nm].tobytes()).hexdigest() == str(g[key]), (name, nm)
        if not m["crop"]:
            assert np.array_equal(inp["pos"], inp["obs"])
        assert np.allclose(g["batch/action"], inp["acts"][idxs]) if "batch/action" in g else m["only_cpc"]


def _oracle_agent(inp):
    m = inp["m"]
    c, out_hw = m["channels"], tuple(m["out_hw"])
    ag = O.OracleAgent((c,) + out_hw, (2,), hidden_dim=m["hidden"], num_layers=m["num_layers"],
                       detach_encoder=m["detach_encoder"], pixel_sac=m["pixel_sac"])
    with torch.no_grad():
        for dst, src in ((ag.actor, inp["actor"]), (ag.critic, inp["critic"]), (ag.critic_target, inp["target"])):
            assert set(dst) == set(src)
            for k in dst:
                dst[k].copy_(src[k])
        ag.W.copy_(inp["W"])
    return ag


def test_mode_fixtures_match_the_oracle():
    """The branches of update() tiny.npz does not walk -- an odd step, pixel_sac, only_cpc, detach_encoder and the
    six-layer / 12-channel / identity-augmentation geometry -- each a whole reference update() from seeded weights
    and fresh optimizers: phase gradients and losses to 1e-5 / 2e-5, then the oracle agent's own chained update (its
    torch.optim.Adam steps, soft update) to the reference's post-update parameters."""
    for name in MODE_NAMES:
        g, inp = _mode_case(name)
        m = inp["m"]
        hp = dict(num_layers=m["num_layers"], log_std_min=-10, log_std_max=2)
        obs, nxt, pos = _f(inp["obs"]), _f(inp["next_obs"]), _f(inp["pos"])
        idxs = inp["idxs"]
        act, rew = _f(inp["acts"][idxs]), _f(inp["rews"][idxs])[:, None]
        nd = _f(1.0 - inp["dones"][idxs].astype(np.float32))[:, None]
        if "batch/reward" in g:
            assert np.array_equal(g["batch/reward"], rew.numpy()) and np.array_equal(g["batch/not_done"], nd.numpy())
        actor, critic, target, W, la = inp["actor"], inp["critic"], inp["target"], inp["W"], inp["log_alpha"]
        sac, curl, even = not m["only_cpc"], not m["pixel_sac"], m["step"] % 2 == 0
        # which phases ran in the reference: by what it recorded
        assert ("scalar/train_critic/loss" in g) == sac and ("scalar/train/curl_loss" in g) == curl, name
        assert ("scalar/train_actor/loss" in g) == (sac and even), name
        if sac:
            r = O.critic_phase(actor, critic, target, la, obs, act, rew, nxt, nd, _f(g["noise/critic"]), discount=0.99,
                               detach_encoder=m["detach_encoder"], **hp)
            assert_close(r["loss"], g["scalar/train_critic/loss"], 1e-5, name + " critic loss")
            for k in ("q1", "q2"):
                assert_close(r[k], g[f"critic/{k}"], 1e-5, name + " " + k)
            ref = sub(g, "critic/grad/")
            live = {k for k, v in r["grads"].items() if v is not None}
            assert set(ref) == live, name  # (detach_encoder: the convs have NO gradient, curl_sac.py:358)
            assert len(ref) == (4 + 6 * 2 + 0 if m["detach_encoder"] else 2 * m["num_layers"] + 4 + 12)
            for k, v in ref.items():
                assert_close(like(r["grads"][k], v), v, 1e-5, f"{name} critic grad {k}")
            for k, v in sub(g, "critic/gradsum/", as_torch=False).items():  # (tensors stored as a sample: the whole)
                assert_close(summarize(r["grads"][k]), v, 2e-5, f"{name} critic grad {k} (summary)")
            assert (len(sub(g, "critic/gradsum/")) > 0) == bool(m.get("unpatched")), name
        # the oracle agent's own chained update: later phases see the parameters its Adam steps produced
        ag = _oracle_agent(inp)
        nc = _f(g["noise/critic"]) if "noise/critic" in g else None
        na = _f(g["noise/actor"]) if "noise/actor" in g else None
        out = ag.update(obs, act, rew, nxt, nd, pos, nc, na, step=m["step"], only_cpc=m["only_cpc"])
        if sac and even:
            assert_close(out["actor_loss"], g["scalar/train_actor/loss"], 2e-5, name + " actor loss")
            assert_close(out["alpha_loss"], g["scalar/train_alpha/loss"], 2e-5, name + " alpha loss")
        if curl:
            assert_close(out["curl_loss"], g["scalar/train/curl_loss"], 2e-5, name + " curl loss")
        else:
            assert "curl_loss" not in out
        lr = 1e-3
        for tag, params in (("actor", ag.actor), ("critic", ag.critic), ("critic_target", ag.critic_target)):
            for k, want in sub(g, f"post/{tag}/", as_torch=False).items():
                if tag == "actor" and ".convs." in k:
                    got = ag.critic[k]  # tied (curl_sac.py:281)
                else:
                    got = params[k]
                _post_check(name, got, want, lr, f"post {tag}/{k}")
        _post_check(name, ag.W, g["post/W"].ravel(), lr, "post W")
        assert abs(float(ag.log_alpha.detach()) - float(g["post/log_alpha"])) <= 2.1e-4 * (1 if sac and even else 0) + 1e-12
        # what must NOT have moved, bit for bit
        same = lambda a, b: np.array_equal(np.asarray(a.detach()).ravel()[:len(b)], b)  # noqa: E731
        if not (sac and even):  # no actor phase, no target update
            for k, want in sub(g, "post/actor/", as_torch=False).items():
                if ".convs." not in k:
                    assert same(inp["actor"][k], want), (name, k)
            for k, want in sub(g, "post/critic_target/", as_torch=False).items():
                assert same(inp["target"][k], want), (name, k)
        if not sac:
            for k, want in sub(g, "post/critic/", as_torch=False).items():
                if k.startswith("Q"):
                    assert same(inp["critic"][k], want), (name, k)
        if not curl:
            assert same(inp["W"], g["post/W"].ravel())
        # the optimizers' step counts tell which tensors each Adam touched (curl_sac.py:299-313)
        n_enc = 2 * m["num_layers"] + 4
        want_steps = {"critic": [0, 0] if not sac else [(n_enc - 2 * m["num_layers"] if m["detach_encoder"] else n_enc) + 12, 1],
                      "actor": [10, 1] if sac and even else [0, 0], "alpha": [1, 1] if sac and even else [0, 0],
                      "encoder": [n_enc, 1] if curl else [0, 0], "cpc": [n_enc + 1, 1] if curl else [0, 0]}
        for k, v in want_steps.items():
            assert g[f"post/adam_steps/{k}"].tolist() == v, (name, k, g[f"post/adam_steps/{k}"].tolist(), v)


def test_noisy_cover_cover_logic_matches_reference():
    """The cover rows / colours / clamp of NoisyCover are the reference's own code (augmentations.py:185-203);
    the noise comes through a recorded stand-in for kornia's RandomGaussianNoise."""
    g = load("noisy_cover.npz")
    rs = np.random.RandomState(int(g["imgs_seed"]))
    imgs = rs.randint(0, 256, (5, 9, 34, 40), dtype=np.uint8)
    noise = torch.from_numpy(rs.randn(5, 9, 34, 40).astype(np.float32) * 10.0)
    np.random.seed(int(g["numpy_seed"]))
    colors = [np.random.randint(0, 255) for _ in range(3)]  # augmentations.py:188-190 draw order
    assert list(g["colors"]) == colors
    out = O.noisy_cover(torch.from_numpy(imgs).float(), colors, noise)
    assert abs(out.double().sum().item() - float(g["out_sum"])) <= 1e-6 * abs(float(g["out_sum"]))
    assert np.abs(out.numpy() - g["out"].astype(np.float32)).max() <= 0.13  # fixture stored as float16
    import curla_amd
    aug = curla_amd.NoisyCover((34, 40))
    assert (aug.top, aug.bottom) == (int(g["top"]), int(g["bottom"]))


def test_color_jiggle_restatement_properties():
    """PARITY UNPINNED (kornia): the restatement is only checked for self-consistency -- identity when not
    applied, HSV round trip, range, per-frame independence."""
    rs = np.random.RandomState(4)
    imgs = rs.randint(0, 256, (3, 9, 10, 12), dtype=np.uint8)
    params = torch.tensor([[0, 1.1, 1.2, 0.3]] * 9, dtype=torch.float32)
    out = O.color_jiggle(imgs, params, [0, 1, 2, 3])
    assert torch.allclose(out, torch.from_numpy(imgs).float(), atol=1e-4)
    x = torch.from_numpy(imgs[:, :3]).float() / 255
    h, s, v = O._rgb_to_hsv(x)
    assert torch.allclose(O._hsv_to_rgb(h, s, v), x, atol=1e-5)
    params = torch.tensor([[1, 1.0, 1.0, 0.0]] * 9, dtype=torch.float32)  # neutral factors
    assert torch.allclose(O.color_jiggle(imgs, params, [3, 2, 1, 0]), torch.from_numpy(imgs).float(), atol=1e-3)
    params = torch.tensor([[1, 1.2, 0.5, 2.0]] * 9, dtype=torch.float32)
    params[4, 0] = 0
    out = O.color_jiggle(imgs, params, [2, 0, 3, 1])
    assert out.min() >= 0 and out.max() <= 255.0001
    assert torch.allclose(out[1, 3:6], torch.from_numpy(imgs[1, 3:6]).float(), atol=1e-4)  # image 4 = sample 1, frame 1
