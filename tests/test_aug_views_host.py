"""``aug_views = 2`` on the host: the buffer's draw rule, the refusals of buffer and agent, the launches of
a views agent's phases under the launch-trace hook (as tests/test_update_launches_host.py records them), and the float64
reference of the two kernels (tests/_aug_views_ref.py) against torch's own mse_loss and cross_entropy."""
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import curla_amd
from tests import _aug_views_ref as V
from tests import _loss_head_ref as R
from tests.test_update_launches_host import Log, Recorder, make

C, IN_HW, OUT_HW, A, CAP, B = 9, (34, 40), (28, 34), 2, 32, 8


def _buffer(aug=None, batch=B, **kw):
    aug = aug or curla_amd.RandomCrop(IN_HW, OUT_HW)
    rb = curla_amd.ReplayBuffer((C,) + IN_HW, (A,), CAP, batch, "cpu", aug, **kw)
    rs = np.random.RandomState(3)
    for _ in range(20):
        f = rs.randint(0, 256, (C,) + IN_HW, dtype=np.uint8)
        rb.add(f, [0.1, -0.2], 0.5, f, False)
    return rb


# ------------------------------------------------------------------------------------------------------- 1. draw rule
@pytest.mark.parametrize("aug", ["crop", "cutout"])
def test_two_views_draw_half_the_rows_once_and_every_word_per_position(aug):
    make_aug = {"crop": lambda: curla_amd.RandomCrop(IN_HW, OUT_HW),
                "cutout": lambda: curla_amd.RandomCutout(IN_HW)}[aug]
    rb = _buffer(make_aug(), aug_views=2)
    seed = 11
    np.random.seed(seed)
    idxs, offs = rb.draw_indices()
    after = np.random.rand()
    np.random.seed(seed)
    want = np.tile(np.random.randint(0, rb.idx, B // 2), 2)
    words = [rb.augmentor.draw_index_words(B) for _ in range(3)]
    assert np.random.rand() == after  # the stream stands where the hand-made draws leave it
    assert idxs.shape == (B,) and np.array_equal(idxs, want) and np.array_equal(idxs[:B // 2], idxs[B // 2:])
    for j in range(3):
        for r, word in enumerate(words[j]):
            assert (offs[6 * (r // 2) + 2 * j + r % 2] == word).all(), (j, r)  # (a word may be one scalar)
    if aug == "crop":  # the two views of a transition are cropped independently
        for j in range(3):
            h1, w1 = offs[2 * j], offs[2 * j + 1]
            assert (h1[:B // 2] != h1[B // 2:]).any() and (w1[:B // 2] != w1[B // 2:]).any(), j


def test_one_view_is_the_buffer_without_the_keyword():
    plain, one = _buffer(), _buffer(aug_views=1)
    assert one.aug_views == 1 and plain.aug_views == 1 and _buffer(aug_views=2).aug_views == 2
    assert plain.block_layout() == one.block_layout() == _buffer(aug_views=2).block_layout()
    assert plain.graph_supported() == one.graph_supported()
    blocks = []
    for rb in (plain, one):
        np.random.seed(4)
        idxs, offs = rb.draw_indices()
        host = torch.zeros(rb.block_layout()["nbytes"], dtype=torch.uint8)
        rb._fill_index_block(host, idxs, offs)
        blocks.append((idxs, offs, host.numpy().tobytes(), np.random.rand()))
    assert np.array_equal(blocks[0][0], blocks[1][0]) and np.array_equal(blocks[0][1], blocks[1][1])
    assert blocks[0][2] == blocks[1][2] and blocks[0][3] == blocks[1][3]
    with pytest.raises(AttributeError):
        one.aug_views = 2  # fixed at construction


# --------------------------------------------------------------------------------------------------------- 2. refusals
@pytest.mark.parametrize("bad", [0, 3, 2.0, True, "2", None])
def test_only_the_ints_one_and_two_are_taken(bad):
    with pytest.raises(ValueError, match="aug_views"):
        _buffer(aug_views=bad)
    with pytest.raises(ValueError, match="aug_views"):
        curla_amd.CurlSacAgent((C,) + OUT_HW, (A,), "cpu", curla_amd.RandomCrop(IN_HW, OUT_HW), aug_views=bad)


def test_the_buffer_refuses_an_odd_batch_and_prioritized_rows():
    with pytest.raises(ValueError, match="even"):
        _buffer(batch=7, aug_views=2)
    with pytest.raises(ValueError, match="prioritized.*drawn on the device"):
        _buffer(aug_views=2, prioritized=True)
    _buffer(batch=7, aug_views=1)
    _buffer(aug_views=1, prioritized=True)


def test_the_agent_refuses_quantile_critics():
    aug = curla_amd.RandomCrop(IN_HW, OUT_HW)
    with pytest.raises(ValueError, match="critic_quantiles.*out of scope"):
        curla_amd.CurlSacAgent((C,) + OUT_HW, (A,), "cpu", aug, aug_views=2, critic_quantiles=5)


class _Foreign:
    """A buffer that says nothing about views: it counts as one view."""

    def sample_cpc(self):
        raise AssertionError("not reached")


@pytest.mark.parametrize("graphed", [False, True])
def test_agent_and_buffer_must_agree_in_both_directions(graphed):
    agent2, rb2 = make(dict(agent=dict(aug_views=2), rb=dict(aug_views=2)))
    agent1, rb1 = make({})
    for agent, rb in ((agent2, rb1), (agent1, rb2), (agent2, _Foreign())):
        check = (lambda: agent._update_graphed(rb, Log(), 1)) if graphed else (lambda: agent.update(rb, Log(), 1))
        with pytest.raises(ValueError, match="aug_views"):
            check()
    with pytest.raises(AssertionError, match="not reached"):
        agent1.update(_Foreign(), Log(), 1)


def test_graph_keys_grow_only_with_two_views():
    agent2, rb2 = make(dict(agent=dict(aug_views=2), rb=dict(aug_views=2)))
    agent1, rb1 = make(dict(agent=dict(aug_views=1), rb=dict(aug_views=1)))
    agent0, rb0 = make({})
    for agent, rb in ((agent2, rb2), (agent1, rb1), (agent0, rb0)):
        agent._graph_rb = rb
    assert agent1._graph_key() == agent0._graph_key() and agent1._graph_rb_key() == agent0._graph_rb_key()
    assert "aug_views" not in vars(agent1) and vars(agent1).keys() == vars(agent0).keys()
    assert agent2._graph_key()[len(agent0._graph_key()):] == (("aug_views", 2),)
    assert agent2._graph_rb_key() == agent0._graph_rb_key() + (("aug_views", 2),)
    assert agent2._graph_rb_key() in agent2._graph_key()  # (the buffer's entry, inside its key)


def test_a_checkpoint_carries_the_setting(tmp_path):
    agent2, _ = make(dict(agent=dict(aug_views=2), rb=dict(aug_views=2)))
    agent1, _ = make({})
    agent2.save_checkpoint(str(tmp_path / "two.pt"), 3)
    agent1.save_checkpoint(str(tmp_path / "one.pt"), 3)
    assert torch.load(str(tmp_path / "two.pt"), weights_only=False)["aug_views"] == 2
    assert "aug_views" not in torch.load(str(tmp_path / "one.pt"), weights_only=False)
    with pytest.warns(RuntimeWarning, match="aug_views = 2"):
        agent1.load_checkpoint(str(tmp_path / "two.pt"))
    with pytest.warns(RuntimeWarning, match="aug_views = 1"):
        agent2.load_checkpoint(str(tmp_path / "one.pt"))
    assert agent1.aug_views == 1 and agent2.aug_views == 2
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        agent2.load_checkpoint(str(tmp_path / "two.pt"))


# ----------------------------------------------------------------------------------------------------- 3. launch lists
def _lists(spec, steps=((4, False), (2, False), (1, False), (4, True))):
    agent, rb = make(spec)
    rec = Recorder(agent, rb)
    return [rec.run(lambda: agent.update(rb, Log(), step, only_cpc=only_cpc)) for step, only_cpc in steps]


def _names(calls):
    return [n for n, _ in calls]


@pytest.mark.parametrize("shape", ["b8", "b128"])
def test_a_views_agent_launches_the_two_kernels_in_their_phases(shape):
    views = dict(shape=shape, agent=dict(aug_views=2), rb=dict(aug_views=2))
    full, soft, critic, only_cpc = _lists(views)
    for calls in (full, soft, critic):  # the critic phase: the loss on its own, then the plain last-layer backward
        names = _names(calls)
        assert names.count("curla_critic_td_loss_views") == 1 and "curla_critic_td_loss" not in names
        at = names.index("curla_critic_td_loss_views")
        assert names[at + 1] in ("curla_mlp_out_bwd", "curla_mlp_out_bwd_bias")
    # the actor phase keeps its loss inside the backward launch: the one fused-loss launch of a full update is its
    assert _names(full).count("curla_mlp_out_bwd_loss") == 1
    assert "curla_mlp_out_bwd_loss" not in _names(soft) + _names(critic) + _names(only_cpc)
    for calls in (full, only_cpc):  # the CURL phase: the unfused head with the masked cross-entropy
        names = _names(calls)
        assert names.count("curla_curl_ce_views") == 1 and "curla_curl_ce" not in names and "curla_curl_head" not in names
    assert "curla_curl_ce_views" not in _names(soft) + _names(critic)
    plain = _lists(dict(shape=shape))
    assert "curla_mlp_out_bwd_loss" in _names(plain[2]) and "curla_critic_td_loss_views" not in _names(plain[0])
    assert ("curla_curl_head" in _names(plain[0])) == (shape == "b128")


@pytest.mark.parametrize("shape", ["b8", "b128"])
def test_one_view_launches_what_the_agent_without_the_keyword_launches(shape):
    assert _lists(dict(shape=shape, agent=dict(aug_views=1), rb=dict(aug_views=1))) == _lists(dict(shape=shape))


def test_one_view_has_the_workspace_of_the_agent_without_the_keyword():
    (a1, rb1), (a0, rb0) = make(dict(agent=dict(aug_views=1), rb=dict(aug_views=1))), make({})
    for agent, rb in ((a1, rb1), (a0, rb0)):
        Recorder(agent, rb).run(lambda: agent.update(rb, Log(), 4))
    shapes = lambda ws: {k: tuple(v.shape) for k, v in vars(ws).items() if torch.is_tensor(v)}  # noqa: E731
    assert shapes(a1._ws(B)) == shapes(a0._ws(B))
    for m1, m0 in ((a1.actor, a0.actor), (a1.critic, a0.critic), (a1.CURL, a0.CURL)):
        assert [(n, tuple(p.shape)) for n, p in m1.named_parameters()] == \
            [(n, tuple(p.shape)) for n, p in m0.named_parameters()]


# ---------------------------------------------------------------------------------- 4. the reference against torch
@pytest.mark.parametrize("Bn", [2, 4, 130])
def test_the_views_td_loss_reference_is_drqs_loss(Bn):
    d = R.loss_inputs(Bn, Bn, seed=Bn)
    H = Bn // 2
    tbar, Sbar = V.views_target(d["tq1"], d["tq2"], d["log_pi"], d["reward"], d["not_done"], d["log_alpha"], 0.99)
    assert torch.equal(tbar[:H], tbar[H:]) and torch.equal(Sbar[:H], Sbar[H:])
    t, _ = R.td_target(d["tq1"], d["tq2"], d["log_pi"], d["reward"], d["not_done"], d["log_alpha"], 0.99)
    assert torch.allclose(tbar[:H], (t[:H] + t[H:]) / 2, rtol=0, atol=1e-15)
    if Bn > 2:
        assert not torch.equal(t[:H], t[H:])  # (the two views' own targets differ: the mean is not either's)
    ref = V.views_critic_loss(d["q1"], d["q2"], tbar)
    q1, q2 = R.f64(d["q1"]).requires_grad_(True), R.f64(d["q2"]).requires_grad_(True)
    # DrQ: the critic loss of the first view plus the critic loss of the second, each two mse terms over H transitions
    loss = (F.mse_loss(q1[:H], tbar[:H]) + F.mse_loss(q2[:H], tbar[:H])) + \
        (F.mse_loss(q1[H:], tbar[H:]) + F.mse_loss(q2[H:], tbar[H:]))
    loss.backward()
    loss = float(loss.detach())
    assert abs(float(ref["loss"]) - loss) <= 1e-13 * abs(loss)
    assert torch.allclose(ref["dq"], torch.stack([q1.grad, q2.grad]), rtol=1e-13, atol=0)
    assert abs(float(ref["terms"].mean()) - loss) <= 1e-13 * abs(loss)
    # mirrored inputs: the plain loss's target, and (over half as many transitions) twice its gradient
    m = V.mirrored(d)
    tm, _ = V.views_target(m["tq1"], m["tq2"], m["log_pi"], m["reward"], m["not_done"], m["log_alpha"], 0.99)
    tp, _ = R.td_target(m["tq1"], m["tq2"], m["log_pi"], m["reward"], m["not_done"], m["log_alpha"], 0.99)
    assert torch.equal(tm, tp)
    assert torch.allclose(V.views_critic_loss(m["q1"], m["q2"], tm)["dq"], 2 * R.critic_loss(m["q1"], m["q2"], tp)["dq"],
                          rtol=1e-13, atol=0)


@pytest.mark.parametrize("Bn", [2, 4, 66])
def test_the_masked_infonce_reference_is_cross_entropy_without_the_partner_column(Bn):
    logits = torch.randn(Bn, Bn, generator=torch.Generator().manual_seed(Bn), dtype=torch.float64) * 3
    ref = V.curl_ce_views(logits)
    # an independent removal of the partner column: row a keeps columns in order, its own entry stays the label
    rows, labels = [], []
    for a in range(Bn):
        cols = [j for j in range(Bn) if j != (a + Bn // 2) % Bn]
        rows.append(logits[a, cols])
        labels.append(cols.index(a))
    small = torch.stack(rows).requires_grad_(True)
    assert small.shape == (Bn, Bn - 1)
    loss = F.cross_entropy(small, torch.tensor(labels))
    loss.backward()
    assert abs(float(ref["loss"]) - float(loss.detach())) <= 1e-13 * max(abs(float(loss.detach())), 1e-300)
    p = V.partner(Bn)
    assert bool((ref["dlogits"][torch.arange(Bn), p] == 0).all())
    for a in range(Bn):
        cols = [j for j in range(Bn) if j != (a + Bn // 2) % Bn]
        assert torch.allclose(ref["dlogits"][a, cols], small.grad[a], rtol=1e-12, atol=1e-18)
    # ... and what the plain InfoNCE gives on logits whose partner entries are -inf
    plain = R.curl_ce(V.masked(logits))
    assert torch.allclose(plain["row_loss"], ref["row_loss"], rtol=1e-12, atol=1e-14)
    assert torch.allclose(plain["dlogits"], ref["dlogits"], rtol=1e-12, atol=1e-18)
    b = V.curl_ce_views_bounds(logits)
    assert bool(torch.isfinite(b["row_loss"]).all()) and bool(torch.isfinite(b["dlogits"]).all())
