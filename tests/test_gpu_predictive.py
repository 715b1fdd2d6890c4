"""CurlSacAgent(cpc_objective="predictive") on the MI355X: one representation phase against autograd through
the differentiable modules, whole updates eager against graph-replayed and across a checkpoint, the objective beside the
other options, reset_networks() and two live data-parallel ranks.  The tiny geometry of the other agent tests
(tests/test_gpu_critic_ln.py's helpers), B = 8."""
import os
import traceback

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _pred_ref as R
from tests.test_gpu_critic_ln import HP, IN_HW, OUT_HW, NullLogger, _grads_of, _ring, _state_of, check

pytestmark = pytest.mark.gpu

B, HIDDEN, FEAT, A = 8, 96, 50, 2


def make_agent(seed=0, **kw):
    import curla_amd
    aug = curla_amd.RandomCrop(IN_HW, OUT_HW)
    torch.manual_seed(seed)
    agent = curla_amd.CurlSacAgent((9,) + OUT_HW, (A,), torch.device("cuda"), aug, hidden_dim=HIDDEN,
                                   cpc_objective="predictive", **{**HP, **kw})
    return agent, aug


def ring(aug, **kw):
    return _ring(aug, B=B, **{"pos_offset": 1, **kw})


def predictor_state(agent):
    return {k: v.detach().clone() for k, v in agent.CURL.predictor.state_dict().items()}


def moved(before, agent):
    now = agent.CURL.predictor.state_dict()
    return all(not torch.equal(before[k], now[k]) for k in before)


# ------------------------------------------------------------------------------------- 1. one phase against autograd
def test_one_cpc_phase_against_autograd_through_the_differentiable_modules():
    """update_cpc's gradients -- the encoder's twelve tensors and the predictor's four, as the phase left them in the flat
    gradient buffer -- against loss.backward() of the same loss built from agent.critic.encoder(obs) (autograd.py), torch
    Linears over the predictor's own parameters and tests/_pred_ref.py's loss in float32; the tolerance is the one
    tests/test_gpu_hlg.py holds its autograd comparison to (RTOL per tensor: two float32 evaluations in different
    orders).  Then the same phase with its optimizer steps: CURL.W has a zero gradient and is bitwise where it was, the
    Q functions, the target and the actor are untouched, the encoder and the predictor have moved."""
    np.random.seed(2)
    agent, aug = make_agent(seed=2, predictor_hidden=40)
    rb = ring(aug)
    obs, act, rew, nxt, nd, kw = rb.sample_cpc()
    anchor, pos = kw["obs_anchor"], kw["obs_pos"]
    pred, enc = agent.CURL.predictor, agent.critic.encoder
    assert pred[0].weight.shape == (40, FEAT + A) and pred[0].weight.is_cuda
    agent.encoder_optimizer.step = agent.cpc_optimizer.step = lambda: None  # the gradients, before Adam consumes them
    L = NullLogger()
    agent.update_cpc(anchor, pos, kw, L, 1, action=act)
    torch.cuda.synchronize()
    got = {k: v for k, v in _grads_of(agent.critic).items() if k.startswith("encoder.")}
    got_pred = {k: p.grad.detach().cpu().clone() for k, p in pred.named_parameters()}
    assert not bool(agent.CURL.W.grad.any())
    for k, v in _grads_of(agent.critic).items():
        if not k.startswith("encoder."):
            assert not bool(v.any()), k  # (the Q functions receive nothing)

    agent.encoder_optimizer.zero_grad()
    agent.cpc_optimizer.zero_grad()
    z = enc(anchor)
    with torch.no_grad():
        zt = agent.critic_target.encoder(pos)
    assert z.requires_grad and not zt.requires_grad
    h = F.relu(F.linear(torch.cat([z, act], 1), pred[0].weight, pred[0].bias))
    loss = R.loss_of(F.linear(h, pred[2].weight, pred[2].bias), zt)
    loss.backward()
    torch.cuda.synchronize()
    want = {k: v for k, v in _grads_of(agent.critic).items() if k.startswith("encoder.")}
    assert set(got) == set(want) and len(want) == 12
    check("predictive phase loss", L.scalars["train/pred_loss"], float(loss.detach()))
    for k in want:
        check(f"predictive phase grad {k}", got[k], want[k])
    for k, p in pred.named_parameters():
        assert p.grad.data_ptr() == agent._critic_gflat.data_ptr() + (p.data_ptr() - agent._critic_flat.data_ptr())
        check(f"predictive phase grad predictor.{k}", got_pred[k], p.grad)
    ws = agent._ws(B)
    rows, total, dp = R.loss(ws.p_out.cpu(), ws.z_pos.cpu())  # the kernel inside the phase, on the phase's own tensors
    check("predictive phase row losses", ws.row_loss, rows)
    check("predictive phase dp", ws.p_dout, dp)

    # the phase with its steps
    del agent.encoder_optimizer.step, agent.cpc_optimizer.step
    lay = agent._lay
    before = agent._critic_flat.clone(), agent._target_flat.clone(), agent._actor_flat.clone(), predictor_state(agent)
    agent.update_cpc(anchor, pos, kw, L, 1, action=act)
    torch.cuda.synchronize()
    flat, (w0, w1), (e0, e1) = agent._critic_flat, lay["w"], lay["enc"]
    n_w = agent.CURL.W.numel()
    assert torch.equal(flat[:n_w], before[0][:n_w]) and not bool(agent.CURL.W.grad.any())  # W: same bits, zero gradient
    assert torch.equal(flat[e1:], before[0][e1:])  # Q1 | Q2
    assert torch.equal(agent._target_flat, before[1]) and torch.equal(agent._actor_flat, before[2])
    assert not torch.equal(flat[e0:e1], before[0][e0:e1]) and moved(before[3], agent)
    assert bool(torch.isfinite(flat).all())


# ------------------------------------------------------------------------------ 2. whole updates: graphs, checkpoints
SAME_KIND = dict(actor_update_freq=1, critic_target_update_freq=1, cpc_update_freq=1, log_interval=5)


def _run(graphs, steps=range(1, 6)):
    np.random.seed(11)
    torch.manual_seed(11)
    torch.cuda.manual_seed_all(11)
    agent, aug = make_agent(seed=11, **SAME_KIND)
    rb = ring(aug)
    if graphs:
        agent.enable_update_graphs(rb, warm=1, depth=2)
    L = NullLogger()
    for step in steps:  # 1: eager (warm); 2, 3: captured (two blocks) and replayed; 4: replayed; 5: a logging step, eager
        agent.update(rb, L, step)
    torch.cuda.synchronize()
    return agent, _state_of(agent), dict(L.scalars)


def test_update_graphs_replay_predictive_updates_bit_identically():
    _, eager, logged_e = _run(False)
    agent, graphed, logged_g = _run(True)
    assert len(agent._graphs) == 1 and all(st["graph"] is not None for r in agent._graphs.values() for st in r)
    assert agent._graph_key_at_capture[-1] == ("cpc", "predictive", HIDDEN)
    assert set(eager) == set(graphed) and len(eager) > 20
    for k, v in eager.items():
        assert torch.equal(v, graphed[k]), k
    assert logged_e == logged_g and np.isfinite(logged_e["train/pred_loss"]) and "train/curl_loss" not in logged_e
    assert any(k.startswith("cpc.") and k.endswith("exp_avg") and bool(v.any()) for k, v in eager.items())


def test_a_checkpoint_resumes_bit_for_bit(tmp_path):
    np.random.seed(5)
    agent, aug = make_agent(seed=5)
    rb, L = ring(aug), NullLogger()
    agent.update(rb, L, 0)
    ck = str(tmp_path / "pred.pt")
    agent.save_checkpoint(ck, 1)
    for step in (1, 2):
        agent.update(rb, L, step)
    torch.cuda.synchronize()
    want, logged = _state_of(agent), dict(L.scalars)

    np.random.seed(99)  # another process state: everything must come from the file
    other, aug2 = make_agent(seed=99)
    rb2, L2 = ring(aug2), NullLogger()
    assert other.load_checkpoint(ck) == 1
    for step in (1, 2):
        other.update(rb2, L2, step)
    torch.cuda.synchronize()
    got = _state_of(other)
    assert set(got) == set(want)
    for k, v in want.items():
        assert torch.equal(v, got[k]), k
    assert L2.scalars["train/pred_loss"] == logged["train/pred_loss"]
    import curla_amd
    torch.manual_seed(0)
    plain = curla_amd.CurlSacAgent((9,) + OUT_HW, (A,), torch.device("cuda"), aug, hidden_dim=HIDDEN, **HP)
    flat = plain._critic_flat.clone()
    with pytest.raises(ValueError, match="cpc_objective"):
        plain.load_checkpoint(ck)
    assert torch.equal(plain._critic_flat, flat)


# ------------------------------------------------------------------------------------------- 3. beside the other options
COMBINATIONS = [
    ("aug_views", dict(aug_views=2), dict(aug_views=2)),
    ("n_step", {}, dict(n_step=3, discount=HP["discount"])),
    ("utd_ratio", dict(utd_ratio=2), {}),
    ("critic_bins", dict(critic_bins=51, critic_value_range=(-5.0, 5.0)), {}),
    ("deterministic policy", dict(policy="deterministic"), {}),
    ("weight_decay", dict(weight_decay=1e-2), {}),
    ("max_grad_norm", {}, {}),
]


@pytest.mark.parametrize("name,agent_kw,rb_kw", COMBINATIONS, ids=[c[0] for c in COMBINATIONS])
def test_the_objective_beside_the_other_options(name, agent_kw, rb_kw):
    np.random.seed(3)
    agent, aug = make_agent(seed=3, **agent_kw)
    if name == "max_grad_norm":
        agent.set_max_grad_norm(1e-3)
    rb, L = ring(aug, **rb_kw), NullLogger()
    before, w = predictor_state(agent), agent.CURL.W.detach().clone()
    for step in (0, 1):
        agent.update(rb, L, step)
    torch.cuda.synchronize()
    assert np.isfinite(L.scalars["train/pred_loss"]) and 0.0 <= L.scalars["train/pred_loss"] <= 4.0
    assert moved(before, agent) and bool(torch.isfinite(agent._critic_flat).all())
    assert torch.equal(agent.CURL.W, w)  # (never stepped -- nor decayed)
    if name == "max_grad_norm":
        assert np.isfinite(L.scalars["train/curl_grad_norm"]) and float(agent.grad_clip_stats[2, 1]) < 1.0
    if name == "weight_decay":
        assert agent.cpc_optimizer.param_groups[0]["weight_decay"] == 1e-2


def test_update_refuses_a_buffer_without_temporal_positives():
    agent, aug = make_agent()
    flat = agent._critic_flat.clone()
    for kw in (dict(pos_offset=0), dict(pos_offset=2)):
        with pytest.raises(ValueError, match="pos_offset"):
            agent.update(ring(aug, **kw), NullLogger(), 1)
    assert torch.equal(agent._critic_flat, flat)


# ------------------------------------------------------------------------------------------------------------ 4. resets
def test_reset_networks_treats_the_predictor_as_it_treats_w():
    np.random.seed(7)
    agent, aug = make_agent(seed=7)
    rb, L = ring(aug), NullLogger()
    for step in range(2):
        agent.update(rb, L, step)
    w0, w1 = agent._lay["w"]
    old = agent._critic_flat[w0:w1].clone()
    keep = 0.25
    agent.reset_networks(encoder_keep=keep)
    torch.cuda.synchronize()
    fresh = agent._reset_stage["critic"]["host"][w0:w1].cuda()
    new = agent._critic_flat[w0:w1]
    n_w = agent.CURL.W.numel()
    assert not torch.equal(new[:n_w], old[:n_w]) and not torch.equal(new[n_w:], old[n_w:])
    # shrink and perturb, three float32 operations per element: W and the predictor by the same rule, the same keep
    check("reset W group", new, keep * old.double() + (1 - keep) * fresh.double(), 1e-6)
    assert not bool(agent.cpc_optimizer._m.any()) and set(agent.cpc_optimizer._steps) == {0}
    assert not bool(agent._critic_gflat.any())
    for step in range(2, 4):
        agent.update(rb, L, step)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(agent._critic_flat).all()) and np.isfinite(L.scalars["train/pred_loss"])


# ------------------------------------------------------------------------------------------------- 5. two live ranks
def _dp_train(rank, world, overlap, steps=3):
    import curla_amd
    import torch.distributed as dist
    from tests import test_gpu_dp2 as D
    dev = torch.device("cuda", 0)
    curla_amd.set_seed_everywhere(1 + rank)  # the ranks start from different parameters
    aug = curla_amd.RandomCrop(D.IN_HW, D.OUT_HW)
    agent = curla_amd.CurlSacAgent((9,) + D.OUT_HW, (2,), dev, aug, hidden_dim=D.HIDDEN, cpc_objective="predictive", **D.HP)
    rb = curla_amd.ReplayBuffer((9,) + D.IN_HW, (2,), D.CAPACITY // world, D.B, dev, aug, pos_offset=1)
    agent.enable_data_parallel(overlap=overlap, check_every=1)  # check_replicas() on every update: raises on drift
    D._fill(rb, D._shard_data(rank))
    curla_amd.set_seed_everywhere(11 + rank)
    sizes, real = [], dist.all_reduce

    def spy(t, *a, **k):
        sizes.append(int(t.numel()))
        return real(t, *a, **k)
    dist.all_reduce = spy
    try:
        L = D._Log()
        for step in range(steps):
            agent.update(rb, L, step)
        torch.cuda.synchronize()
        agent.check_replicas()
    finally:
        dist.all_reduce = real
    return dict(bits=D._replica_bits(agent), sizes=sizes, lay=dict(agent._lay), losses=dict(L.s),
                w_grad=agent.CURL.W.grad.detach().cpu().clone())


def _dp_worker(rank, world, port, out_dir):
    """Entry point of a rank (a fresh ``spawn`` process, as tests/test_gpu_dp2.py's)."""
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
        torch.cuda.set_device(0)
        out = dict(blocking=_dp_train(rank, world, False), overlapped=_dp_train(rank, world, True))
        torch.save(out, os.path.join(out_dir, f"rank{rank}.pt"))
        dist.barrier()
        dist.destroy_process_group()
    except BaseException:
        with open(os.path.join(out_dir, f"rank{rank}.err"), "w") as f:
            f.write(traceback.format_exc())
        raise


def test_two_live_ranks_stay_bitwise_replicas(tmp_path):
    """Two ranks on the one GPU in the manner of tests/test_gpu_dp2.py (fresh spawn processes over a gloo group, own
    shards, different initial parameters): after three updates under either schedule the replicas are bit-identical,
    predictor included -- the cpc bucket [W group | encoder] covers it with nothing added."""
    import torch.multiprocessing as mp
    from tests import test_gpu_dp2 as D
    out_dir, world = str(tmp_path), 2
    port = D._free_port()
    procs = [mp.get_context("spawn").Process(target=_dp_worker, args=(r, world, port, out_dir)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
    errs = []
    for r, p in enumerate(procs):
        if p.is_alive():
            p.kill()
            errs.append(f"rank {r}: still running after 300 s")
        path = os.path.join(out_dir, f"rank{r}.err")
        if os.path.exists(path):
            errs.append(f"rank {r}:\n" + open(path).read())
        elif p.exitcode != 0:
            errs.append(f"rank {r}: exit code {p.exitcode}")
    assert not errs, "\n".join(errs)
    r0, r1 = (torch.load(os.path.join(out_dir, f"rank{r}.pt"), weights_only=False) for r in range(world))
    for schedule in ("blocking", "overlapped"):
        a, b = r0[schedule], r1[schedule]
        assert a["bits"].keys() == b["bits"].keys()
        for k in a["bits"]:
            assert torch.equal(a["bits"][k], b["bits"][k]), f"{schedule}: ranks differ in {k}"
            assert torch.equal(a["bits"][k], r0["blocking"]["bits"][k]), f"the schedules differ in {k}"
        lay = a["lay"]
        assert lay["w"][1] >= FEAT * FEAT + D.HIDDEN * (FEAT + 2) + D.HIDDEN + FEAT * D.HIDDEN + FEAT  # (W | predictor)
        assert bool(torch.isfinite(a["bits"]["critic"]).all()) and not bool(a["w_grad"].any())
        assert a["losses"] != b["losses"] and np.isfinite(a["losses"]["train/pred_loss"])
        assert bool(a["bits"]["m/cpc"][:lay["w"][1] - FEAT * FEAT].any())  # (the predictor's moments: it was stepped)
    # blocking schedule: the cpc phase's ONE all-reduce is the bucket [W group | encoder], predictor inside
    assert r0["blocking"]["lay"]["enc"][1] in r0["blocking"]["sizes"]
