"""Clipping by the global gradient norm inside the flat Adam launches (``FlatAdam(max_grad_norm=...)``,
``CurlSacAgent.set_max_grad_norm``) on the MI355X: the semantics of ``torch.nn.utils.clip_grad_norm_(params, max_norm)``
right in front of the optimizer's step, with the norm taken by ``curla_grad_sqsum`` in float64 and the coefficient
applied by the ``curla_adam_step*_clip`` launch that follows.

Adam's FIRST step does not see the gradient's scale (m / sqrt(v) is +-1), so every parity test here takes at least three
steps with norms that differ from step to step, or compares the moments, which scale with coef and coef^2.

Bounds.  The norm: the squares are exact in double and their sum of n <= 2^22 terms is good to n 2^-53 (5e-10), so the
device's double norm and NumPy's agree far inside half a float32 ulp and their float32 roundings are at most 1 ulp apart;
the same for the coefficient, one division and one rounding later.  Steps: the 2e-6 that
``test_gpu_kernels.test_flat_adam_matches_torch_adam`` holds the unclipped step to (the reference is fed the gradient the
test clipped itself).  Everything else is bit for bit."""
import functools

import numpy as np
import pytest
import torch

from tests._util import rel_err
from tests.test_gpu_kernels import _flat_params

pytestmark = pytest.mark.gpu


def check(name, got, ref, tol):
    e = rel_err(got, ref)
    print(f"{name}: rel err {e:.3e} (bound {tol:.1e})")
    assert np.isfinite(e) and e <= tol, f"{name}: rel err {e:.3e} > {tol:.1e}"


def within_ulps(got, want, ulps=1):
    """|got - want| <= ulps float32 ulps of want, element by element."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    return bool(np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <=
                       ulps * np.spacing(np.abs(want)).astype(np.float64)))


def norm_and_coef(grads, max_norm):
    """clip_grad_norm_'s two numbers from float32 gradients, in float64, each rounded to float32 once."""
    total = sum(float(np.sum(np.square(np.asarray(g, dtype=np.float64)))) for g in grads)
    norm = float(np.sqrt(total))
    return np.float32(norm), np.float32(min(1.0, max_norm / (norm + 1e-6))), norm


def _flat_params_shifted(sizes, shift, seed=0):
    """_flat_params' layout on buffers that start ``shift`` floats behind a 16-byte boundary: the runs are 4-byte but
    not 16-byte aligned, as the actor's run inside its bucket."""
    total = sum((int(np.prod(n)) + 3) & ~3 for n in sizes)
    g = torch.Generator().manual_seed(seed)
    flat = torch.zeros(total + 4, device="cuda")[shift:shift + total]
    gflat = torch.zeros(total + 4, device="cuda")[shift:shift + total]
    assert flat.data_ptr() % 16 == 4 * shift and gflat.data_ptr() % 16 == 4 * shift
    params, off = [], 0
    for n in sizes:
        cnt = int(np.prod(n))
        flat[off:off + cnt] = torch.randn(cnt, generator=g).cuda()
        p = torch.nn.Parameter(flat[off:off + cnt].view(n))
        p.grad = gflat[off:off + cnt].view(n)
        params.append(p)
        off += (cnt + 3) & ~3
    return flat, gflat, params


# run length -> (sizes, shift of the buffers in floats, index of a parameter that loses its gradient)
NORM_CASES = {
    "n1": ([(1,)], 0, None),
    "n7_tail_only": ([(4,), (3,)], 0, None),
    "n255": ([(100,), (155,)], 0, None),
    "n1027_off_16_bytes": ([(512,), (512,), (3,)], 1, None),
    "n300001_loop_wraps": ([(65536,), (200000,), (34465,)], 0, None),
    "two_runs": ([(1027,), (33,), (300,), (2, 50)], 0, 1),
}


@pytest.mark.parametrize("case", list(NORM_CASES))
def test_norm_and_coefficient(case):
    from curla_amd.optim import FlatAdam
    sizes, shift, lost = NORM_CASES[case]
    flat, gflat, params = _flat_params_shifted(sizes, shift) if shift else _flat_params(sizes, "cuda")
    run = sum(int(np.prod(n)) for n in sizes)
    if case.startswith("n") and lost is None:
        assert str(run) == case[1:].split("_")[0]  # the padded slots add up to the run the case is named after
    gen = torch.Generator().manual_seed(21)
    grads = [torch.randn(p.shape, generator=gen) * 10.0 ** (i % 7 - 4) for i, p in enumerate(params)]
    for p, g in zip(params, grads):
        p.grad.copy_(g.cuda())
    if lost is not None:
        params[lost].grad = None
    live = [g.numpy() for i, g in enumerate(grads) if i != lost]
    _, _, norm64 = norm_and_coef(live, 1.0)
    opt = FlatAdam(params, flat, gflat, lr=1e-3)
    for max_norm in (0.37 * norm64, 2.0 * norm64, float("inf")):
        opt.max_grad_norm = max_norm
        for p, g in zip(params, grads):  # (the previous round wrote the clipped gradient back)
            if p.grad is not None:
                p.grad.copy_(g.cuda())
        opt.step()
        want_norm, want_coef, _ = norm_and_coef(live, max_norm)
        got = opt.clip_stats.cpu().numpy()
        print(f"{case} max_norm {max_norm:.6g}: norm {got[0]!r} (float64 {want_norm!r}), coef {got[1]!r} ({want_coef!r})")
        assert within_ulps(got[0], want_norm) and within_ulps(got[1], want_coef), (got, want_norm, want_coef)
        assert (got[1] < 1.0) == (max_norm < norm64)
    assert bool(torch.isfinite(flat).all())


def test_zero_gradient_is_norm_zero_coefficient_one_and_no_nan():
    from curla_amd.optim import FlatAdam
    flat, gflat, params = _flat_params([(300, 7), (5,), (1027,)], "cuda")
    before = flat.clone()
    opt = FlatAdam(params, flat, gflat, lr=1e-3, max_grad_norm=0.5)
    opt.clip_stats.fill_(float("nan"))
    for _ in range(2):
        opt.step()
    assert opt.clip_stats.tolist() == [0.0, 1.0]
    for t in (flat, gflat, opt._m, opt._v):
        assert bool(torch.isfinite(t).all())
    assert torch.equal(flat, before) and float(gflat.abs().sum()) == 0.0  # (m = 0: Adam's update is 0 / eps)


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.5, 0.999)])
def test_clipped_steps_match_torch_adam_fed_the_clipped_gradient(betas):
    """5 steps of FlatAdam(max_grad_norm=m) against torch.optim.Adam on the CPU fed g * coef, the coefficient computed
    here from the float64 norm.  The gradient's scale changes from step to step so that some steps clip and others do
    not; one parameter loses its gradient on steps 2 and 3 (a step over two runs, ONE norm over both) and the optimizer
    is rebuilt from its state_dict() after step 3.  The flat gradient buffer afterwards holds g * coef -- g itself, bit
    for bit, where coef = 1.  (Fails without the feature: FlatAdam takes no max_grad_norm.)"""
    from curla_amd.optim import FlatAdam
    sizes = [(32, 9, 3, 3), (32,), (50, 1203), (50,), (1,), (1024, 57), (7,)]
    max_norm, scales = 50.0, [1.0, 0.01, 1.0, 0.003, 3.0]
    flat, gflat, params = _flat_params(sizes, "cuda")
    ref_params = [torch.nn.Parameter(p.detach().cpu().clone()) for p in params]
    opt = FlatAdam(params, flat, gflat, lr=1e-3, betas=betas, max_grad_norm=max_norm)
    ref = torch.optim.Adam(ref_params, lr=1e-3, betas=betas)
    gen = torch.Generator().manual_seed(5)
    saved = params[2].grad
    coefs = []
    for step, scale in enumerate(scales):
        skip = step in (2, 3)
        grads = [torch.randn(p.shape, generator=gen) * (10.0 ** (i % 3 - 2) * scale) for i, p in enumerate(params)]
        live = [i for i in range(len(params)) if not (skip and i == 2)]
        want_norm, coef, _ = norm_and_coef([grads[i].numpy() for i in live], max_norm)
        coefs.append(float(coef))
        params[2].grad = None if skip else saved
        for i, (p, r) in enumerate(zip(params, ref_params)):
            if i in live:
                p.grad.copy_(grads[i].cuda())
                r.grad = grads[i] * torch.tensor(coef)  # float32 product: one rounding per element
            else:
                r.grad = None
        untouched = saved.clone()
        opt.step()
        ref.step()
        got = opt.clip_stats.cpu().numpy()
        print(f"step {step}: norm {got[0]!r} (float64 {want_norm!r}), coef {got[1]!r} ({coef!r})")
        assert within_ulps(got[0], want_norm) and within_ulps(got[1], coef)
        for i in live:
            if coef == 1.0:
                assert torch.equal(params[i].grad.cpu(), grads[i]), (step, i)
            else:
                assert within_ulps(params[i].grad.cpu().numpy(), ref_params[i].grad.numpy()), (step, i)
        if skip:
            assert torch.equal(saved, untouched)  # a parameter without a gradient: its slot is not scaled
        if step == 3:  # a resumed optimizer continues identically (the threshold is not state: given again)
            sd = opt.state_dict()
            opt = FlatAdam(params, flat, gflat, lr=1e-3, betas=betas, max_grad_norm=max_norm)
            opt.load_state_dict(sd)
    assert any(c < 1.0 for c in coefs) and any(c == 1.0 for c in coefs), coefs
    torch.cuda.synchronize()
    for i, (p, r) in enumerate(zip(params, ref_params)):
        check(f"clipped flat_adam{betas} param{i}", p.detach(), r.detach(), 2e-6)
        st, rst = opt.state[p], ref.state[r]
        check(f"clipped flat_adam{betas} exp_avg{i}", st["exp_avg"], rst["exp_avg"], 2e-6)
        check(f"clipped flat_adam{betas} exp_avg_sq{i}", st["exp_avg_sq"], rst["exp_avg_sq"], 2e-6)
    sd, rsd = opt.state_dict(), ref.state_dict()
    assert sd["param_groups"][0].keys() == rsd["param_groups"][0].keys()
    for k in sd["state"]:
        assert float(sd["state"][k]["step"]) == float(rsd["state"][k]["step"])


def _three_steps(max_grad_norm, sizes=((32, 9, 3, 3), (32,), (50, 1203), (50,), (1,), (300, 57), (7,)), lost=None):
    from curla_amd.optim import FlatAdam
    flat, gflat, params = _flat_params(list(sizes), "cuda", seed=4)
    opt = FlatAdam(params, flat, gflat, lr=1e-3, max_grad_norm=max_grad_norm)
    gen = torch.Generator().manual_seed(17)
    if lost is not None:
        params[lost].grad = None
    stats = []
    for scale in (1.0, 0.1, 3.0):
        gflat.copy_(torch.randn(gflat.shape, generator=gen).cuda() * scale)
        opt.step()
        if max_grad_norm is not None:
            stats.append(opt.clip_stats.clone())
    torch.cuda.synchronize()
    return (flat.clone(), opt._m.clone(), opt._v.clone(), gflat.clone()), stats


def test_inactive_clipping_has_no_side_effects():
    """max_grad_norm = inf, and a finite value above every norm, leave parameters, moments and the gradient buffer
    exactly as the unclipped run does."""
    plain, _ = _three_steps(None)
    for m in (float("inf"), 1e6):
        got, stats = _three_steps(m)
        assert all(float(s[1]) == 1.0 and 10.0 < float(s[0]) < 1e6 for s in stats), stats
        for a, b in zip(plain, got):
            assert torch.equal(a, b)


@pytest.mark.parametrize("lost", [None, 2])
def test_same_bytes_same_result(lost):
    """Determinism: the same gradient bytes stepped from the same state give the same bits and the same stats (one run
    of 80 000 elements over many blocks; a step over two runs)."""
    a, sa = _three_steps(40.0, lost=lost)
    b, sb = _three_steps(40.0, lost=lost)
    assert any(float(s[1]) < 1.0 for s in sa)
    for x, y in zip(a + tuple(sa), b + tuple(sb)):
        assert torch.equal(x, y)
    plain, _ = _three_steps(None, lost=lost)
    assert not torch.equal(plain[1], a[1])  # (clipping acted)


def _scaled_reference(gflat, coef):
    """g <- coef * g where coef != 1, as one float32 product per element (what the clipping launch writes back)."""
    if float(coef) != 1.0:
        gflat.mul_(coef)


def test_step_pair_clips_once_fused_or_not():
    """With clipping active, FlatAdam.step_pair's one launch, its two separate steps (one square-sum over
    [W | encoder], encoder_optimizer's clipped step, cpc_optimizer's step with the same coefficient and no second
    scaling) and the plain statement -- scale the gradient once by the coefficient, then the two UNCLIPPED steps -- end
    with the same parameters, moments and step counts, bit for bit."""
    from curla_amd.optim import FlatAdam
    sizes = [(50, 50), (32, 9, 3, 3), (32,), (50, 1203), (50,)]
    res, coefs = [], []
    for how in ("fused", "separate", "by hand"):
        flat, gflat, params = _flat_params(sizes, "cuda", seed=3)
        m = None if how == "by hand" else 0.5
        enc = FlatAdam(params[1:], flat, gflat, lr=1e-3, max_grad_norm=m)
        cpc = FlatAdam(params, flat, gflat, lr=2e-3, betas=(0.8, 0.99), max_grad_norm=m)
        gen = torch.Generator().manual_seed(9)
        for k in range(3):
            gflat.copy_(torch.randn(gflat.shape, generator=gen).cuda() * 0.01 * (k + 1))
            if how == "fused":
                FlatAdam.step_pair(enc, cpc)
                coefs.append(cpc.clip_stats.clone())
            elif how == "separate":
                FlatAdam._two_steps(enc, cpc)
                assert torch.equal(cpc.clip_stats, coefs[k])
            else:
                _scaled_reference(gflat[cpc._lo:cpc._hi], coefs[k][1])  # cpc's run, [W | encoder]
                enc.step()
                cpc.step()
        torch.cuda.synchronize()
        res.append((flat.clone(), enc._m.clone(), enc._v.clone(), cpc._m.clone(), cpc._v.clone(), gflat.clone(),
                    list(enc._steps), list(cpc._steps)))
    assert all(float(c[1]) < 1.0 for c in coefs), coefs
    for other in res[1:]:
        for a, b in zip(res[0][:6], other[:6]):
            assert torch.equal(a, b)
        assert res[0][6:] == other[6:] == ([3] * 4, [3] * 5)


def test_step_pair_with_a_replaced_step_still_clips_once():
    """A ``step`` replaced on the instance (how a test looks at the gradient before it is consumed) sends step_pair to
    the separate steps: still one norm over [W | encoder] and one scaling per element."""
    from curla_amd.optim import FlatAdam
    sizes = [(50, 50), (32, 9, 3, 3), (32,), (50, 1203), (50,)]
    res = []
    for replaced in (False, True):
        flat, gflat, params = _flat_params(sizes, "cuda", seed=3)
        enc = FlatAdam(params[1:], flat, gflat, lr=1e-3, max_grad_norm=0.5)
        cpc = FlatAdam(params, flat, gflat, lr=2e-3, betas=(0.8, 0.99), max_grad_norm=0.5)
        seen = []
        if replaced:
            def step(closure=None, cpc=cpc):
                seen.append(gflat.clone())
                return FlatAdam.step(cpc)
            cpc.step = step
        gen = torch.Generator().manual_seed(9)
        for k in range(3):
            gflat.copy_(torch.randn(gflat.shape, generator=gen).cuda() * 0.01 * (k + 1))
            FlatAdam.step_pair(enc, cpc)
        torch.cuda.synchronize()
        assert len(seen) == (3 if replaced else 0)
        res.append((flat.clone(), enc._m.clone(), enc._v.clone(), cpc._m.clone(), cpc._v.clone(), gflat.clone(),
                    cpc.clip_stats.clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert float(res[0][6][1]) < 1.0


def test_step_with_target_lerp_clipped():
    from curla_amd import ops
    from curla_amd.optim import FlatAdam
    sizes = [(32, 9, 3, 3), (32,), (50, 1203), (50,), (64, 52), (64,), (1, 64), (1,)]
    res = []
    for fused in (False, True):
        flat, gflat, params = _flat_params(sizes, "cuda", seed=7)
        n = flat.numel()
        target = (flat + 0.01 * torch.randn(n, generator=torch.Generator().manual_seed(2)).cuda()).contiguous()
        opt = FlatAdam(params, flat, gflat, lr=1e-3, betas=(0.9, 0.999), max_grad_norm=0.7)
        lo, hi = opt._lo, opt._hi
        split = (params[4].data_ptr() - flat.data_ptr()) // 4 - lo
        gen = torch.Generator().manual_seed(13)
        coefs = []
        for k in range(3):
            gflat.copy_(torch.randn(gflat.shape, generator=gen).cuda() * 0.01 * (k + 1))
            if fused:
                assert not FlatAdam.step_with_lerp(opt, target, lo + 4, hi, split, 0.05, 0.01)  # not its run: refused
                assert FlatAdam.step_with_lerp(opt, target, lo, hi, split, 0.05, 0.01)
            else:
                opt.step()
                ops.soft_update2(flat[lo:hi], target[lo:hi], split, 0.05, 0.01)
            coefs.append(float(opt.clip_stats[1]))
        torch.cuda.synchronize()
        assert all(c < 1.0 for c in coefs), coefs
        res.append((flat.clone(), opt._m.clone(), opt._v.clone(), target.clone(), gflat.clone(), opt.clip_stats.clone(),
                    list(opt._steps)))
    for a, b in zip(res[0][:6], res[1][:6]):
        assert torch.equal(a, b)
    assert res[0][6] == res[1][6] == [3] * len(sizes)


def test_step_with_float64_scalar_clipped():
    from curla_amd.optim import FlatAdam
    sizes = [(50, 120), (50,), (64, 50), (64,)]
    gen = torch.Generator().manual_seed(11)
    grads = [(torch.randn(sum(int(np.prod(z)) + 3 & ~3 for z in sizes) + 8, generator=gen) * 0.01 * (k + 1),
              torch.randn((), generator=gen, dtype=torch.float64)) for k in range(3)]
    res = []
    for fused in (False, True):
        flat, gflat, params = _flat_params(sizes, "cuda", seed=5)
        a = torch.tensor(np.log(0.1), device="cuda", requires_grad=True)
        a.grad = torch.zeros((), device="cuda", dtype=torch.float64)
        opt = FlatAdam(params, flat, gflat, lr=1e-3, max_grad_norm=0.3)
        sopt = torch.optim.Adam([a], lr=1e-4, betas=(0.5, 0.999), foreach=False)
        coefs = []
        for gf, ga in grads:
            gflat.copy_(gf[:gflat.numel()].cuda())
            a.grad.copy_(ga)
            if fused:
                FlatAdam.step_with_scalar(opt, sopt)
            else:
                opt.step()
                sopt.step()
            coefs.append(float(opt.clip_stats[1]))
            assert float(a.grad) == float(ga)  # the scalar's gradient is not clipped
        torch.cuda.synchronize()
        assert all(c < 1.0 for c in coefs), coefs
        st = sopt.state[a]
        res.append((flat.clone(), opt._m.clone(), opt._v.clone(), gflat.clone(), a.detach().clone(), st["exp_avg"].clone(),
                    st["exp_avg_sq"].clone(), float(st["step"]), list(opt._steps)))
    for x, y in zip(res[0][:4], res[1][:4]):
        assert torch.equal(x, y)
    for x, y in zip(res[0][4:7], res[1][4:7]):  # float64: same formula, torch may contract differently
        assert abs(float(x) - float(y)) <= 4e-16 * max(1.0, abs(float(x))), (float(x), float(y))
    assert res[0][7:] == res[1][7:] == (3.0, [3] * 4)
    assert float(res[1][4]) != float(np.log(0.1))


def test_bad_clip_arguments_fail_before_any_launch():
    from curla_amd import _lib
    lib = _lib.load()
    x = torch.zeros(64, device="cuda")
    part = torch.zeros(256, device="cuda", dtype=torch.float64)
    stats = torch.zeros(2, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    p, pp, ps = x.data_ptr(), part.data_ptr(), stats.data_ptr()
    ERR_ARG = lib.curla_grad_sqsum(None, 16, pp, 1, s)
    assert ERR_ARG != 0
    for args in ((p, 16, None, 1, s), (p, 16, pp, 0, s), (p, 16, pp, 257, s), (p, 0, pp, 1, s), (p + 2, 16, pp, 1, s),
                 (p, 16, pp + 4, 1, s)):
        assert lib.curla_grad_sqsum(*args) == ERR_ARG, args
    adam = (p, p + 64, p + 128, p + 192, 16, 1e-3, 0.9, 0.999, 1e-8, 1, None)
    for clip in ((None, 1, 1.0, ps), (pp, 0, 1.0, ps), (pp, 257, 1.0, ps), (pp, 1, 0.0, ps), (pp, 1, -1.0, ps),
                 (pp, 1, float("nan"), ps), (pp, 1, 1.0, None), (pp + 4, 1, 1.0, ps), (pp, 1, 1.0, ps + 2)):
        assert lib.curla_adam_step_clip(*adam, *clip, s) == ERR_ARG, clip
    torch.cuda.synchronize()
    assert float(x.abs().sum()) == 0.0 and float(part.abs().sum()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# the whole update (tests/test_gpu_graph._run: two agents from the same seeds, 14 steps on the same ring contents)

@functools.lru_cache(maxsize=None)
def _update_run(graphs, m, steps=14, edit_at=0, detach_encoder=False):
    from tests.test_gpu_graph import _run
    edit = None if m is None else (edit_at, lambda agent: agent.set_max_grad_norm(m))
    state, calls, np_pos, logs, agent = _run(graphs, steps=steps, detach_encoder=detach_encoder, edit=edit)
    stats = None if agent.grad_clip_stats is None else agent.grad_clip_stats.detach().cpu().clone()
    n_graphs = None if not graphs else sum(len(r) for r in agent._graphs.values())
    return dict(state=state, calls=calls, np=np_pos, logs=logs, stats=stats, n_graphs=n_graphs)


def _clipping_threshold():
    """Half the smallest norm the probe run (max_grad_norm = inf) met on its last step."""
    probe = _update_run(False, float("inf"))
    norms = probe["stats"][:, 0]
    assert bool((norms > 0).all()) and bool(torch.isfinite(norms).all()), norms
    return 0.5 * float(norms.min())


def test_update_with_an_infinite_threshold_is_the_plain_update():
    plain, probe = _update_run(False, None), _update_run(False, float("inf"))
    for k in plain["state"]:
        assert torch.equal(plain["state"][k], probe["state"][k]), k
    assert plain["np"] == probe["np"]
    assert probe["stats"][:, 1].tolist() == [1.0] * 3 and plain["stats"] is None
    norm_keys = {"train_critic/grad_norm", "train_actor/grad_norm", "train/curl_grad_norm"}
    assert norm_keys <= set(probe["logs"]) and not norm_keys & set(plain["logs"])
    assert {k: v for k, v in probe["logs"].items() if k not in norm_keys} == plain["logs"]
    assert all(probe["logs"][k] > 0 for k in norm_keys)


def test_update_clips_every_phase():
    m = _clipping_threshold()
    plain, clipped = _update_run(False, None), _update_run(False, m)
    for name in ("critic", "actor", "encoder", "cpc"):
        for mom in ("_m", "_v"):
            assert not torch.equal(plain["state"][name + mom], clipped["state"][name + mom]), name + mom
        assert torch.equal(plain["state"][name + "_steps"], clipped["state"][name + "_steps"])
    assert float(clipped["stats"][0, 1]) < 1.0
    assert bool((clipped["stats"][:, 1] <= 1.0).all()) and bool((clipped["stats"][:, 0] > 0).all())
    for k, v in clipped["state"].items():
        assert bool(torch.isfinite(v.double()).all()), k


def test_graph_replay_of_the_clipped_update_is_the_eager_one():
    m = _clipping_threshold()
    eager, graph = _update_run(False, m), _update_run(True, m)
    assert min(eager["calls"]) > 15
    replayed = [8, 9, 11, 12, 13]  # (test_gpu_graph: 0, 5, 10 log, 1, 2 warm up, 3, 4, 6, 7 capture)
    assert [graph["calls"][s] for s in replayed] == [0] * len(replayed), graph["calls"]
    assert all(graph["calls"][s] > 15 for s in (0, 1, 2, 3, 4, 5, 6, 7, 10)), graph["calls"]
    assert graph["n_graphs"] == 4
    assert eager["np"] == graph["np"] and eager["logs"] == graph["logs"]
    for k in eager["state"]:
        assert torch.equal(eager["state"][k], graph["state"][k]), k
    assert torch.equal(eager["stats"], graph["stats"])


def test_editing_the_threshold_recaptures():
    m = _clipping_threshold()
    eager, graph = _update_run(False, m, steps=20, edit_at=11), _update_run(True, m, steps=20, edit_at=11)
    calls = graph["calls"]
    assert calls[9] == 0 and calls[11] > 15  # replaying before the edit, eager (warm-up of the new graphs) after
    assert calls[19] == 0                    # ... and replaying again at the end
    assert eager["np"] == graph["np"] and eager["logs"] == graph["logs"]
    for k in eager["state"]:
        assert torch.equal(eager["state"][k], graph["state"][k]), k
    assert torch.equal(eager["stats"], graph["stats"]) and float(eager["stats"][0, 1]) < 1.0


def test_detached_encoder_norm_counts_only_what_the_critic_steps():
    """Under detach_encoder the convs have no gradient at the critic's step: the phase's norm is fc / ln / Q's, as
    torch skips ``grad is None``.  The gradient is seen through a ``step`` replaced on the instance (the route
    FlatAdam.step_pair documents), which clones the flat gradient and then takes the class's step."""
    from curla_amd.optim import FlatAdam
    from tests.test_gpu_graph import _run
    m = _clipping_threshold()
    seen = {}

    def edit(agent):
        agent.set_max_grad_norm(m)
        opt = agent.critic_optimizer

        def step(closure=None):
            seen["g"] = opt._gflat.clone()
            seen["live"] = [(a, b) for (a, b), p in zip(opt._span, opt._plist) if p.grad is not None]
            seen["all"] = len(opt._plist)
            return FlatAdam.step(opt)
        opt.step = step
    _, _, _, _, agent = _run(False, detach_encoder=True, edit=(0, edit))
    assert len(seen["live"]) == seen["all"] - 8  # 4 conv layers x (weight, bias) are out
    g = seen["g"].cpu().numpy()
    want_norm, want_coef, _ = norm_and_coef([g[a:b] for a, b in seen["live"]], m)
    got = agent.grad_clip_stats[0].cpu().numpy()
    print(f"detach_encoder critic norm {got[0]!r} (float64 {want_norm!r}), coef {got[1]!r} ({want_coef!r})")
    assert within_ulps(got[0], want_norm) and within_ulps(got[1], want_coef)
    everything = norm_and_coef([g[a:b] for a, b in agent.critic_optimizer._span], m)[0]
    assert not within_ulps(got[0], everything, ulps=16)  # (the convs' slots are not empty: counting them would show)


# ---------------------------------------------------------------------------------------------------------------------
# data parallel: the norm is taken over the REDUCED gradient, the deferred actor step of the overlapped schedule included

@pytest.fixture(scope="module")
def nccl_world1():
    import torch.distributed as dist
    from tests.test_gpu_dp import _free_port
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    yield dist
    dist.destroy_process_group()


def _dp_run(mode, m, steps=4, B=16):
    import curla_amd
    from tests.test_gpu_dp import HP, Log
    dev = torch.device("cuda", 0)
    curla_amd.set_seed_everywhere(7)
    in_hw, out_hw = (40, 44), (32, 36)
    aug = curla_amd.RandomCrop(in_hw, out_hw)
    agent = curla_amd.CurlSacAgent((9,) + out_hw, (2,), dev, aug, hidden_dim=96, **HP)
    agent.set_max_grad_norm(m)
    if mode is not None:
        agent.enable_data_parallel(single_rank_collectives=True, **mode)
    rb = curla_amd.ReplayBuffer((9,) + in_hw, (2,), 64, B, dev, aug)
    rs = np.random.RandomState(0)
    n = 40
    rb.add_batch(rs.randint(0, 256, (n, 9) + in_hw, dtype=np.uint8), rs.uniform(-1, 1, (n, 2)).astype(np.float32),
                 rs.randn(n).astype(np.float32), rs.randint(0, 256, (n, 9) + in_hw, dtype=np.uint8),
                 (np.arange(n) % 9) == 8)
    curla_amd.set_seed_everywhere(11)
    L = Log()
    for step in range(steps):
        agent.update(rb, L, step)
    torch.cuda.synchronize()
    assert not agent._dp_pending
    return dict(critic=agent._critic_flat.clone(), target=agent._target_flat.clone(), actor=agent._actor_flat.clone(),
                log_alpha=agent.log_alpha.detach().clone(), stats=agent.grad_clip_stats.clone(),
                actor_m=agent.actor_optimizer._m.clone(), critic_m=agent.critic_optimizer._m.clone(),
                cpc_m=agent.cpc_optimizer._m.clone()), dict(L.s)


def test_world1_rccl_clipped_update_is_the_single_gpu_one(nccl_world1):
    probe, _ = _dp_run(None, float("inf"))
    m = 0.5 * float(probe["stats"][:, 0].min())
    assert m > 0
    base, logs = _dp_run(None, m)
    assert bool((base["stats"][:, 1] < 1.0).all()), base["stats"]  # every phase clips on the last step it ran
    assert not torch.equal(base["actor_m"], probe["actor_m"])
    for name, mode in (("overlapped", dict(overlap=True, check_every=2)), ("blocking", dict(overlap=False, check_every=0))):
        other, other_logs = _dp_run(mode, m)
        for k in base:
            assert torch.equal(base[k], other[k]), f"{name} RCCL world-1 clipped run differs from the single-GPU run in {k}"
        assert logs == other_logs, name
