"""Decoupled weight decay (AdamW) inside the flat Adam launches on the MI355X: ``FlatAdam(weight_decay=wd,
decoupled_weight_decay=True)``, the ``curla_adamw_*`` entry points and ``CurlSacAgent.set_weight_decay``.

The specification is exact (tests/test_weight_decay_host.py pins it to the installed torch on the CPU): AdamW is
``param *= float32(1 - lr * weight_decay)`` -- the factor formed in double, rounded once -- followed by the plain Adam
step.  So a decaying launch is compared BIT FOR BIT with that multiply done by torch on the same buffers followed by the
plain launch, in every launch form, clipped and unclipped; a whole decaying update with an agent whose optimizers' steps
do the multiply themselves.  Against ``torch.optim.AdamW`` on the CPU the steps are held to the 2e-6 that
``test_gpu_kernels.test_flat_adam_matches_torch_adam`` holds plain Adam to: the decay adds one exact multiply on both
sides."""
import collections
import functools

import numpy as np
import pytest
import torch

from tests.test_gpu_grad_clip import _flat_params_shifted
from tests.test_gpu_kernels import _flat_params, check

pytestmark = pytest.mark.gpu

# the layout of test_gpu_kernels.test_flat_adam_matches_torch_adam: runs that are and are not multiples of 4, a 1-element
# run (when parameter 2 loses its gradient the step is over two runs: 2624 and 58432 elements)
SIZES = [(32, 9, 3, 3), (32,), (50, 1203), (50,), (1,), (1024, 57), (7,)]
# ... and one whose buffers start 4 bytes behind a 16-byte boundary: no launch takes the 16-byte path
SHIFTED = [(12, 9), (512,), (513,), (3,), (130, 5), (7,)]
LAYOUTS = {"aligned": (SIZES, 0), "off_16_bytes": (SHIFTED, 1)}
LOST = 2            # the parameter that loses its gradient ...
LOST_STEPS = (2, 3)  # ... on these steps
WD, LR = 1e-2, 1e-3
WD2, LR2 = 0.1, 3e-4  # step_pair's second optimizer


def _factor(lr, wd):
    return float(np.float32(1.0 - lr * wd))


def _buffers(layout, seed=0):
    sizes, shift = LAYOUTS[layout]
    return _flat_params_shifted(sizes, shift, seed) if shift else _flat_params(sizes, "cuda", seed)


@functools.lru_cache(maxsize=None)
def _gradients(layout):
    """Six steps' gradients per parameter (CPU), scales from 1e-2 to 1 as in test_flat_adam_matches_torch_adam, and the
    float64 scalar's."""
    sizes, _ = LAYOUTS[layout]
    gen = torch.Generator().manual_seed(5)
    return [([torch.randn(n, generator=gen) * (10.0 ** (i % 3 - 2)) for i, n in enumerate(sizes)],
             torch.randn((), generator=gen, dtype=torch.float64)) for _ in range(6)]


def _mul(opt, wd):
    """The reference's half of the identity: every live parameter times the float32 factor, by torch."""
    g = opt.param_groups[0]
    d = _factor(float(g["lr"]), wd)
    assert d != 1.0
    for p in opt._plist:
        if p.grad is not None:
            p.data.mul_(d)


@functools.lru_cache(maxsize=None)
def _six_steps(form, layout, betas, max_grad_norm, how):
    """Six steps of one launch form.  ``how``: "decay" (FlatAdams with the decay), "by hand" (weight_decay=0 FlatAdams,
    every live parameter multiplied by the factor in front of each one's plain step) or "plain" (no decay at all).
    Returns every buffer the launches touch, cloned, and the clip coefficients."""
    from curla_amd import ops
    from curla_amd.optim import FlatAdam
    flat, gflat, params = _buffers(layout)
    views = [p.grad for p in params]
    kw = dict(decoupled_weight_decay=True) if how == "decay" else {}
    wd1, wd2 = (WD, WD2) if how == "decay" else (0.0, 0.0)
    opt = FlatAdam(params[1:] if form == "pair" else params, flat, gflat, lr=LR, betas=betas, weight_decay=wd1,
                   max_grad_norm=max_grad_norm, **kw)
    second = target = a = sopt = None
    if form == "pair":  # [W | encoder]: the first optimizer's parameters are the tail of the second's
        second = FlatAdam(params, flat, gflat, lr=LR2, betas=(0.8, 0.99), weight_decay=wd2, max_grad_norm=max_grad_norm,
                          **kw)
        if how == "by hand":  # (a step replaced on the instance: the route FlatAdam.step_pair documents and respects)
            for o, wd in ((opt, WD), (second, WD2)):
                def step(closure=None, o=o, wd=wd):
                    _mul(o, wd)
                    return FlatAdam.step(o)
                o.step = step
    if form == "lerp":
        target = (flat + 0.01 * torch.randn(flat.numel(), generator=torch.Generator().manual_seed(2)).cuda()).contiguous()
        lo, hi = opt._lo, opt._hi
        split = (params[4].data_ptr() - flat.data_ptr()) // 4 - lo
    if form == "scalar":
        a = torch.tensor(np.log(0.1), device="cuda", requires_grad=True)
        a.grad = torch.zeros((), device="cuda", dtype=torch.float64)
        sopt = torch.optim.Adam([a], lr=1e-4, betas=(0.5, 0.999), foreach=False)
    coefs, still = [], None
    for k, (grads, ga) in enumerate(_gradients(layout)):
        lost = k in LOST_STEPS
        params[LOST].grad = None if lost else views[LOST]
        gflat.zero_()
        for i, g in enumerate(grads):
            if not (lost and i == LOST):
                views[i].copy_(g.cuda())
        if k == LOST_STEPS[0]:
            still = params[LOST].detach().clone()
        if how == "by hand" and form != "pair":
            _mul(opt, WD)
        if form == "step":
            opt.step()
        elif form == "pair":
            FlatAdam.step_pair(opt, second)
        elif form == "lerp":
            if not FlatAdam.step_with_lerp(opt, target, lo, hi, split, 0.05, 0.01):
                assert k >= LOST_STEPS[0]  # (no longer ONE run with one step count: the caller's two steps)
                opt.step()
                ops.soft_update2(flat[lo:hi], target[lo:hi], split, 0.05, 0.01)
        else:
            a.grad.copy_(ga)
            FlatAdam.step_with_scalar(opt, sopt)
        if max_grad_norm is not None:
            coefs.append(float((second or opt).clip_stats[1]))
        if k == LOST_STEPS[-1]:
            assert torch.equal(params[LOST].detach(), still)  # no gradient: neither stepped nor decayed
    torch.cuda.synchronize()
    out = dict(flat=flat, m=opt._m, v=opt._v, grad=gflat)
    if second is not None:
        out.update(m2=second._m, v2=second._v)
    if target is not None:
        out["target"] = target
    if a is not None:
        st = sopt.state[a]
        out.update(scalar=a.detach(), scalar_m=st["exp_avg"], scalar_v=st["exp_avg_sq"])
    out = {k: v.detach().clone() for k, v in out.items()}
    covered = torch.zeros(flat.numel(), dtype=torch.bool)
    off = flat.data_ptr()
    for p in params:
        covered[(p.data_ptr() - off) // 4:(p.data_ptr() - off) // 4 + p.numel()] = True
    out["padding"] = out["flat"].cpu()[~covered]
    steps = (list(opt._steps), None if second is None else list(second._steps))
    return out, coefs, steps


FORMS = ["step", "pair", "lerp", "scalar"]


@pytest.mark.parametrize("max_grad_norm", [None, 1.0], ids=["unclipped", "clipped"])
@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.5, 0.999)])
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("form", FORMS)
def test_decaying_launch_is_the_multiply_then_the_plain_launch(form, layout, betas, max_grad_norm):
    """Bit for bit: parameters, both moments (of both optimizers), the target copy, the float64 scalar with its moments
    and the written-back gradient.  Steps 2-3 are over two runs (a parameter without a gradient, which must not move)
    and from step 4 on that parameter's step count is its own: the fused forms then take their separate steps, so every
    launch form (steps 0-1) AND the step per run and per piece are covered.  step_pair's
    two optimizers carry different decays and learning rates; the first n_pre elements see only the second's.
    (Fails without the feature: FlatAdam takes no weight_decay.)"""
    got, coefs, steps = _six_steps(form, layout, betas, max_grad_norm, "decay")
    want, coefs_w, steps_w = _six_steps(form, layout, betas, max_grad_norm, "by hand")
    assert set(got) == set(want)
    for k in got:
        assert torch.equal(got[k], want[k]), (form, layout, k)
    assert steps == steps_w and coefs == coefs_w
    if max_grad_norm is not None:
        assert len(coefs) == 6 and all(c < 1.0 for c in coefs), coefs  # every step clips
    assert float(got["padding"].abs().sum()) == 0.0 and got["padding"].numel() > 0  # bridged padding stays zero
    plain, _, _ = _six_steps(form, layout, betas, max_grad_norm, "plain")
    assert not torch.equal(plain["flat"], got["flat"])  # (the decay acts ...)
    if form == "scalar":  # (... and never on the scalar, whose optimizer is its own)
        for k in ("scalar", "scalar_m", "scalar_v"):
            assert torch.equal(plain[k], got[k]), k
    if form == "pair":  # W, in front of n_pre, is decayed by the second optimizer alone: d2 per step from the start
        n_pre = int(np.prod(LAYOUTS[layout][0][0]))
        assert not torch.equal(plain["flat"][:n_pre], got["flat"][:n_pre])


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.5, 0.999)])
@pytest.mark.parametrize("form", ["step", "pair"])
def test_decaying_steps_match_torch_adamw(form, betas):
    """The same six steps against torch.optim.AdamW on the CPU (step_pair: two AdamWs over the same parameters, stepped
    one after the other), to the bound plain Adam is held to."""
    got, _, _ = _six_steps(form, "aligned", betas, None, "decay")
    _, _, params = _buffers("aligned")
    ref_params = [torch.nn.Parameter(p.detach().cpu().clone()) for p in params]
    first = torch.optim.AdamW(ref_params[1:] if form == "pair" else ref_params, lr=LR, betas=betas, weight_decay=WD)
    second = torch.optim.AdamW(ref_params, lr=LR2, betas=(0.8, 0.99), weight_decay=WD2) if form == "pair" else None
    for k, (grads, _) in enumerate(_gradients("aligned")):
        for i, (r, g) in enumerate(zip(ref_params, grads)):
            r.grad = None if (k in LOST_STEPS and i == LOST) else g.clone()
        first.step()
        if second is not None:
            second.step()
    flat, off = got["flat"].cpu(), 0
    last = second or first
    for i, r in enumerate(ref_params):
        n = r.numel()
        check(f"adamw {form}{betas} param{i}", flat[off:off + n].view(r.shape), r.detach(), 2e-6)
        m, v = (got["m2"], got["v2"]) if form == "pair" else (got["m"], got["v"])
        check(f"adamw {form}{betas} exp_avg{i}", m.cpu()[off:off + n].view(r.shape), last.state[r]["exp_avg"], 2e-6)
        check(f"adamw {form}{betas} exp_avg_sq{i}", v.cpu()[off:off + n].view(r.shape), last.state[r]["exp_avg_sq"], 2e-6)
        off += (n + 3) & ~3


def _raw(n, extra=0, seed=0):
    gen = torch.Generator().manual_seed(seed)
    t = lambda k, scale=1.0: (torch.randn(k, generator=gen) * scale).cuda()  # noqa: E731
    return dict(p=t(n), g=t(n, 0.1), m=t(n, 0.01), v=t(n, 0.01).abs(), m2=t(n, 0.01), v2=t(n, 0.01).abs(), tgt=t(n),
                s=torch.randn(4, generator=gen, dtype=torch.float64).abs().cuda(),
                part=torch.zeros(256, device="cuda", dtype=torch.float64), stats=torch.zeros(2, device="cuda"))


def _entry_args(form, b, n, n_pre, new, clipped, wd=0.0, wd2=0.0):
    """The argument tuple of curla_adam_<form>[_clip] (``new`` False) or curla_adamw_<form> over the raw buffers ``b``."""
    decay = lambda w: (w,) if new else ()  # noqa: E731
    ptr = {k: v.data_ptr() for k, v in b.items()}
    if form == "step2":
        args = (ptr["p"], ptr["g"], ptr["m"], ptr["v"], ptr["m2"], ptr["v2"], n, n_pre,
                1e-3, 0.9, 0.999, 1e-8) + decay(wd) + (2, 3e-4, 0.8, 0.99, 1e-7) + decay(wd2) + (3, None)
    else:
        args = (ptr["p"], ptr["g"], ptr["m"], ptr["v"], n, 1e-3, 0.9, 0.999, 1e-8) + decay(wd) + (2, None)
        if form == "step_lerp":
            args += (ptr["tgt"], 2592, 0.05, 0.95, 0.01, 0.99)
        if form == "step_scalar64":
            s = ptr["s"]
            args += (s, s + 8, s + 16, s + 24, 1e-4, 0.5, 0.999, 1e-8, 2, None)
    if clipped:
        args += (ptr["part"], 4, 0.5, ptr["stats"])
    elif new:
        args += (None, 0, 0.0, None)
    return args


@pytest.mark.parametrize("clipped", [False, True], ids=["unclipped", "clipped"])
@pytest.mark.parametrize("misalign", [0, 1], ids=["aligned", "off_16_bytes"])
@pytest.mark.parametrize("form", ["step", "step_lerp", "step_scalar64", "step2"])
def test_zero_decay_through_the_new_entry_points_is_the_old_entry_point(form, misalign, clipped):
    """weight_decay = 0 gives d = 1 and p * 1 is exact: curla_adamw_* then leaves what curla_adam_*[_clip] leaves, bit
    for bit, in every buffer (60157 elements: the vector path and a 1-element tail; from an address 4 bytes behind a
    16-byte boundary: the scalar path alone)."""
    from curla_amd import _lib
    n, n_pre = 60157, 2592
    s = torch.cuda.current_stream().cuda_stream
    res = []
    for new in (False, True):
        b = _raw(n + 4)
        if misalign:
            b = {k: (v[1:] if v.dtype == torch.float32 and v.numel() > 2 else v) for k, v in b.items()}
        if clipped:
            _lib.call("curla_grad_sqsum", b["g"].data_ptr(), n, b["part"].data_ptr(), 4, s)
        name = ("curla_adamw_" + form) if new else ("curla_adam_" + form + ("_clip" if clipped else ""))
        _lib.call(name, *_entry_args(form, b, n, n_pre, new, clipped), s)
        torch.cuda.synchronize()
        res.append({k: v.clone() for k, v in b.items()})
    for k in res[0]:
        assert torch.equal(res[0][k], res[1][k]), (form, k)
    fresh = _raw(n + 4)
    assert not torch.equal(res[0]["p"], fresh["p"][misalign:] if misalign else fresh["p"])  # (a step was taken)
    if clipped:
        assert float(res[1]["stats"][1]) < 1.0


def test_decay_order_inside_step2():
    """curla_adamw_step2 with two different decays against the launches it stands for, bit for bit: behind n_pre
    p *= d1, Adam 1, p *= d2, Adam 2; the first n_pre elements p *= d2, Adam 2 -- from raw buffers with non-zero moments,
    the 16-byte path and (n_pre = 2591) the scalar path."""
    from curla_amd import _lib
    n = 60157
    s = torch.cuda.current_stream().cuda_stream
    for n_pre in (2592, 2591):
        one = _raw(n)
        _lib.call("curla_adamw_step2", *_entry_args("step2", one, n, n_pre, True, False, wd=0.3, wd2=0.7), s)
        two = _raw(n)
        p = {k: v.data_ptr() for k, v in two.items()}
        two["p"][n_pre:].mul_(_factor(1e-3, 0.3))
        _lib.call("curla_adam_step", p["p"] + 4 * n_pre, p["g"] + 4 * n_pre, p["m"], p["v"], n - n_pre, 1e-3, 0.9, 0.999,
                  1e-8, 2, None, s)
        two["p"][:n].mul_(_factor(3e-4, 0.7))
        _lib.call("curla_adam_step", p["p"], p["g"], p["m2"], p["v2"], n, 3e-4, 0.8, 0.99, 1e-7, 3, None, s)
        torch.cuda.synchronize()
        for k in one:
            assert torch.equal(one[k], two[k]), (n_pre, k)


def test_bad_arguments_fail_before_any_launch():
    from curla_amd import _lib
    lib = _lib.load()
    n = 16
    b = _raw(64)
    before = {k: v.clone() for k, v in b.items()}
    s = torch.cuda.current_stream().cuda_stream
    ERR_ARG = lib.curla_grad_sqsum(None, 16, b["part"].data_ptr(), 1, s)
    assert ERR_ARG != 0
    nan, inf = float("nan"), float("inf")
    pp, ps = b["part"].data_ptr(), b["stats"].data_ptr()
    for form in ("step", "step_lerp", "step_scalar64", "step2"):
        fn = getattr(lib, "curla_adamw_" + form)
        good = _entry_args(form, b, n, 8, True, False, wd=0.1, wd2=0.2)
        wd_at = (12, 18) if form == "step2" else (9,)
        clip_at = len(good) - 4
        bad = []
        for at in wd_at:
            bad += [good[:at] + (w,) + good[at + 1:] for w in (-1e-3, nan, inf, -inf)]
        # partials == NULL with n_partials != 0; and what the _clip namesake refuses of a clip argument
        for clip in ((None, 1, 0.0, None), (None, 1, 1.0, ps), (pp, 0, 1.0, ps), (pp, 257, 1.0, ps), (pp, 1, 0.0, ps),
                     (pp, 1, nan, ps), (pp, 1, 1.0, None), (pp + 4, 1, 1.0, ps), (pp, 1, 1.0, ps + 2)):
            bad.append(good[:clip_at] + clip)
        # ... and of the step itself: a NULL or misaligned float pointer, n = 0, step 0, beta 1
        bad += [(None,) + good[1:], good[:1] + (None,) + good[2:], (good[0] + 2,) + good[1:]]
        n_at, step_at = (6, 13) if form == "step2" else (4, 10)
        bad += [good[:n_at] + (0,) + good[n_at + 1:], good[:step_at] + (0,) + good[step_at + 1:]]
        beta_at = 9 if form == "step2" else 6
        bad.append(good[:beta_at] + (1.0,) + good[beta_at + 1:])
        if form == "step2":
            bad.append(good[:7] + (n + 1,) + good[8:])  # n_pre > n
        if form == "step_lerp":
            bad += [good[:12] + (None,) + good[13:], good[:13] + (n + 1,) + good[14:]]  # no target; split > n
        if form == "step_scalar64":
            bad += [good[:12] + (None,) + good[13:], good[:12] + (good[12] + 4,) + good[13:]]
        for args in bad:
            assert len(args) == len(good)
            assert fn(*args, s) == ERR_ARG, (form, args)
    torch.cuda.synchronize()
    for k in b:
        assert torch.equal(b[k], before[k]), k


# ---------------------------------------------------------------------------------------------------------------------
# the whole update (tests/test_gpu_graph._run: agents from the same seeds, the same steps on the same ring contents)

AGENT_WD = 1e-2
NETWORK_OPTIMIZERS = ("critic", "actor", "encoder", "cpc")


def _decay_by_hand(agent, wd=AGENT_WD):
    """No decay in the groups; each network optimizer's ``step`` replaced on the instance by: every parameter with a
    gradient times that optimizer's float32 factor, then the class's step (the route FlatAdam documents and respects:
    the fused launches step aside for it).
    Beside a replaced actor step, log_alpha would be stepped by torch's own float64 Adam, which is the launch's float64
    rider only to 4e-16 (torch may contract a product and a sum: test_gpu_kernels.test_flat_adam_step_with_float64_scalar)
    -- a difference that has nothing to do with weight decay and would hide everything behind it.  So log_alpha's step is
    replaced as well, by that rider: the one launch form that has it, over a one-element flat run of its own."""
    from curla_amd.optim import FlatAdam
    for name in NETWORK_OPTIMIZERS:
        opt = getattr(agent, name + "_optimizer")

        def step(closure=None, opt=opt):
            with torch.no_grad():
                _mul(opt, wd)
            return FlatAdam.step(opt)
        opt.step = step
    flat, gflat = torch.zeros(4, device="cuda"), torch.zeros(4, device="cuda")
    p = torch.nn.Parameter(flat[:1])
    p.grad = gflat[:1]
    carrier, la_opt = FlatAdam([p], flat, gflat), agent.log_alpha_optimizer

    def la_step(closure=None):
        del la_opt.step  # (step_with_scalar steps aside for a replaced step: take it off for the call)
        try:
            FlatAdam.step_with_scalar(carrier, la_opt)
        finally:
            la_opt.step = la_step
    la_opt.step = la_step


def _set(wd):
    return lambda agent: agent.set_weight_decay(wd)


def _both(*fns):
    def edit(agent):
        for fn in fns:
            fn(agent)
    return edit


EDITS = {
    None: None,
    "decay": (0, _set(AGENT_WD)),
    "by hand": (0, _decay_by_hand),
    "other decay at 11": (11, _set(3e-2)),
    "lr at 11": (11, lambda agent: agent.critic_optimizer.param_groups[0].__setitem__("lr", 3e-4)),
}


@functools.lru_cache(maxsize=None)
def _update_run(graphs, first, then=None, steps=14, detach_encoder=False, clip=None):
    """``first`` / ``then``: names of EDITS, applied in front of their steps."""
    from tests.test_gpu_graph import _run
    edits = [EDITS[e] for e in (first, then) if EDITS[e] is not None]
    if clip is not None:
        edits.append((0, lambda agent: agent.set_max_grad_norm(clip)))
    # _run takes ONE (step, fn): a second edit, at a later step, is made by the agent's update() wrapped at step 0
    by_step = collections.defaultdict(list)
    for at, fn in edits:
        by_step[at].append(fn)
    ats = sorted(by_step)
    if not ats:
        hook = None
    elif len(ats) == 1:
        hook = (ats[0], _both(*by_step[ats[0]]))
    else:
        assert ats[0] == 0 and len(ats) == 2

        def at_zero(agent):
            _both(*by_step[0])(agent)
            real = agent.update

            def update(rb, L, step, *a, **k):
                if step == ats[1]:
                    _both(*by_step[ats[1]])(agent)
                return real(rb, L, step, *a, **k)
            agent.update = update
        hook = (0, at_zero)
    st, calls, np_pos, logs, agent = _run(graphs, steps=steps, detach_encoder=detach_encoder, edit=hook)
    n_graphs = None if not graphs else sum(len(r) for r in agent._graphs.values())
    stats = None if agent.grad_clip_stats is None else agent.grad_clip_stats.detach().cpu().clone()
    return dict(state=st, calls=calls, np=np_pos, logs=logs, n_graphs=n_graphs, wd=agent.weight_decay, stats=stats)


def _same(a, b):
    assert set(a["state"]) == set(b["state"])
    for k in a["state"]:
        assert torch.equal(a["state"][k], b["state"][k]), k


@pytest.mark.parametrize("detach_encoder", [False, True])
def test_decaying_update_is_the_update_whose_steps_multiply_first(detach_encoder):
    """14 eager steps: set_weight_decay(wd) against the agent whose four optimizers' steps multiply by their float32
    factor themselves -- every tensor of the state, bit for bit; and the decay is live in every phase.  Under
    detach_encoder the convs have no gradient at the critic's step: they carry only the encoder / cpc decays (the
    by-hand agent multiplies only parameters with a gradient, as torch's AdamW does)."""
    a = _update_run(False, "decay", detach_encoder=detach_encoder)
    b = _update_run(False, "by hand", detach_encoder=detach_encoder)
    assert a["wd"] == AGENT_WD and b["wd"] == 0.0
    _same(a, b)
    assert a["np"] == b["np"] and a["logs"] == b["logs"]
    plain = _update_run(False, None, detach_encoder=detach_encoder)
    for name in NETWORK_OPTIMIZERS:  # the moments see the decay through the next gradients: live in each phase
        assert not torch.equal(plain["state"][name + "_m"], a["state"][name + "_m"]), name
        assert torch.equal(plain["state"][name + "_steps"], a["state"][name + "_steps"])
    for k in ("critic", "actor", "target"):
        assert not torch.equal(plain["state"][k], a["state"][k]), k
        assert bool(torch.isfinite(a["state"][k]).all())


def test_graph_replay_of_the_decaying_update_is_the_eager_one():
    eager, graph = _update_run(False, "decay"), _update_run(True, "decay")
    assert min(eager["calls"]) > 15
    replayed = [8, 9, 11, 12, 13]  # (test_gpu_graph: 0, 5, 10 log, 1, 2 warm up, 3, 4, 6, 7 capture)
    assert [graph["calls"][s] for s in replayed] == [0] * len(replayed), graph["calls"]
    assert all(graph["calls"][s] > 15 for s in (0, 1, 2, 3, 4, 5, 6, 7, 10)), graph["calls"]
    assert graph["n_graphs"] == 4
    assert eager["np"] == graph["np"] and eager["logs"] == graph["logs"]
    _same(eager, graph)


@pytest.mark.parametrize("then", ["other decay at 11", "lr at 11"])
def test_editing_the_decay_or_a_decaying_optimizers_lr_recaptures(then):
    """A captured launch holds float32(1 - lr * weight_decay) by value: a new decay, and a new lr of an optimizer that
    decays, make the graphs stale.  They are captured again and the run stays the eager one."""
    eager, graph = _update_run(False, "decay", then, steps=20), _update_run(True, "decay", then, steps=20)
    calls = graph["calls"]
    assert calls[9] == 0 and calls[11] > 15  # replaying before the edit, eager (warm-up of the new graphs) after
    assert calls[19] == 0                    # ... and replaying again at the end
    assert eager["np"] == graph["np"] and eager["logs"] == graph["logs"]
    _same(eager, graph)
    unedited = _update_run(False, "decay", None, steps=20)
    assert not torch.equal(unedited["state"]["critic"], eager["state"]["critic"])  # (the edit matters)


def test_graph_replay_with_decay_and_clipping():
    from tests.test_gpu_grad_clip import _clipping_threshold
    m = _clipping_threshold()
    eager, graph = _update_run(False, "decay", clip=m), _update_run(True, "decay", clip=m)
    assert [graph["calls"][s] for s in (8, 9, 11, 12, 13)] == [0] * 5, graph["calls"]
    _same(eager, graph)
    assert torch.equal(eager["stats"], graph["stats"]) and float(eager["stats"][0, 1]) < 1.0
    assert not torch.equal(eager["state"]["critic"], _update_run(False, "decay")["state"]["critic"])


@pytest.mark.parametrize("wd", [AGENT_WD, 0.0])
def test_launch_counts_of_an_even_step(wd):
    """With weight decay an update launches as many optimizer kernels as without: the critic's step shares its launch
    with the target lerp, the actor's with log_alpha, the encoder's with cpc's -- the curla_adamw_* forms with decay,
    the plain family (the counts test_gpu_agent asserts) without."""
    import curla_amd.optim as optim_mod
    from tests.test_gpu_graph import _run
    names = []

    def edit(agent):
        agent.set_weight_decay(wd)
        inner = optim_mod.call  # (_run's counting wrapper, which _run itself takes off again)

        def call(name, *a):
            names.append(name)
            return inner(name, *a)
        optim_mod.call = call
    _run(False, steps=3, edit=(2, edit))
    c = collections.Counter(names)
    family = "curla_adamw_" if wd else "curla_adam_"
    other = "curla_adam_" if wd else "curla_adamw_"
    assert c[family + "step_lerp"] == 1 and c[family + "step_scalar64"] == 1 and c[family + "step2"] == 1, c
    assert sum(v for k, v in c.items() if k.startswith(other)) == 0, c
    assert sum(v for k, v in c.items() if k.startswith(family)) == 3, c


def test_checkpoint_of_a_decaying_agent_resumes_bitwise(tmp_path):
    from tests.test_gpu_agent import NullLogger
    from tests.test_gpu_graph import _run
    _, _, _, _, agent = _run(False, steps=6, edit=(0, _set(AGENT_WD)))
    path = str(tmp_path / "decay.pt")
    agent.save_checkpoint(path, 6)
    _, _, _, _, other = _run(False, steps=2)  # a fresh agent without decay, somewhere else in its run
    assert other.weight_decay == 0.0
    out = []
    for ag in (agent, other):
        assert ag.load_checkpoint(path) == 6  # (both continue from the file: the RNG streams are in it)
        assert ag.weight_decay == AGENT_WD
        for name in NETWORK_OPTIMIZERS:
            g = getattr(ag, name + "_optimizer").param_groups[0]
            assert g["weight_decay"] == AGENT_WD and g["decoupled_weight_decay"] is True
        assert ag.log_alpha_optimizer.param_groups[0]["weight_decay"] == 0
        L = NullLogger()
        for step in range(6, 10):
            ag.update(ag._test_rb, L, step)
        torch.cuda.synchronize()
        out.append({k: v.detach().cpu().clone() for k, v in dict(
            critic=ag._critic_flat, target=ag._target_flat, actor=ag._actor_flat, log_alpha=ag.log_alpha.detach(),
            critic_m=ag.critic_optimizer._m, actor_v=ag.actor_optimizer._v, cpc_m=ag.cpc_optimizer._m).items()})
    for k in out[0]:
        assert torch.equal(out[0][k], out[1][k]), k
