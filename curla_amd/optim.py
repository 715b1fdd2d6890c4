"""Adam over the learner's flat parameter buffers.

``FlatAdam`` IS a ``torch.optim.Adam`` (same constructor hyper-parameters,
``param_groups``, ``state`` keys, ``state_dict()`` / ``load_state_dict()``
format -- curl_sac.py:299-313 builds five of them), but its ``step()`` is one
HIP launch per contiguous run of live parameters in the flat buffer
(``curla_adam_step``) instead of torch's multi-tensor launches, which put ~70
workgroups on a 256-CU chip (45 us for 6 MB of parameters; the flat kernel
streams the same 7 arrays at HBM rate).  The moments live in two flat mirror
buffers; ``state[p]['exp_avg']`` / ``['exp_avg_sq']`` are views into them, so a
checkpoint written from ``state_dict()`` is what torch's Adam would write.

``max_grad_norm`` (off by default) clips the gradient of a step by its global norm inside those launches:
``torch.nn.utils.clip_grad_norm_(live parameters, max_grad_norm)`` right in front of ``step()``, as one square-sum launch
per run (``curla_grad_sqsum``: float64 partial sums in a buffer this optimizer owns) and the coefficient formed and
applied by the Adam launch that follows (``curla_adam_step*_clip``).  No host read, no allocation in the step.

``weight_decay`` with ``decoupled_weight_decay=True`` is ``torch.optim.AdamW``: every launch of a decaying group is the
``curla_adamw_*`` form of the launch it would have been, which multiplies each parameter by
``float32(1 - lr * weight_decay)`` -- one rounding -- in front of its Adam update.  Both live in
``param_groups`` and ``state_dict()`` as torch writes them and are read from the group at step time.  Coupled L2 decay
(``decoupled_weight_decay=False``) is not implemented.
"""
import math
import numbers

import torch

from ._lib import call, stream


def check_max_grad_norm(value):
    """``value`` as a clipping threshold: None (off) or a positive number (inf allowed: the coefficient is then always
    1) as a float; ValueError for a bool, a non-number, NaN or a value <= 0."""
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, numbers.Real) or math.isnan(value) or not value > 0:
        raise ValueError("max_grad_norm must be None or a positive number (inf allowed), got %r" % (value,))
    return float(value)


def check_weight_decay(value):
    """``value`` as a weight decay: a finite number >= 0 as a float; ValueError for a bool, a non-number, NaN, an
    infinite or a negative value."""
    if isinstance(value, bool) or not isinstance(value, numbers.Real) or not math.isfinite(value) or value < 0:
        raise ValueError("weight_decay must be a finite number >= 0, got %r" % (value,))
    return float(value)


def _scalar_adam_state(opt):
    """(param, group, state) of a plain ``torch.optim.Adam`` over one parameter (log_alpha's), the state initialised
    as torch's Adam initialises it (non-capturable: the step count lives on the host)."""
    g = opt.param_groups[0]
    p = g["params"][0]
    st = opt.state[p]
    if len(st) == 0:
        st["step"] = torch.tensor(0.0, dtype=torch.float32)
        st["exp_avg"], st["exp_avg_sq"] = torch.zeros_like(p), torch.zeros_like(p)
    return p, g, st


_NO_CLIP = (0, 0, 0.0, 0)  # the clip arguments (partials, n_partials, max_norm, stats) of an unclipped curla_adamw_* launch


class FlatAdam(torch.optim.Adam):
    CLIP_MAX_PARTIALS = 256  # include/curla_hip.h: one Adam workgroup sums a step's partials with one load per thread
    SQSUM_BLOCK = 1024       # elements a square-sum workgroup takes per trip of its grid-stride loop (256 x 16 bytes)

    def __init__(self, params, flat, gflat, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, *, weight_decay=0.0,
                 decoupled_weight_decay=False, max_grad_norm=None):
        """``params``: Parameters whose ``.data`` are views into ``flat`` and whose ``.grad`` (when not None) are the
        views at the same offsets of ``gflat``.  ``max_grad_norm``: None, or the threshold every step clips its live
        gradient's global norm to (a hyper-parameter, not state: it is neither in ``param_groups`` nor in
        ``state_dict()``).  ``weight_decay`` / ``decoupled_weight_decay``: torch.optim.Adam's, kept in the param group
        as torch keeps them; a non-zero decay must be the decoupled one (AdamW)."""
        weight_decay = check_weight_decay(weight_decay)
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                         decoupled_weight_decay=bool(decoupled_weight_decay))
        for g in self.param_groups:
            self._decay(g)
        self._flat, self._gflat = flat, gflat
        self._plist = [p for g in self.param_groups for p in g["params"]]
        base = flat.data_ptr()
        self._span = []
        for p in self._plist:
            off = (p.data_ptr() - base) // 4
            if p.dtype != torch.float32 or off < 0 or off + p.numel() > flat.numel() or not p.is_contiguous():
                raise ValueError("FlatAdam: every parameter must be a contiguous float32 view into the flat buffer")
            self._span.append((off, off + p.numel()))
        self._lo = min(a for a, _ in self._span)
        self._hi = max(b for _, b in self._span)
        self._m = torch.zeros(self._hi - self._lo, device=flat.device, dtype=torch.float32)
        self._v = torch.zeros_like(self._m)
        self._steps = [0] * len(self._plist)
        self._plans = {}
        # Captured update graphs (CurlSacAgent.enable_update_graphs).  While a graph is being captured, ``_dyn`` is the
        # device address of this optimizer's two step-dependent floats (hyper_floats): the launch reads them from there
        # when it runs, and the step counts are NOT advanced by the launching code (the graph manager advances them
        # once per replay: advance()).
        self._dyn = None
        # Clipping: the partial sums of squares of one step (float64, device) and where its (norm, coefficient) go --
        # ``clip_stats`` may be pointed at any two-float device tensor (CurlSacAgent: a row of grad_clip_stats).
        self._max_grad_norm = None
        self._clip_partials = None
        self.clip_stats = None
        self._shared_clip = None  # step_pair's two separate steps: (the pair's clip arguments, runs already scaled)
        self._touched = ()        # the runs [lo, hi) the last step() launched over
        self.max_grad_norm = max_grad_norm

    @property
    def max_grad_norm(self):
        return self._max_grad_norm

    @max_grad_norm.setter
    def max_grad_norm(self, value):
        value = check_max_grad_norm(value)
        if value is not None:
            if self._clip_partials is None:  # (here, not in the step: a captured step allocates nothing)
                dev = self._flat.device
                self._clip_partials = torch.zeros(self.CLIP_MAX_PARTIALS, device=dev, dtype=torch.float64)
                if self.clip_stats is None:
                    self.clip_stats = torch.zeros(2, device=dev, dtype=torch.float32)
        self._max_grad_norm = value

    # -- state kept in torch's format ------------------------------------------------------------------------
    def _views(self, i):
        a, b = self._span[i]
        shape = self._plist[i].shape
        return self._m[a - self._lo:b - self._lo].view(shape), self._v[a - self._lo:b - self._lo].view(shape)

    def _ensure_state(self, i):
        p = self._plist[i]
        st = self.state[p]
        if len(st) == 0:
            m, v = self._views(i)
            st["step"] = torch.tensor(0.0, dtype=torch.float32)
            st["exp_avg"], st["exp_avg_sq"] = m, v
        return st

    def state_dict(self):
        for i, p in enumerate(self._plist):
            if p in self.state and len(self.state[p]):
                self.state[p]["step"] = torch.tensor(float(self._steps[i]), dtype=torch.float32)
        return super().state_dict()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)  # deep-copies the tensors: move them back into the flat mirrors
        with torch.no_grad():
            for i, p in enumerate(self._plist):
                st = self.state.get(p)
                if not st:
                    self._steps[i] = 0
                    continue
                m, v = self._views(i)
                m.copy_(st["exp_avg"])
                v.copy_(st["exp_avg_sq"])
                st["exp_avg"], st["exp_avg_sq"] = m, v
                self._steps[i] = int(round(float(st["step"])))
                st["step"] = torch.tensor(float(self._steps[i]), dtype=torch.float32)

    @torch.no_grad()
    def reset_state(self):
        """Back to the state of a newly built optimizer without giving up an address (CurlSacAgent.reset_networks): the
        moment mirrors are FILLED with zeros in place on the current stream -- a fill, not a multiply: a NaN does not
        survive, and a captured graph keeps reading the same buffers --, every step count is 0, the launch plans stay.
        Parameters that have state keep its entries (views of the mirrors), with ``step`` 0."""
        self._m.zero_()
        self._v.zero_()
        self._steps = [0] * len(self._plist)
        for p in self._plist:
            st = self.state.get(p)
            if st:
                st["step"] = torch.tensor(0.0, dtype=torch.float32)

    def moment_addresses(self, off, n):
        """Device addresses of ``exp_avg`` / ``exp_avg_sq`` of the flat buffer's elements [off, off + n): the moment
        mirrors follow the flat layout from this optimizer's first parameter on (CurlSacAgent.redo_pass)."""
        if off < self._lo or off + n > self._hi:
            raise ValueError("FlatAdam: elements [%d, %d) are not all this optimizer's" % (off, off + n))
        return self._m.data_ptr() + 4 * (off - self._lo), self._v.data_ptr() + 4 * (off - self._lo)

    # -- captured graphs: the step-dependent factors as data ------------------------------------------------------
    def live_indices(self, live=None):
        """Indices of the parameters a step touches: ``live`` (an iterable of Parameters) or all of them."""
        if live is None:
            return range(len(self._plist))
        ids = {id(p) for p in live}
        return [i for i, p in enumerate(self._plist) if id(p) in ids]

    def next_step(self, live=None):
        """The 1-based count of the step the next ``step()`` takes for the parameters it touches (they share it in
        graph mode; parameters whose gradient is None at step time -- the convs under detach_encoder -- are not
        ``live`` and keep their own count, as in torch's Adam)."""
        counts = {self._steps[i] for i in self.live_indices(live)}
        if len(counts) != 1:
            raise RuntimeError("FlatAdam: the parameters of a captured step must share one step count")
        return counts.pop() + 1

    def hyper_floats(self, t):
        """(lr / (1 - beta1^t), sqrt(1 - beta2^t)) as the two float32 values curla_adam_step evaluates from ``step`` on
        the host: the same double arithmetic (libm pow), rounded to float once."""
        import numpy as np
        g = self.param_groups[0]
        b1, b2 = float(g["betas"][0]), float(g["betas"][1])
        return np.float32(float(g["lr"]) / (1.0 - b1 ** float(t))), np.float32((1.0 - b2 ** float(t)) ** 0.5)

    def advance(self, live=None, by=1):
        """One step's worth of host bookkeeping (what step() does besides launching) for the parameters the step
        touches; ``by=-1`` takes it back (a capture that failed after the bookkeeping)."""
        for i in self.live_indices(live):
            self._ensure_state(i)
            self._steps[i] += by

    # -- the step --------------------------------------------------------------------------------------------
    @staticmethod
    def _decay(group):
        """The group's decoupled weight decay, read at step time (0.0: none -- the launches are the plain ones);
        NotImplementedError for the Adam options the launches do not implement."""
        wd = group.get("weight_decay", 0)
        if group.get("amsgrad", False) or group.get("maximize", False):
            raise NotImplementedError("FlatAdam implements the options the learner uses: Adam and AdamW, no amsgrad, "
                                      "no maximize")
        if wd != 0 and not group.get("decoupled_weight_decay", False):
            raise NotImplementedError("FlatAdam: weight_decay is implemented in its decoupled form only (AdamW): pass "
                                      "decoupled_weight_decay=True; coupled L2 decay is not supported")
        return float(wd)

    def _plan(self, gi, group, live):
        """Contiguous runs [a, b) of the flat buffer covered by this group's live parameters (alignment padding
        between two adjacent parameters -- at most 3 floats, always zero gradient -- is bridged), each with the
        indices of its parameters."""
        idx0 = sum(len(g["params"]) for g in self.param_groups[:gi])
        items = sorted((self._span[idx0 + j] + (idx0 + j,) for j in range(len(group["params"])) if live[idx0 + j]))
        runs = []
        for a, b, i in items:
            if runs and a - runs[-1][1] <= 3 and a >= runs[-1][1]:
                runs[-1][1] = b
                runs[-1][2].append(i)
            else:
                runs.append([a, b, [i]])
        return runs

    def _segments(self, commit):
        """The flat runs [lo, hi) a step launches over, each with its group and the step count its parameters share:
        [(group, lo, hi, t)].  ``commit``: do the step's bookkeeping (state, step counts) as well."""
        live = tuple(p.grad is not None for p in self._plist)
        plans = self._plans.get(live)
        if plans is None:
            base = self._gflat.data_ptr()
            for i, p in enumerate(self._plist):
                if live[i] and (p.grad.data_ptr() - base) // 4 != self._span[i][0]:
                    raise ValueError("FlatAdam: a gradient is not the flat gradient buffer's view of its parameter")
            plans = self._plans[live] = [self._plan(gi, g, live) for gi, g in enumerate(self.param_groups)]
        segs = []
        for group, runs in zip(self.param_groups, plans):
            self._decay(group)
            for a, b, members in runs:
                # parameters of one run normally share their step count; split the run where they do not
                k = 0
                while k < len(members):
                    t = self._steps[members[k]]
                    e = k
                    while e + 1 < len(members) and self._steps[members[e + 1]] == t:
                        e += 1
                    lo = a if k == 0 else self._span[members[k]][0]
                    hi = b if e == len(members) - 1 else self._span[members[e]][1]
                    if not commit:
                        pass
                    elif self._dyn is None:
                        for i in members[k:e + 1]:
                            self._ensure_state(i)
                            self._steps[i] = t + 1
                    elif len(plans) != 1 or len(runs) != 1 or e != len(members) - 1 or k != 0:
                        raise RuntimeError("FlatAdam: a captured step must be ONE run with one step count")
                    segs.append((group, lo, hi, t))
                    k = e + 1
        return segs

    def _sqsum(self, runs, s):
        """One square-sum launch per run [lo, hi) of the flat gradient, into disjoint slots of the partials buffer;
        returns the clip arguments of the Adam launches of the step: (partials, their total count, max_norm, stats).
        A run's workgroup count is a function of its length alone, capped so that the step's partials stay within
        CLIP_MAX_PARTIALS: the norm depends only on the gradient's bytes and the layout of the runs."""
        if len(runs) > self.CLIP_MAX_PARTIALS:
            raise NotImplementedError("FlatAdam: a clipped step over more than %d runs" % self.CLIP_MAX_PARTIALS)
        cap = self.CLIP_MAX_PARTIALS // len(runs)
        base, count = self._clip_partials.data_ptr(), 0
        for lo, hi in runs:
            nb = max(1, min(cap, -(-(hi - lo) // self.SQSUM_BLOCK)))
            call("curla_grad_sqsum", self._gflat.data_ptr() + 4 * lo, hi - lo, base + 8 * count, nb, s)
            count += nb
        return base, count, self._max_grad_norm, self.clip_stats.data_ptr()

    @staticmethod
    def _hyper(g, t, wd=None):
        """(lr, beta1, beta2, eps, step) of a launch; a curla_adamw_* launch (``wd`` not None) takes weight_decay
        behind eps."""
        return (float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"])) + \
            (() if wd is None else (wd,)) + (t + 1,)

    def _adam_args(self, lo, hi, t, g, wd=None):
        return (self._flat.data_ptr() + 4 * lo, self._gflat.data_ptr() + 4 * lo, self._m.data_ptr() + 4 * (lo - self._lo),
                self._v.data_ptr() + 4 * (lo - self._lo), hi - lo) + self._hyper(g, t, wd) + (self._dyn,)

    @staticmethod
    def _launch(form, args, wd, clip, s):
        """One Adam launch: ``curla_adam_<form>`` / ``curla_adam_<form>_clip`` as ever without weight decay (``wd``
        None), ``curla_adamw_<form>`` (its clip arguments empty when the launch does not clip) with it; ``args``
        carry the decay already (_hyper)."""
        if wd is not None:
            call("curla_adamw_" + form, *args, *(_NO_CLIP if clip is None else clip), s)
        elif clip is None:
            call("curla_adam_" + form, *args, s)
        else:
            call("curla_adam_" + form + "_clip", *args, *clip, s)

    @staticmethod
    def _pieces(lo, hi, done):
        """[lo, hi) cut at the borders of the runs in ``done``: (a, b, inside one of them?) in order."""
        cuts = sorted({lo, hi} | {x for r in done for x in r if lo < x < hi})
        return [(a, b, any(c <= a and b <= d for c, d in done)) for a, b in zip(cuts[:-1], cuts[1:])]

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        segs = self._segments(commit=True)
        self._touched = tuple((lo, hi) for _, lo, hi, _ in segs)
        s = stream()
        clip, done = None, ()
        if self._max_grad_norm is not None and segs:
            if self._shared_clip is not None:  # step_pair's separate steps: ONE norm for both, each element scaled once
                clip, done = self._shared_clip
            else:
                clip = self._sqsum(self._touched, s)  # one norm over all the runs of the step
        for group, lo, hi, t in segs:
            wd = self._decay(group) or None
            for a, b, scaled in self._pieces(lo, hi, done):
                self._launch("step", self._adam_args(a, b, t, group, wd), wd, None if scaled else clip, s)
        return loss

    # -- two optimizers, one pass ------------------------------------------------------------------------------
    def _single_run(self):
        """(lo, hi, step, group) when every parameter is live, they form ONE run of the flat buffer and share their
        step count; else None."""
        if len(self.param_groups) != 1 or any(p.grad is None for p in self._plist):
            return None
        live = (True,) * len(self._plist)
        plans = self._plans.get(live)
        if plans is None:
            plans = self._plans[live] = [self._plan(0, self.param_groups[0], live)]
        runs = plans[0]
        if len(runs) != 1 or len(set(self._steps)) != 1:
            return None
        g = self.param_groups[0]
        try:
            self._decay(g)
        except NotImplementedError:  # (the step the caller then takes raises it)
            return None
        return runs[0][0], runs[0][1], self._steps[0], g

    @staticmethod
    @torch.no_grad()
    def step_pair(first, second):
        """``first.step(); second.step()`` for two FlatAdams over the same flat buffer where first's parameters are the
        tail of second's (the encoder inside [CURL.W | encoder]): one launch that applies both steps per element in
        that order.  Anything else (partial gradients, unequal step counts, other layouts) takes the two steps.
        With weight decay in either, each optimizer's factor goes in front of its own step (``curla_adamw_step2``).
        With ``max_grad_norm`` set (both must carry the same value) the gradient is clipped ONCE, by its norm over the
        second optimizer's run, and both steps consume the clipped gradient -- in the two separate steps as well
        (_two_steps)."""
        plain = isinstance(first, FlatAdam) and isinstance(second, FlatAdam) and first._flat is second._flat and \
            first._gflat is second._gflat and "step" not in vars(first) and "step" not in vars(second)  # (a step
        # replaced on the instance -- tests do that to look at gradients before they are consumed -- is respected)
        ra, rb = (first._single_run(), second._single_run()) if plain else (None, None)
        if ra is None or rb is None or ra[1] != rb[1] or ra[0] < rb[0] or first.max_grad_norm != second.max_grad_norm:
            FlatAdam._two_steps(first, second)
            return
        (a0, a1, ta, ga), (b0, b1, tb, gb) = ra, rb
        if first._dyn is None:
            for opt in (first, second):
                for i in range(len(opt._plist)):
                    opt._ensure_state(i)
                    opt._steps[i] += 1
        elif second._dyn != first._dyn + 8:
            raise RuntimeError("FlatAdam.step_pair: the second optimizer's captured factors must follow the first's")
        flat, gflat = first._flat, first._gflat
        wda, wdb = first._decay(ga), second._decay(gb)
        if not (wda or wdb):  # (curla_adamw_step2 takes both decays, one of which may be 0)
            wda = wdb = None
        args = (flat.data_ptr() + 4 * b0, gflat.data_ptr() + 4 * b0,
                first._m.data_ptr() + 4 * (a0 - first._lo), first._v.data_ptr() + 4 * (a0 - first._lo),
                second._m.data_ptr() + 4 * (b0 - second._lo), second._v.data_ptr() + 4 * (b0 - second._lo), b1 - b0,
                a0 - b0) + FlatAdam._hyper(ga, ta, wda) + FlatAdam._hyper(gb, tb, wdb) + (first._dyn,)
        s = stream()
        clip = None if second.max_grad_norm is None else second._sqsum([(b0, b1)], s)
        FlatAdam._launch("step2", args, wda, clip, s)

    @staticmethod
    def _two_steps(first, second):
        """``first.step(); second.step()``.  When both are FlatAdams over one gradient buffer that clip to the same
        ``max_grad_norm`` and every run first steps over lies inside a run of second's, the two steps are ONE clipped
        step, as the fused launch is: one norm, over second's runs; first's step scales its runs by the coefficient
        (and writes them back); second's step scales only what first has not -- its launches over first's runs are
        the unclipped ones, so no element is scaled twice.  Otherwise each step clips (or not) on its own."""
        shared = isinstance(first, FlatAdam) and isinstance(second, FlatAdam) and first._gflat is second._gflat and \
            first.max_grad_norm is not None and first.max_grad_norm == second.max_grad_norm
        if shared:
            runs1 = [(lo, hi) for _, lo, hi, _ in first._segments(commit=False)]
            runs2 = [(lo, hi) for _, lo, hi, _ in second._segments(commit=False)]
            shared = bool(runs1) and all(any(c <= a and b <= d for c, d in runs2) for a, b in runs1)
        if not shared:
            first.step()
            second.step()
            return
        clip = second._sqsum(runs2, stream())
        try:
            first._shared_clip = (clip, ())
            first.step()
            second._shared_clip = (clip, first._touched)
            second.step()
        finally:
            first._shared_clip = second._shared_clip = None

    # -- this optimizer's step and the target copy's soft update, one launch ---------------------------------------
    @staticmethod
    @torch.no_grad()
    def step_with_lerp(opt, target_flat, lo, hi, split, tau_a, tau_b):
        """``opt.step()`` followed by ``target[lo:hi] <- tau * flat[lo:hi] + (1 - tau) * target[lo:hi]`` (tau_a for
        [lo, lo + split), tau_b behind) in ONE launch, when ``opt`` is a FlatAdam whose live parameters are exactly the
        flat run [lo, hi) with one step count and a ``step`` that has not been replaced.  Returns False -- having done
        nothing -- when that does not hold: the caller then takes the two steps."""
        if not isinstance(opt, FlatAdam) or "step" in vars(opt):
            return False
        run = opt._single_run()
        # (the run ends with its last parameter, the announced block may include up to 3 floats of alignment padding
        # behind it: zeros in both copies, which a soft update leaves as they are)
        if run is None or run[0] != lo or not (run[1] <= hi <= run[1] + 3):
            return False
        _, hi, t, g = run
        if opt._dyn is None:
            for i in range(len(opt._plist)):
                opt._ensure_state(i)
                opt._steps[i] = t + 1
        wd = opt._decay(g) or None
        args = opt._adam_args(lo, hi, t, g, wd) + (target_flat.data_ptr() + 4 * lo, split, float(tau_a),
                                                   float(1.0 - tau_a), float(tau_b), float(1.0 - tau_b))
        s = stream()
        opt._launch("step_lerp", args, wd, None if opt.max_grad_norm is None else opt._sqsum([(lo, hi)], s), s)
        return True

    # -- this optimizer and a float64 scalar's, one launch -----------------------------------------------------------
    @staticmethod
    @torch.no_grad()
    def step_with_scalar(first, scalar_opt):
        """``first.step(); scalar_opt.step()`` where ``scalar_opt`` is a plain ``torch.optim.Adam`` over ONE float64
        one-element parameter on the device (log_alpha): its step rides in first's launch.  Anything else (first not a
        single flat run, a replaced ``step``, no gradient, other Adam options) takes the two steps."""
        groups = scalar_opt.param_groups
        p = groups[0]["params"][0] if len(groups) == 1 and len(groups[0]["params"]) == 1 else None
        g = groups[0] if p is not None else {}
        ok = isinstance(first, FlatAdam) and type(scalar_opt) is torch.optim.Adam and p is not None and \
            "step" not in vars(first) and "step" not in vars(scalar_opt) and p.dtype == torch.float64 and \
            p.numel() == 1 and p.is_cuda and p.grad is not None and p.grad.dtype == torch.float64 and \
            not (g.get("weight_decay", 0) or g.get("amsgrad") or g.get("maximize") or g.get("capturable") or
                 g.get("fused") or g.get("differentiable"))
        run = first._single_run() if ok else None
        if run is None:
            first.step()
            scalar_opt.step()
            return
        st = _scalar_adam_state(scalar_opt)[2]
        if st["step"].is_cuda:
            st["step"] = st["step"].cpu()
        t64 = int(round(float(st["step"]))) + 1
        lo, hi, t, grp = run
        frozen = first._dyn is not None  # (captured graph: the manager advances both step counts per replay)
        if not frozen:
            for i in range(len(first._plist)):
                first._ensure_state(i)
                first._steps[i] = t + 1
        wd = first._decay(grp) or None  # (the flat run's: log_alpha's optimizer is its own and is never decayed)
        args = first._adam_args(lo, hi, t, grp, wd) + (
            p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), float(g["lr"]),
            float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), t64, getattr(scalar_opt, "_curla_dyn64", None))
        s = stream()  # (the norm is the flat run's: the scalar is not clipped)
        first._launch("step_scalar64", args, wd, None if first.max_grad_norm is None else first._sqsum([(lo, hi)], s), s)
        if not frozen:
            st["step"] = torch.tensor(float(t64), dtype=torch.float32)


__all__ = ["FlatAdam", "check_max_grad_norm", "check_weight_decay"]
