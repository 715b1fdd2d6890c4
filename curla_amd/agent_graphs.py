"""CurlSacAgent's captured update graphs: a hipGraph per kind of step, replayed with the per-update values as data."""
import contextlib
import gc
import warnings

import numpy as np
import torch

from .networks import _device_generator
from .optim import FlatAdam, _scalar_adam_state


@contextlib.contextmanager
def _collector_held_off():
    """Python's cyclic collector off for the length of a graph capture, and back as it was -- also when the capture
    raises.  A collection that starts inside the captured region finalizes whatever dead cycles the process holds,
    other agents' ``torch.cuda.CUDAGraph`` objects among them, and finalizers that call the runtime are not legal under
    a capturing stream: a whole-suite run on an MI355X aborted in exactly that place ("Found on the
    way").  Nothing is collected here; what is dead stays so until the capture has ended."""
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was_enabled:
            gc.enable()


class _NullLog:
    """What a captured update logs to: nothing (logging steps are never captured)."""

    def log(self, *a, **k):
        pass

    log_histogram = log_param = log_image = log


class _UpdateGraphsMixin:
    """CurlSacAgent's update-graph methods; the state they use is the agent's (``_graphs``, ``_graph_cap``: __init__)."""

    def enable_update_graphs(self, replay_buffer, warm=1, depth=2):
        """Replay ``update()`` from captured hipGraphs (kernels only enqueue, take no host syncs and
        allocate nothing, so a whole update can be captured).  One graph per KIND of step -- (actor phase?, target soft
        update?, CURL phase?): with train.py's frequencies that is "even" and "odd" -- is captured the first time the
        kind comes up after ``warm`` eager updates of it, and replayed from then on: the host's work per update shrinks
        to drawing the indices (NumPy, the reference's stream and order), writing them and ~80 bytes of per-update
        control values into a pinned block, and one graph launch.  What changes from update to update is DATA the
        captured kernels read on the device: the minibatch's indices / crop offsets (as before), the Philox stream
        position of each policy-noise draw and every optimizer's two step-dependent Adam factors (curla_hip.h: the
        ``rng_dev`` / ``dyn`` arguments); the block's staging kernel is the first node of the graph.
        A ``ReplayBuffer(..., staged_aug=True)`` with ColorJiggle, NoisyCover or RandomConv is covered the same way: the host draws
        the three tensors' parameters per replay (``draw_aug``: torch's CPU generator / NumPy, in the eager order; for
        NoisyCover also the Philox positions of the three in-kernel noise draws, taken from the device generator IN
        FRONT of the two policy draws, as an eager staged update takes them) and writes them into the block behind the
        indices; the jitter / cover / convolution launches are nodes that read the block's device copy.  A ``dedup_frames`` buffer
        needs no flag: its gather_stacks launches are nodes that read the frame-id table when the graph runs.
        (ColorJiggle's arithmetic stays PARITY UNPINNED, graphed or not: augmentations.py.)
        ``depth`` graphs are captured per kind, each with its own pinned block, and used in rotation: the host may then
        prepare update n + 2 depth - 1 while the GPU still reads the block of update n (with one graph per kind it would
        wait for the replay two updates back before every update).
        Results are bit-identical to the eager path (tests/test_gpu_graph.py).  Steps the graphs do not cover run
        eagerly, in any mix: logging steps (``step % log_interval == 0``: they compute extra scalars), histogram /
        image recording steps, ``only_cpc``, other replay buffers, data-parallel runs on a backend other than RCCL.  A
        float augmentation on a buffer built WITHOUT ``staged_aug=True`` is refused here (its parameters go through a
        pinned block and a copy of their own per call).  Data-parallel updates over RCCL
        ARE captured, collectives included (round 5; the replica check stays on the host, in front of the replay).
        Values the graphs hold as kernel arguments (discount, taus, betas / eps, detach_encoder, the update
        frequencies, the data-parallel group and schedule, ``max_grad_norm``, ``critic_dropout``,
        ``critic_drop_quantiles``, ``critic_value_range``, ``critic_bin_sigma``, ``n_step`` and ``discount`` of an n-step
        replay buffer) are fingerprinted at capture: editing one of them drops the graphs and they are captured again;
        so does ``load_checkpoint``.  A capture that raises leaves the agent's
        state untouched and that update runs eagerly.
        ``utd_ratio = G > 1``: a call replays the critic-only kind's graph (actor=False, soft, cpc=False) G-1 times -- the
        graph an ordinary critic-only step captures, each replay on the next block of the kind's rotation -- and then the
        step's own kind; a call that runs eagerly (above) runs all its sub-steps eagerly.  No graph holds the ratio: it
        is not fingerprinted and may be edited between calls.
        Weight decay (``set_weight_decay``): a captured Adam launch holds its factor ``float32(1 - lr * weight_decay)``
        by value, so for an optimizer that decays, ``lr`` is fingerprinted too -- an lr schedule on a decaying optimizer
        re-captures at every change of lr (without weight decay lr travels as data and never re-captures)."""
        if self.device.type != "cuda":
            raise RuntimeError("update graphs need the HIP device")
        if not getattr(replay_buffer, "graph_supported", lambda: False)():
            raise ValueError("enable_update_graphs: this replay buffer / augmentation is not graph-replayable "
                             "(covered: RandomCrop, RandomShift, RandomCutout, RandomTranslate or identity, plain storage with both rings in one "
                             "allocation or dedup_frames storage -- RandomFlip, RandomRotate, RandomGrayscale and RandomAffine like them; ColorJiggle / NoisyCover / RandomConv "
                             "only on a ReplayBuffer constructed with staged_aug=True; pinned index slots, i.e. not "
                             "CURLA_STAGE_COPY=1; not a prioritized=True buffer, whose draw and priority update are not "
                             "nodes of the graphs)")
        opts = (self.critic_optimizer, self.actor_optimizer, self.encoder_optimizer, self.cpc_optimizer)
        if not all(isinstance(o, FlatAdam) and "step" not in vars(o) for o in opts) or \
                type(self.log_alpha_optimizer) is not torch.optim.Adam or self._noise_launch:
            raise ValueError("enable_update_graphs needs the FlatAdam optimizers and the in-kernel policy noise")
        self._graphs = {}
        self._graph_rb = replay_buffer
        self._graph_warm = int(warm)
        self._graph_depth = max(1, int(depth))
        self._graph_seen = {}
        self._graph_key_at_capture = None

    def disable_update_graphs(self):
        self._graphs = None

    def _graph_kind(self, step):
        return (step % self.actor_update_freq == 0, step % self.critic_target_update_freq == 0,
                (not self.pixel_sac) and step % self.cpc_update_freq == 0)

    def _graph_usable(self, replay_buffer, step, only_cpc):
        # data parallel: RCCL collectives are capturable (they are enqueued on streams like kernels); a backend that is
        # staged through the host (gloo) is not
        # (_dp_avg: the group's backend is RCCL; every other backend takes the sum-and-divide / staged path)
        return (replay_buffer is self._graph_rb and not only_cpc and not (self._dp_active and not self._dp_avg)
                and not self._records(step) and step % self.log_interval != 0 and self.training
                and not self._redo_due(step, only_cpc))  # (a redo step's update runs eagerly: DESIGN.md 7j)

    def _graph_live(self, opt):
        """The parameters ``opt``'s step touches in a captured update (None: all).  Under detach_encoder the critic's
        convs have no gradient at step time (curl_sac.py:358): Adam skips them and their step counts stay behind."""
        if opt is self.critic_optimizer and self.detach_encoder:
            convs = {id(p) for m in self.critic.encoder.convs for p in (m.weight, m.bias)}
            return [p for p in opt._plist if id(p) not in convs]
        return None

    def _graph_key(self):
        """Everything a captured graph holds BY VALUE (kernel arguments baked in at capture): a change of any of it
        makes the captured graphs stale -- they are dropped and re-captured (``lr`` travels as data and is not here,
        except for a param group with weight decay: its launch holds 1 - lr * weight_decay by value)."""
        opts = (self.critic_optimizer, self.actor_optimizer, self.encoder_optimizer, self.cpc_optimizer,
                self.log_alpha_optimizer)
        hyper = tuple((float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g.get("weight_decay", 0))) +
                      ((float(g["lr"]),) if g.get("weight_decay", 0) != 0 else ())  # (0: the key without weight decay)
                      for o in opts for g in o.param_groups)
        return (float(self.discount), float(self.critic_tau), float(self.encoder_tau), bool(self.detach_encoder),
                bool(self.pixel_sac), float(self.target_entropy), float(self.actor.log_std_min),
                float(self.actor.log_std_max), self.actor_update_freq, self.critic_target_update_freq,
                self.cpc_update_freq, self._dp_active, self._dp_overlap, id(self._dp_group) if self._dp_active else 0,
                hyper, self._graph_rb_key(), self._max_grad_norm) + \
            ((float(self.critic_dropout),) if self.critic_dropout else ()) + \
            ((("aug_views", 2),) if self.aug_views == 2 else ()) + \
            self._critic_head_graph_key() + self._policy_graph_key() + self._cpc_graph_key()
        # (a feature that is off adds nothing: the key of an agent without the keyword.  The critic head's entry is the
        # quantiles', which two views are not combined with, or the bins', behind the views' -- the order as it was)

    def _graph_rb_key(self):
        """(n_step, discount, pos_offset, n_envs) of the graphs' replay buffer: its staging launch holds them by value
        (n_envs as the stride of the chain walks)."""
        rb = getattr(self, "_graph_rb", None)
        n = getattr(rb, "n_step", 1)
        views = getattr(rb, "aug_views", 1)  # (held by no graph: the entry makes a changed buffer re-capture)
        return ((n, float(rb.discount)) if n > 1 else (1, None)) + \
            (getattr(rb, "pos_offset", 0), getattr(rb, "n_envs", 1)) + ((("aug_views", views),) if views == 2 else ())

    def _graph_tail(self, kind, B):
        """The 80 control bytes of one graphed update (ReplayBuffer.GRAPH_TAIL) -- and the host-side bookkeeping of
        everything they stand for: the torch generator's offset moves on as _noise() would move it, every optimizer that
        steps in this kind of update counts its step.  Only called once the update's graph exists (a capture that failed
        has run eagerly instead), so there is nothing to take back."""
        do_actor, _, do_cpc = kind
        u64 = np.zeros(4, dtype=np.uint64)
        gen = _device_generator(self.device)
        n = B * self.action_dim
        for j in range(2 if do_actor else 1):  # critic-phase draw, then the actor phase's (curl_sac.py:352, 378)
            off = gen.get_offset()
            gen.set_offset(off + 4 * ((n + 3) // 4))
            u64[2 * j], u64[2 * j + 1] = np.uint64(gen.initial_seed() & (2 ** 64 - 1)), np.uint64(off // 4)
        f64 = np.zeros(2, dtype=np.float64)
        f32 = np.zeros(8, dtype=np.float32)
        steps = [(0, self.critic_optimizer)]
        if do_actor:
            steps.append((1, self.actor_optimizer))
            _, g, st = _scalar_adam_state(self.log_alpha_optimizer)
            t64 = int(round(float(st["step"]))) + 1
            b1, b2 = float(g["betas"][0]), float(g["betas"][1])
            f64[0], f64[1] = float(g["lr"]) / (1.0 - b1 ** float(t64)), (1.0 - b2 ** float(t64)) ** 0.5
            st["step"] = torch.tensor(float(t64), dtype=torch.float32)
        if do_cpc:
            steps += [(2, self.encoder_optimizer), (3, self.cpc_optimizer)]
        for slot, opt in steps:
            live = self._graph_live(opt)
            f32[2 * slot], f32[2 * slot + 1] = opt.hyper_floats(opt.next_step(live))
            opt.advance(live)
        return u64.tobytes() + f64.tobytes() + f32.tobytes()

    GRAPH_CAPTURE_RETRIES = 3  # failed captures (on any rank) after which update graphs are switched off

    def _graph_capture_agreed(self, ok):
        """True when the capture succeeded on EVERY rank of the data-parallel group (one rank: ``ok`` itself)."""
        if not (self._dp_active and self._dp_world > 1):
            return bool(ok)
        import torch.distributed as dist
        flag = torch.tensor([1 if ok else 0], dtype=torch.int32, device=self.device)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=self._dp_group)
        return bool(int(flag.item()))

    def _drop_graphs(self):
        """Forget the captured graphs (they are re-captured after ``warm`` further eager updates of each kind)."""
        if self._graphs is not None:
            torch.cuda.synchronize()
            self._graphs = {}
            self._graph_seen = {}
            self._graph_key_at_capture = None

    def _update_graphed(self, rb, L, step):
        self._check_n_step(rb)
        self._check_aug_views(rb)
        key = self._graph_key()
        if self._graphs and key != self._graph_key_at_capture:
            self._drop_graphs()  # a value the graphs hold as a kernel argument has been edited since the capture
        kind = self._graph_kind(step)
        leading = self.utd_ratio - 1
        if leading == 0:
            return self._graphed_substep(rb, step, kind, key, lambda: self._update_eager(rb, L, step))
        # utd_ratio > 1: the critic-only kind's graph G-1 times -- the one an ordinary critic-only step captures and
        # replays, positive's sampling nodes included --, then the step's own kind.  Every sub-step takes the next turn
        # of its kind's ring, so consecutive replays of one kind read different blocks, and graph_write waits for the
        # replay that last read a block before the host rewrites it.
        lead_kind = (False, kind[1], False)
        for k in range(leading):
            self._graphed_substep(rb, step, lead_kind, key, lambda k=k: self._substep_eager(
                rb, None, step, leading=True, first=k == 0), leading=True, first=k == 0)
        self._graphed_substep(rb, step, kind, key, lambda: self._substep_eager(rb, L, step, first=False), first=False)

    def _graphed_substep(self, rb, step, kind, key, eager, leading=False, first=True):
        """One minibatch of a graphed update: the replay of ``kind``'s graph (captured here when its turn has none) or,
        while the kind is warming up and where a capture fails, ``eager()``."""
        if self._graphs is None:  # (an earlier sub-step of this call has given the graphs up)
            return eager()
        seen = self._graph_seen.get(kind, 0)
        self._graph_seen[kind] = seen + 1
        if seen < self._graph_warm:  # (first uses allocate workspaces and set kernel attributes: not capturable)
            return eager()
        ring = self._graphs.setdefault(kind, [])
        turn = (seen - self._graph_warm) % self._graph_depth
        if turn >= len(ring):
            ring.append(dict(slot=sum(len(r) for r in self._graphs.values()), graph=None))
        st = ring[turn]
        B = rb.batch_size
        if st["graph"] is None:
            # capture FIRST, commit the host's bookkeeping (NumPy draw, generator offset, step counts) only once the
            # capture has succeeded: nothing inside the captured region draws from NumPy, torch's CPU generator or
            # moves the device generator (draw_indices / draw_aug / _graph_tail run after it), so a capture that raises (a first-use attribute call after an
            # option change, a HIP call from another thread) has touched only the phase-to-phase hints below, which are
            # reset, and this update runs eagerly
            blk = rb.graph_block(st["slot"])
            base = blk["dev"].data_ptr() + blk["tail"]
            dyn = {self.critic_optimizer: base + 48, self.actor_optimizer: base + 56, self.encoder_optimizer: base + 64,
                   self.cpc_optimizer: base + 72}
            self._graph_cap = dict(rng=(base, base + 16), n_noise=0)
            for opt, addr in dyn.items():
                opt._dyn = addr
            self.log_alpha_optimizer._curla_dyn64 = base + 32
            null = _NullLog()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            err = None
            try:
                with _collector_held_off(), torch.cuda.graph(graph, capture_error_mode="thread_local"):
                    if leading:
                        self._leading_phases(rb.graph_refs(st["slot"]), step)
                    else:
                        self._update_phases(rb.graph_refs(st["slot"]), null, step)
            except Exception as e:  # noqa: BLE001
                err = e
                # what the phases set for each other and had no chance to clear; collectives enqueued under the failed
                # capture are dropped without waiting for them (_graph_cap is still set)
                self._reset_handover()
            finally:
                self._graph_cap = None
                for opt in dyn:
                    opt._dyn = None
                self.log_alpha_optimizer._curla_dyn64 = None
            # data parallel: every rank captures at the same step; ONE rank replaying while another runs eagerly would
            # still pair up collective for collective, but the ranks would sit on different schedules indefinitely with
            # nothing checking it -- so the outcome is agreed on (one host-side flag, at capture time only)
            ok_everywhere = self._graph_capture_agreed(err is None)
            if not ok_everywhere:
                self._graph_failures = getattr(self, "_graph_failures", 0) + 1
                where = "on this rank" if err is not None else "on another rank"
                give_up = self._graph_failures >= self.GRAPH_CAPTURE_RETRIES
                warnings.warn(f"curla_amd: capturing the update graph of {kind} failed {where} ({err!r}); this update "
                              "runs eagerly" + (" and update graphs are now disabled (every rank of the group does the same)"
                                                if give_up else " and the capture is tried again next time"),
                              RuntimeWarning, stacklevel=4)
                if give_up:
                    self._graphs = None
                else:
                    self._graph_seen[kind] = seen  # (the slot keeps its empty entry: the same turn captures again)
                return eager()
            st["graph"] = graph
            self._graph_key_at_capture = key
        # the eager order of host draws: indices, then the three tensors' augmentation parameters (staged_aug: NoisyCover
        # reserves its noise counters on the device generator here), then the policy draws of _graph_tail
        idxs, offs = rb.draw_indices()
        aug = rb.draw_aug()
        tail = self._graph_tail(kind, B)
        blk = rb.graph_write(st["slot"], idxs, offs, tail, aug)
        if self._replica_check_due(step, first):
            self.check_replicas()
        st["graph"].replay()
        if blk["event"] is None:
            blk["event"] = torch.cuda.Event()
        blk["event"].record()
