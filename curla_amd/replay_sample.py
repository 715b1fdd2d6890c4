"""Read side of ``ReplayBuffer`` (replay.py): the host draws, a minibatch's block (``block_layout``), its upload and
staging, where the loaders read it from (``_sources``) and its assembly into handles, the slots of captured update
graphs, and prioritized replay's handle and methods."""
import collections
import os

import numpy as np
import torch

from . import ops
from .replay_write import _lib_tracing


def _checked_discount(d):
    """``discount`` of an n-step ReplayBuffer as a float; ValueError unless it is a number in (0, 1]."""
    if isinstance(d, bool) or not isinstance(d, (int, float, np.floating, np.integer)) or not 0.0 < float(d) <= 1.0:
        raise ValueError("n_step > 1 needs discount, a float in (0, 1] (the agent's), got %r" % (d,))
    return float(d)


def _checked_per(alpha, beta, eps):
    """(per_alpha, per_beta, per_eps) of a prioritized ReplayBuffer as floats; ValueError unless 0 <= alpha,
    0 <= beta <= 1 and eps > 0."""
    vals = []
    for name, v in (("per_alpha", alpha), ("per_beta", beta), ("per_eps", eps)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)):
            raise ValueError("%s must be a number, got %r" % (name, v))
        vals.append(float(v))
    a, b, e = vals
    if not (0.0 <= a < float("inf") and 0.0 <= b <= 1.0 and 0.0 < e < float("inf")):
        raise ValueError("prioritized replay needs 0 <= per_alpha, 0 <= per_beta <= 1 and per_eps > 0, got %r, %r, %r"
                         % (alpha, beta, eps))
    return a, b, e


class PerHandle:
    """What a prioritized minibatch hands the learner (``obs.per``, the way ``ObsRef.pair`` rides on the obs handle):
    ``rows`` int64 [B] and ``prob`` float32 [B], views of the minibatch's device block -- the drawn ring rows and their
    sampling probabilities --, and ``td_update``, the priority half of a critic update.  Valid as long as the
    minibatch's pixel handles are."""

    __slots__ = ("buffer", "rows", "prob", "guard")

    def __init__(self, buffer, rows, prob, guard):
        self.buffer, self.rows, self.prob, self.guard = buffer, rows, prob, guard

    def td_update(self, q, twin_stride, target_q, dq, loss, w, value):
        """Behind the critic's TD loss launch (``q``, ``target_q`` and the unweighted ``dq`` are there): the importance
        weights into ``w``, ``dq`` scaled by them in place, the weighted loss into ``loss``, and the rows' new stored
        values ``(0.5 (|q1 - t| + |q2 - t|) + per_eps) ** per_alpha`` into ``value`` and from there into the buffer (a row
        drawn twice keeps the larger one).  Two entry points: curla_per_td, curla_per_set.
        The rows are those of the DRAW: call this before any ``add`` that may overwrite one of them (``agent.update()``
        does).  An add between the draw and this call that lands on a drawn row would see its fresh transition's
        maximum priority replaced by the old transition's TD error; the guard only notices a recycled sample slot."""
        g = self.guard
        if g is not None and g[0][g[1]] != g[2]:
            raise RuntimeError("stale minibatch: the replay buffer has recycled this sample's device block")
        rb = self.buffer
        alpha, beta, eps = _checked_per(rb.per_alpha, rb.per_beta, rb.per_eps)
        B = rb.batch_size
        ops.per_td(q, twin_stride, target_q, self.prob, beta, eps, alpha, B, dq, loss, w, value)
        ops.per_set(rb._per_s, rb._per_sums, rb._per_max, B, rows=self.rows, values=value)


# what ReplayBuffer._sources returns
_Sources = collections.namedtuple("_Sources", "both idx2 h2 w2 tensors off words pos2 run period")


class _ReplaySampleMixin:
    """ReplayBuffer's sampling routes; the state they use is the buffer's (allocated by ``_alloc_sample_slots``)."""

    def _alloc_sample_slots(self):
        """Sampling's staging: the pinned index slots, and per sample slot the device block, the scalar buffer and the
        minibatch stores of a frame store or a "scratch" augmentation."""
        B, A, frame, dev = self.batch_size, self._n_act, self._frame, self.device
        pin = dev.type == "cuda"
        # the host may run several updates ahead of the GPU: a small ring of pinned slots, each guarded by an
        # event, keeps an index upload's source intact until its async copy has executed
        # (an event record is a packet of its own in the stream, ~5 us: one per EVENT_EVERY uses, and a slot is
        # re-written only after the first event recorded at or after its last use has completed)
        self._n_slots, self._slot_use = 16, 0
        # frame indices (obs | next_obs) + the six crop-offset rows (+ staged_aug: the three tensors' parameters)
        self._layout = self.block_layout()
        nbytes = self._layout["nbytes"]
        self._h_index = torch.empty((self._n_slots, nbytes), dtype=torch.uint8, pin_memory=pin)
        self._slot_events = {}
        # pinned slots are read by the GPU in place (ops.sample_stage): no copy-engine transfer in front of an update
        # (a prioritized block goes by the copy: the draw is a kernel of its own between the block and the gathers)
        self._h_index_dev = ([ops.host_device_pointer(self._h_index[k]) for k in range(self._n_slots)]
                             if pin and os.environ.get("CURLA_STAGE_COPY", "0") != "1" and not self.prioritized else None)
        # every minibatch gets its own device index block (and, de-duplicated, its own assembled stacks), so the
        # references of one sample stay valid while the next one is drawn (N_SAMPLE_SLOTS alive at a time)
        self._d_index = torch.empty((self.N_SAMPLE_SLOTS, nbytes), dtype=torch.uint8, device=dev)
        self._d_scal = torch.empty((self.N_SAMPLE_SLOTS, B * (A + 2)), dtype=torch.float32, device=dev)
        self._sample_gen = [0] * self.N_SAMPLE_SLOTS
        self._sample_slot = -1
        if self.dedup_frames:
            # (obs stacks | next_obs stacks) of a minibatch, contiguous: also one [2B] ring for ObsRef.pair
            # (pos_offset > 0: | the positives' stacks, [3B])
            self._mb_store = torch.zeros((self.N_SAMPLE_SLOTS, (3 if self._pos_offset else 2) * B * frame + 32),
                                         dtype=torch.uint8, device=dev)
        if self._kind == "scratch":
            # The scratch of a "scratch" augmentation: a minibatch's augmented frames, uint8 [3B][Ho][Wo][C] = (obs |
            # next_obs | pos) -- (Ho, Wo) = the augmentor's output_shape -- + 32 B of slack like a ring, per sample slot
            # (each slot starts on a 256-byte boundary: the kernel then stores 16 bytes per lane).  Downstream it IS a
            # ring: rows 0..3B-1, zero crop offsets -- static tensors.
            stride = (3 * B * self._scratch_frame() + 32 + 255) // 256 * 256
            self._shift_store = torch.zeros((self.N_SAMPLE_SLOTS, stride), dtype=torch.uint8, device=dev)
            self._shift_rows = torch.arange(3 * B, dtype=torch.int64, device=dev)
            self._shift_zero = torch.zeros(3 * B, dtype=torch.int32, device=dev)
        # A slot = the buffers ONE minibatch is assembled in (_assemble): ``dev`` the device block, ``scal`` the
        # transitions' scalars and ``scalars`` its (actions, rewards, not_dones) views, ``mb_u8`` the gathered stacks +
        # ``ar2`` = rows 0..2B-1 (frame store; pos_offset > 0: 0..3B-1), ``shift_u8`` the frames of a "scratch"
        # augmentation, ``both_f32`` / ``pos_f32`` the float tensors (absent here: allocated per call).  The rotating
        # slots are views of the stores above; a captured update graph has slots of its own with the same keys
        # (graph_block).
        ar2 = (torch.arange((3 if self._pos_offset else 2) * B, dtype=torch.int64, device=dev)
               if self.dedup_frames else None)
        self._sample_slots = []
        for s in range(self.N_SAMPLE_SLOTS):
            slot = dict(dev=self._d_index[s], scal=self._d_scal[s], scalars=self._scalar_views(self._d_scal[s]))
            if self.dedup_frames:
                slot.update(mb_u8=self._mb_store[s], ar2=ar2)
            if self._kind == "scratch":
                slot["shift_u8"] = self._shift_store[s]
            self._sample_slots.append(slot)
        self._graph_blocks = {}

    # ------------------------------------------------------------------ sampling
    def _scratch_frame(self):
        """Bytes of a frame of the scratch: a MINIBATCH frame (C, Ho, Wo), (Ho, Wo) the augmentor's output_shape.  Only a
        RandomTranslate (larger) or a Compose over one or over a RandomCrop (smaller) makes it differ from a stored frame
        (``_frame``: the rings, add, save / load, the frame store)."""
        oh, ow = self.augmentor.output_shape
        return self.obs_shape[0] * oh * ow

    def draw_indices(self):
        """Host RNG draws of sample_cpc, in the reference's order (utils.py:147 then augmentations.py:66-67 for obs,
        next_obs, pos).  Returns (idxs, offsets) with offsets an int32 array [6, B]: rows 2j, 2j + 1 = the first two words
        the augmentation draws for tensor j (``draw_index_words``: h1 / w1 of a RandomCrop, (dy, dx) / (ty, tx) of a
        RandomShift / RandomTranslate, (y0, x0) of a RandomCutout's boxes; zeros when it draws none).  An augmentation of
        four words -- RandomCutout -- returns int32 [12, B], rows 6 + 2j, 6 + 2j + 1 = the other two (its packed sizes
        and colours); one of six -- Compose -- int32 [18, B] by the same rule (word r of tensor j in row 6 (r // 2) + 2 j +
        r % 2): the move's offsets, the box's (y0, x0), its sizes and colours -- or RandomAffine's six words of the map,
        m00 m01 | m02 m10 | m11 m12.
        ``prioritized``: returns (u, offsets), u float64 [B] the stratified targets (k + r_k) / B with
        r = np.random.random_sample(B) drawn where the rows are drawn otherwise -- the rows themselves are drawn by
        curla_per_sample from u.
        ``aug_views = 2``: ``np.random.randint(0, n, size=B // 2)`` in the place of the B rows, returned tiled twice
        (``idxs[b + B // 2] == idxs[b]``); the words behind it are drawn for all B positions as ever."""
        B = self.batch_size
        if self.prioritized:
            # the stratified targets instead of the rows: u_k = (k + r_k) / B; the rows are drawn on the device
            if not self.full and self.idx == 0:
                raise ValueError("cannot sample an empty prioritized buffer")
            idxs = (np.arange(B) + np.random.random_sample(B)) / B
        elif self._aug_views == 2:
            # B / 2 transitions, each at positions b and b + B / 2; what follows draws per position as ever
            idxs = np.tile(np.random.randint(0, self.capacity if self.full else self.idx, size=B // 2), 2)
        else:
            idxs = np.random.randint(0, self.capacity if self.full else self.idx, size=B)
        if self._kind is None:
            raise NotImplementedError("unknown augmentation object: %r" % (self.augmentor,))
        offs = np.zeros((6 * max(1, (self._index_rows + 1) // 2), B), dtype=np.int32)
        for j in range(3):
            for r, word in enumerate(self.augmentor.draw_index_words(B)):
                offs[6 * (r // 2) + 2 * j + r % 2] = word
        return idxs, offs

    def _float_augmented(self, ring, idx, dev, j, out=None, draw_only=False):
        """Tensor ``j`` (0 obs, 1 next_obs, 2 pos) of a minibatch as an augmented float NHWC tensor [B, H, W, C] from
        ``ring`` rows ``idx`` (None: rows 0..B-1) (utils.py:168-182 branch: the torch/kornia augmentations).  With
        staged_aug the tensor's parameters are already on the device, in the minibatch's block ``dev`` (_aug_args) --
        nothing is drawn, allocated or copied here.  ``draw_only`` (a positive nobody wants): what the tensor's launch
        would draw is drawn -- nothing with staged_aug --, nothing is launched and None is returned."""
        B = self.batch_size
        c, h, w = self.obs_shape
        if draw_only:
            if not self.staged_aug:
                self.augmentor.draw_unstaged(B, (B, h, w, c), self.device)
            return None
        if out is None:
            out = torch.empty((B, h, w, c), dtype=torch.float32, device=self.device)
        self.augmentor.launch(ring, idx, B, out, self._aug_args(dev, j) if self.staged_aug else None)
        return out

    def block_layout(self):
        """Byte offsets inside a minibatch's block -- the ONE place that knows them.  Every block starts with
        idx int64 [2B] | crop offsets int32 [6][B] at ``offs`` .. ``offs_end`` (_fill_index_block).  ``staged_aug``
        appends the parameters of the three tensors (obs, next_obs, pos), ``aug_stride`` bytes each, laid out by
        the augmentation (``staged_layout``):
          ColorJiggle  params float [B k][4] (apply, contrast, saturation, hue) | order int32 [4]   (at ``aug_order``)
          NoisyCover   colours float [3] | 4 bytes of padding | (seed, Philox counter) uint64 [2]   (at ``aug_rng`` = 16)
          RandomConv   weights float [B][81] | 4 bytes of padding when B is odd (``aug_weights`` = 324 B, the bytes of the
                       weights; a key only this layout has -- the stride keeps ``nbytes`` a multiple of 8)
        An augmentation that draws four index words -- RandomCutout -- appends ``cut`` int32 [2][3B] behind them: the third
        words of obs | next_obs | pos (its packed box sizes), then the fourth (its colour words) -- contiguous runs for
        one launch of n = 3B.  One that draws six -- Compose, RandomAffine -- appends ``cut`` int32 [4][3B]: the third to
        sixth words, the box's y0 | x0 | sizes | colours, or the map's m02 | m10 | m11 | m12.
        ``n_step > 1`` appends ``next_row`` int64 [B] behind them: the bootstrap rows, written by the composing kernel.
        ``pos_offset > 0`` appends ``pos_row`` int64 [2][B] behind them, written by the positive's walk: the rows r whose
        next_obs is the positive, then capacity + r (the same rows in the double ring) -- and for a "scratch" augmentation
        ``pos_run`` int64 [3B], the double-ring rows of obs | next_obs | pos as one run for its single launch.
        ``prioritized`` appends ``u`` float64 [B], the targets of the draw (written by the host), and ``prob`` float32 [B]
        (+ 4 bytes of padding when B is odd), the drawn rows' probabilities (written by curla_per_sample, which also
        writes the idx run: the host leaves zeros there).
        ``nbytes`` is what a rotating sample slot stages per minibatch; the block of a captured update graph carries
        GRAPH_TAIL more bytes of per-update control values behind it (at ``tail``; ``graph_nbytes`` in all)."""
        B = self.batch_size
        n = 2 * B * 8 + 6 * B * 4
        lay = dict(idx=0, offs=2 * B * 8, offs_end=n, aug=None, aug_stride=0, aug_order=None, aug_rng=None)
        if self.staged_aug:
            stride, fields = self.augmentor.staged_layout(B, self.obs_shape)
            lay.update(aug=n, aug_stride=stride, **fields)
            n += 3 * stride
        if self._index_rows > 2:
            lay["cut"] = n
            n += (self._index_rows - 2) * 3 * B * 4
        assert n % 8 == 0
        if self.n_step > 1:  # next_row int64 [B]: the bootstrap rows without the double ring's offset (device-written)
            lay["next_row"] = n
            n += 8 * B
        if self._pos_offset:  # pos_row int64 [2][B] (| pos_run int64 [3B], scratch): the positive's walk writes them
            lay["pos_row"] = n
            n += 16 * B
            if self._kind == "scratch":
                lay["pos_run"] = n
                n += 24 * B
        if self.prioritized:  # u float64 [B]: the draw's targets (host-written) | prob float32 [B] (device-written)
            lay["u"] = n
            n += 8 * B
            lay["prob"] = n
            n += (4 * B + 7) // 8 * 8
        lay.update(nbytes=n, tail=n, graph_nbytes=n + self.GRAPH_TAIL)
        return lay

    def _noise_generator(self):
        """The torch generator of the HIP device: staged NoisyCover takes (seed, Philox counter) of its in-kernel noise
        from it, exactly as the policy-noise draws do (CurlSacAgent._noise) -- one non-overlapping counter sequence."""
        if self.device.type != "cuda":
            raise RuntimeError("no HIP device generator on a %s buffer" % self.device.type)
        return torch.cuda.default_generators[self.device.index if self.device.index is not None
                                             else torch.cuda.current_device()]

    def draw_aug(self):
        """(staged_aug) The host draws of the three tensors' augmentations, obs then next_obs then pos -- what the
        default path draws one tensor at a time (utils.py:173-182), by the augmentation's ``draw_staged``:
        ``ColorJiggle.draw_params`` and ``RandomConv.draw_weights`` from torch's CPU generator, ``NoisyCover.draw_colors``
        from NumPy; NoisyCover also reserves the tensor's Philox counters in the device generator (_noise_generator).
        None when nothing is staged."""
        if not self.staged_aug:
            return None
        return [self.augmentor.draw_staged(self.batch_size, self.obs_shape, self._noise_generator) for _ in range(3)]

    def _fill_aug(self, host, aug):
        """draw_aug()'s values into a pinned block (block_layout)."""
        lay = self._layout
        for j, drawn in enumerate(aug):
            self.augmentor.fill_staged(host, lay["aug"] + j * lay["aug_stride"], drawn)

    def _aug_args(self, dev, j):
        """What the augmentation kernel of tensor j reads from the device copy ``dev`` of a block (``staged_args``):
        ColorJiggle (params [B k, 4], order [4]) as tensors, RandomConv its weights [B, 81] as a tensor, NoisyCover
        (colours, (seed, counter)) as device addresses."""
        lay = self._layout
        return self.augmentor.staged_args(dev, lay["aug"] + j * lay["aug_stride"], self.batch_size, self.obs_shape)

    def _fill_index_block(self, host, idxs, offs):
        """A minibatch's indices and crop offsets in the layout the kernels read:
        idx [B] | idx + capacity [B] (the same transitions in the next_obs half of the double ring) | h1 of obs,
        next_obs, pos | w1 of obs, next_obs, pos -- so that (obs, next_obs) is ONE run of 2B frame indices, 2B row
        offsets and 2B column offsets."""
        B, lay = self.batch_size, self._layout
        i64 = host[lay["idx"]:lay["offs"]].view(torch.int64)
        if self.prioritized:  # ``idxs`` are the targets u: the rows are the draw kernel's to write
            u = np.ascontiguousarray(idxs, dtype=np.float64).reshape(-1)
            if np.asarray(idxs).dtype.kind != "f" or u.shape != (B,) or not ((u >= 0.0) & (u < 1.0)).all():
                raise ValueError("a prioritized buffer takes indices=(u, offs) with u float64 [B] in [0, 1) (draw_indices)")
            i64.zero_()
            host[lay["u"]:lay["u"] + 8 * B].view(torch.float64).copy_(torch.from_numpy(u))
            host[lay["prob"]:lay["nbytes"]].zero_()
        else:
            i64[:B].copy_(torch.from_numpy(np.ascontiguousarray(idxs, dtype=np.int64)))
            i64[B:].copy_(i64[:B] + self.capacity)
        o32 = host[lay["offs"]:lay["offs_end"]].view(torch.int32).view(6, B)
        offs = np.ascontiguousarray(offs, dtype=np.int32)
        if "cut" in lay and len(offs) != 3 * self._index_rows:
            raise ValueError("the block of an augmentor of %d index words takes offsets of %d rows (draw_indices), got %d"
                             % (self._index_rows, 3 * self._index_rows, len(offs)))
        o32.copy_(torch.from_numpy(np.ascontiguousarray(offs[[0, 2, 4, 1, 3, 5]])))
        if "cut" in lay:  # per further word a run of obs | next_obs | pos: sizes, then colours (Compose: y0, x0 in front)
            runs = self._index_rows - 2
            c32 = host[lay["cut"]:lay["cut"] + 12 * runs * B].view(torch.int32).view(3 * runs, B)
            c32.copy_(torch.from_numpy(np.ascontiguousarray(offs[[6 * (r // 2) + 2 * j + r % 2 for r in range(2, 2 + runs)
                                                                  for j in range(3)]])))

    def _upload_indices(self, idxs, offs, aug=None, want_pos=True):
        """A minibatch's indices and crop offsets (and, staged_aug, its augmentation parameters ``aug``) into the next
        rotating slot's device block, the transitions' scalars (n_step: composed) into its scalar buffer; returns the
        slot and the guard of handles into it."""
        u, every = self._slot_use, self.EVENT_EVERY
        self._slot_use = u + 1
        k = u % self._n_slots
        if u >= self._n_slots:
            e = (u - self._n_slots) // every
            ev = self._slot_events.get(e)
            if ev is not None:
                ev.synchronize()
            for old in [i for i in self._slot_events if i < e]:
                del self._slot_events[old]
        host = self._h_index[k]
        self._fill_index_block(host, idxs, offs)
        if aug is not None:
            self._fill_aug(host, aug)
        s = self._sample_slot = (self._sample_slot + 1) % self.N_SAMPLE_SLOTS
        self._sample_gen[s] += 1
        slot = self._sample_slots[s]
        dst = slot["dev"]
        if self._h_index_dev is not None:  # the block is read from the pinned slot by the staging launch
            self._stage(self._h_index_dev[k], dst, host.numel(), slot["scalars"])
        else:
            dst.copy_(host, non_blocking=True)
            if self.device.type == "cuda" or _lib_tracing():
                self._stage(None, dst, host.numel(), slot["scalars"], copied=True, want_pos=want_pos)
        if self.device.type == "cuda" and u % every == every - 1:
            ev = torch.cuda.Event()
            ev.record()
            self._slot_events[u // every] = ev
        return slot, (self._sample_gen, s, self._sample_gen[s])

    def _nstep_discount(self):
        """``discount`` as the kernels take it: read at every sample, so an edit of the attribute is seen."""
        return _checked_discount(self.discount)

    def _scalar_views(self, scal):
        """actions [B, ...], rewards [B, 1], not_dones [B, 1] (utils.py:159-166) inside a slot's scalar buffer (made
        once per slot: ``scalars``)."""
        B, A = self.batch_size, self._n_act
        return (scal[:B * A].view((B,) + tuple(self.actions.shape[1:])), scal[B * A:B * A + B].view(B, 1),
                scal[B * A + B:].view(B, 1))

    def _stage(self, host_dev, dev, nbytes, out, copied=False, want_pos=True):
        """Staging a minibatch: the transitions' scalars into ``out`` (_scalar_views; n_step > 1: composed) and, with
        pos_offset > 0, the positive's rows into the block.  ``host_dev``, the pinned block's device address: ONE launch,
        which also brings the block to ``dev``.  ``copied``, the block is in ``dev`` already: a launch each -- and
        without ``want_pos`` none for the positive's walk (in the one launch it rides along as it is)."""
        B, A, lay = self.batch_size, self._n_act, self._layout
        cont = self._cont if self._keep_cont else None
        lane = dict(stride=self._n_envs) if self._n_envs > 1 else {}  # the walks' step (the _strided entry points)
        if copied:
            if self.prioritized:  # the draw: rows into the block's idx run, their probabilities into ``prob``
                ops.per_sample(self._per_s, self._per_sums, dev, lay["u"], lay["prob"], B)
            ops.gather_transition_scalars(self._sc, dev[lay["idx"]:lay["idx"] + 8 * B].view(torch.int64), B, A, *out)
            if self.n_step > 1:  # the bootstrap rows must be in the block before anything reads pixels
                ops.nstep_compose(dev, lay["next_row"], self._sc, cont, self.capacity, self.n_step,
                                  self._nstep_discount(), B, A, *out, **lane)
            if self._pos_offset and want_pos:  # ... and so must the positive's rows (behind the draw: it writes the idx run)
                ops.pos_walk(dev, lay["pos_row"], lay.get("pos_run"), lay.get("next_row"), cont, self.capacity,
                             self._pos_offset, self.n_step, B, **lane)
        elif self._pos_offset:
            ops.sample_stage_pos(host_dev, dev, nbytes, lay.get("next_row"), lay["pos_row"], lay.get("pos_run"), self._sc,
                                 cont, self.capacity, self.n_step, self._nstep_discount() if self.n_step > 1 else 1.0,
                                 self._pos_offset, B, A, *out, **lane)
        elif self.n_step > 1:
            ops.sample_stage_nstep(host_dev, dev, nbytes, lay["next_row"], self._sc, cont, self.capacity, self.n_step,
                                   self._nstep_discount(), B, A, *out, **lane)
        else:
            ops.sample_stage(host_dev, dev, nbytes, self._sc, B, A, *out)

    def _require_cuda(self):
        from . import _lib
        if self.device.type != "cuda" and _lib._trace_hook is None:
            raise RuntimeError("sampling pixels needs the HIP device: curla_amd has no CPU fallback for the learner path")

    def _sources(self, slot, want_pos=True):
        """Where the loaders read the minibatch of ``slot`` from -- which storage, which rows for next_obs: decided
        here and nowhere else.  Returns a _Sources:
          tensors  (ring, rows) of obs, next_obs, pos: ONE ring each, ``rows`` int64 [B] or None for rows 0..B-1;
                   next_obs at the sampled rows, or with n_step > 1 at the bootstrap rows that the composition wrote into
                   the block (block_layout: next_row); pos the obs ring at the sampled rows, or with pos_offset > 0 the
                   next_obs ring at the rows the positive's walk wrote (block_layout: pos_row)
          off      the six offset rows: off[2j] / off[2j+1] = h1 / w1 of tensor j
          both     the ring of obs frames then next_obs frames in which (obs | next_obs) is ONE run of 2B rows ``idx2``
                   (None: rows 0..2B-1) with offsets ``h2`` / ``w2``; None when the rings are two allocations
          pos2     the positive's rows in ``both`` (None with ``idx2``: rows 0..B-1, pos_offset > 0: 2B..3B-1)
          run      in ``both``, the rows that ONE launch over obs | next_obs | pos reads, sample s row run[s % period]
                   (None: s % period): ``idx2`` with period 2B, with pos_offset > 0 the block's pos_run with period 3B
          words    the index words of obs, next_obs, pos as int32 runs of 3B each: the h rows, the w rows (RandomShift's
                   (dy, dx), RandomTranslate's (ty, tx), RandomCutout's (y0, x0)) and, where four words are drawn, the
                   runs of ``cut`` (RandomCutout's packed box sizes and colour words; Compose's y0, x0, sizes, colours)
        Plain storage reads the rings at the sampled rows.  The frame store first assembles the k frames of every
        sampled stack into the slot's [2B][H][W][3k] uint8 buffer (one gather kernel per tensor; with pos_offset > 0 a third
        one, the next_obs stacks of the positive's rows, into a buffer of [3B]).
        Without ``want_pos`` (sample_cpc_refs) nothing is launched for the positive and nothing reads rows its walk would
        have written: no third gather, and ``run`` is ``idx2`` with period 2B whatever pos_offset says."""
        B, lay, dev = self.batch_size, self._layout, slot["dev"]
        d64 = dev[lay["idx"]:lay["offs"]].view(torch.int64)
        d32 = dev[lay["offs"]:lay["offs_end"]].view(torch.int32)
        off = [d32[(j // 2 + 3 * (j % 2)) * B:(j // 2 + 3 * (j % 2) + 1) * B] for j in range(6)]
        rows = d64[:B]
        rows_n = rows if self.n_step == 1 else dev[lay["next_row"]:lay["next_row"] + 8 * B].view(torch.int64)
        kp = self._pos_offset
        # the positive: an augmentation of obs again, or with pos_offset > 0 of next_obs at the rows its walk wrote
        p64 = dev[lay["pos_row"]:lay["pos_row"] + 16 * B].view(torch.int64) if kp else None
        rows_p, period = (p64[:B] if kp else rows), (3 if kp else 2) * B
        if self.dedup_frames:
            c, h, w = self.obs_shape
            nt = 3 if kp else 2
            both = slot["mb_u8"][:nt * B * self._frame].view(nt * B, h, w, c)
            rings, idx2 = tuple(both[j * B:(j + 1) * B] for j in range(nt)), None
            for j, r in enumerate((rows, rows_n, rows_p)[:nt if want_pos else 2]):
                ops.gather_stacks(self.frames, self._fid[:, min(j, 1), :], r, B, rings[j])
            rows = rows_n = rows_p = None
            pos, pos2, run = (rings[2 if kp else 0], None), None, None
        else:
            both, rings, idx2 = self._both, (self.obses, self.next_obses), d64
            pos = (rings[1 if kp else 0], rows_p)
            pos2 = p64[B:] if kp else rows  # (the double ring's next_obs half: capacity + r)
            run = dev[lay["pos_run"]:lay["pos_run"] + 24 * B].view(torch.int64) if "pos_run" in lay else d64
            if not want_pos:
                run, period = d64, 2 * B
        words = (d32[:3 * B], d32[3 * B:])
        if "cut" in lay:
            runs = self._index_rows - 2
            c32 = dev[lay["cut"]:lay["cut"] + 12 * runs * B].view(torch.int32)
            words += tuple(c32[3 * B * k:3 * B * (k + 1)] for k in range(runs))
        return _Sources(both, idx2, d32[:2 * B], d32[3 * B:5 * B], ((rings[0], rows), (rings[1], rows_n), pos), off, words,
                        pos2, run, period)

    def _scratch_aug(self, slot, src, want_pos=True):
        """A "scratch" augmentation: the frames of a minibatch (``src``: _sources) augmented by its ``scratch_launch`` --
        shifted, boxes painted, placed on the canvas -- into the slot's scratch as obs | next_obs | pos; returns the
        [3B][Ho][Wo][C] view ((Ho, Wo) = output_shape).  With ``both`` ONE launch, pos reading the obs rows again (period
        2B) or, pos_offset > 0, its own rows (period 3B); with the rings in two allocations one launch per tensor.
        Without ``want_pos`` the one launch is of n = 2B, obs | next_obs, and the third of the per-tensor ones is left out:
        the scratch's last B rows then hold an earlier minibatch's positives."""
        B = self.batch_size
        oh, ow = self.augmentor.output_shape
        out = slot["shift_u8"][:3 * B * self._scratch_frame()].view(3 * B, oh, ow, self.obs_shape[0])

        def launch(ring, rows, period, lo, hi):
            self.augmentor.scratch_launch(ring, rows, period, [w[lo:hi] for w in src.words], hi - lo, out[lo:hi])
        if src.both is not None:
            launch(src.both, src.run, src.period, 0, (3 if want_pos else 2) * B)
        else:
            for j, (ring, rows) in enumerate(src.tensors[:3 if want_pos else 2]):
                launch(ring, rows, B, j * B, (j + 1) * B)
        return out

    def _shift_refs(self, shifted, guard):
        """(obs, next_obs, pos) handles over the minibatch in a scratch: an ordinary uint8 ring of 3B rows of
        ``output_shape``, nothing left to crop; obs carries the (obs | next_obs) pair of 2B rows."""
        B = self.batch_size
        hw = tuple(self.augmentor.output_shape)
        ar, z = self._shift_rows, self._shift_zero
        obses, next_obses, pos = (ops.ObsRef.from_ring(shifted, ar[j * B:(j + 1) * B], z[:B], z[:B], B, hw, guard)
                                  for j in range(3))
        obses.pair = (ops.ObsRef.from_ring(shifted, ar[:2 * B], z[:2 * B], z[:2 * B], 2 * B, hw, guard), next_obses)
        return obses, next_obses, pos

    def _assemble(self, slot, guard, want_pos=True):
        """The (obs, next_obs, pos) handles of the minibatch whose block and scalars are staged in ``slot`` -- a rotating
        slot (sample_cpc_refs; ``guard`` from _upload_indices) or a captured graph's (graph_refs; ``guard`` None), whose
        launches then write to fixed addresses: the
        gathers of the frame store (_sources), then by the augmentation's kind ring handles (nothing is launched: the first
        conv layer gathers and crops), the launch(es) into the scratch, or the three float launches.  Without ``want_pos``
        the positive's handle is None and nothing is launched that writes the positive alone."""
        B = self.batch_size
        src = self._sources(slot, want_pos)
        both, idx2, tensors, off = src.both, src.idx2, src.tensors, src.off
        if self._kind == "float":
            # obs, next_obs and pos (= a copy of obs) are augmented independently (utils.py:173-182); obs and
            # next_obs are written into the two halves of one [2B] tensor (ObsRef.pair, see below)
            c, h, w = self.obs_shape
            fb = slot.get("both_f32")
            if fb is None:
                fb = torch.empty((2 * B, h, w, c), dtype=torch.float32, device=self.device)
            outs = fb[:B], fb[B:], slot.get("pos_f32")
            obses, next_obses = (ops.ObsRef.from_nhwc(self._float_augmented(ring, rows, slot["dev"], j, outs[j]))
                                 for j, (ring, rows) in enumerate(tensors[:2]))
            ring, rows = tensors[2]  # (behind the other two: the order of the host draws)
            pos = self._float_augmented(ring, rows, slot["dev"], 2, outs[2], draw_only=not want_pos)
            pos = ops.ObsRef.from_nhwc(pos) if want_pos else None
            obses.pair = (ops.ObsRef.from_nhwc(fb), next_obses)
        elif self._kind == "scratch":
            obses, next_obses, pos = self._shift_refs(self._scratch_aug(slot, src, want_pos), guard)
        else:
            crop = tuple(self.augmentor.output_shape)
            if both is not None:
                # every handle indexes the ONE ring that holds obs frames then next_obs frames, so that any two of
                # them can share a first-layer launch (ops.conv1_fwd2), and (obs | next_obs) is itself a handle of
                # 2B frames: the critic phase runs both through the online convs in one launch per layer
                # (curl_sac.py:350-358)
                pos2 = src.pos2
                if idx2 is None:
                    ar = slot["ar2"]
                    idx2, pos2 = ar[:2 * B], (ar[2 * B:] if self._pos_offset else ar[:B])
                tensors = (both, idx2[:B]), (both, idx2[B:]), (both, pos2)
            # (else rings in two allocations -- the second half would not start on a dword: no pair)
            obses, next_obses, pos = (ops.ObsRef.from_ring(ring, rows, off[2 * j], off[2 * j + 1], B, crop, guard)
                                      for j, (ring, rows) in enumerate(tensors))
            if both is not None:
                obses.pair = (ops.ObsRef.from_ring(both, idx2, src.h2, src.w2, 2 * B, crop, guard), next_obses)
        return obses, next_obses, pos if want_pos else None

    # ---- dedicated sample slots of captured update graphs (CurlSacAgent.enable_update_graphs) ---------------------
    # A captured graph replays the SAME pointers: its minibatch block lives in its own pinned host slot and its own
    # device block, never in the rotating ones above.  Behind the indices the block carries GRAPH_TAIL bytes of per-update
    # control values (RNG stream positions, Adam step factors) that the graph's kernels read from the device copy.
    def graph_supported(self):
        """Graph replay covers every minibatch whose per-update values reach the kernels through the block: the
        uint8-ring ones (RandomCrop / RandomShift / RandomCutout / RandomTranslate / RandomFlip / RandomRotate /
        RandomGrayscale / RandomAffine / identity; plain storage with both rings in one allocation, or ``dedup_frames``,
        whose stacks are gathered into a buffer of the graph's own), and the float augmentations ColorJiggle / NoisyCover /
        RandomConv constructed with ``staged_aug=True`` (either storage).  A
        ``prioritized`` buffer is not covered (its draw and its priority update are not nodes of the captured graphs).
        A float augmentation WITHOUT staged_aug draws and uploads its parameters through a pinned block of its own per
        call and stays eager.  Pinned index slots read in place are required."""
        if self.device.type != "cuda" or self._h_index_dev is None or self.prioritized:
            return False
        if self._kind == "float":
            return self.staged_aug
        return self.dedup_frames or self._both is not None

    def graph_block(self, slot):
        g = self._graph_blocks.get(slot)
        if g is None:
            B, A = self.batch_size, self._n_act
            lay = self._layout
            nb = lay["graph_nbytes"]
            host = torch.zeros(nb, dtype=torch.uint8, pin_memory=self.device.type == "cuda")
            g = dict(host=host, host_dev=ops.host_device_pointer(host),
                     dev=torch.zeros(nb, dtype=torch.uint8, device=self.device),
                     scal=torch.empty(B * (A + 2), dtype=torch.float32, device=self.device), event=None,
                     tail=lay["tail"], guards=[])
            g["scalars"] = self._scalar_views(g["scal"])
            # A replayed graph writes to the SAME addresses every time, so the minibatch tensors that the rotating
            # sample slots / the allocator provide per call are buffers of the graph slot here (allocated now, before
            # the capture): the gathered uint8 stacks of the de-duplicated store, the float NHWC tensors of an
            # augmentation.  Each sits between guard bytes (tests/test_gpu_graph_aug.py).
            frame = self._frame
            if self.dedup_frames:
                nt = 3 if self._pos_offset else 2  # (+32: the loaders' slack, as a ring)
                (g["mb_u8"],) = self._guarded([nt * B * frame + 32], g["guards"])
                g["ar2"] = torch.arange(nt * B, device=self.device, dtype=torch.int64)
            if self._kind == "scratch":  # the augmented (obs | next_obs | pos) frames, + the loaders' slack
                (g["shift_u8"],) = self._guarded([3 * B * self._scratch_frame() + 32], g["guards"])
            if self._kind == "float":
                c, h, w = self.obs_shape
                both, pos = self._guarded([4 * 2 * B * frame, 4 * B * frame], g["guards"])
                g["both_f32"] = both.view(torch.float32).view(2 * B, h, w, c)
                g["pos_f32"] = pos.view(torch.float32).view(B, h, w, c)
            self._graph_blocks[slot] = g
        return g

    def _guarded(self, sizes, guards):
        """Zeroed uint8 device buffers of ``sizes`` bytes in one allocation, GUARD bytes of GUARD_BYTE in front of,
        between and behind them (each buffer starts 256-byte aligned); the guard views are appended to ``guards``."""
        G = self.GUARD
        padded = [(n + G - 1) // G * G for n in sizes]
        store = torch.full((G + sum(p + G for p in padded),), self.GUARD_BYTE, dtype=torch.uint8, device=self.device)
        out, at = [], G
        guards.append(store[:G])
        for n, pn in zip(sizes, padded):
            out.append(store[at:at + n].zero_())
            guards.append(store[at + n:at + pn + G])
            at += pn + G
        return out

    def graph_write(self, slot, idxs, offs, tail, aug=None):
        """Host side of one graphed update: the minibatch's indices / offsets, the augmentation parameters
        (``aug`` = draw_aug(), staged_aug) and the control tail (80 bytes) into the slot's pinned block -- after the
        previous replay that reads this block has finished."""
        g = self.graph_block(slot)
        if g["event"] is not None:
            g["event"].synchronize()
        self._fill_index_block(g["host"], idxs, offs)
        if aug is not None:
            self._fill_aug(g["host"], aug)
        g["host"][g["tail"]:].copy_(torch.from_numpy(np.frombuffer(bytearray(tail), dtype=np.uint8)))
        return g

    def graph_refs(self, slot):
        """Device side, called while the graph is being captured: the staging launch (pinned block -> device block +
        the transitions' scalars), for the de-duplicated store the two gather_stacks launches (they read ``_fid`` when
        the graph is replayed; three with pos_offset > 0), for a "scratch" augmentation its launch into the slot's scratch
        (it reads its index words from the device block), for a staged float augmentation the three jitter / cover /
        convolution launches (they read their parameters from the device block), and the sample_cpc 6-tuple with handles
        into the slot's buffers.  Nothing here draws a random number."""
        g = self.graph_block(slot)
        # (n_step, pos_offset: the launch reads ``cont`` when the graph runs)
        self._stage(g["host_dev"], g["dev"], g["host"].numel(), g["scalars"])
        obses, next_obses, pos = self._assemble(g, None)
        act, rew, nd = g["scalars"]
        return obses, act, rew, next_obses, nd, dict(obs_anchor=obses, obs_pos=pos, time_anchor=None, time_pos=None)

    def sample_cpc_refs(self, indices=None, want_pos=True):
        """The fused form of sample_cpc: same 6-tuple, but obs / next_obs / pos are
        ``ObsRef`` handles (ring + indices + crop offsets) consumed directly by the
        first conv kernel.  ``indices=(idxs, offs)`` injects pre-drawn indices (tests, DP).
        The handles of one call stay valid until N_SAMPLE_SLOTS further samples have been drawn (using an older
        one raises).
        ``want_pos=False`` (a leading sub-step of CurlSacAgent(utd_ratio=G): no CURL phase follows): everything is drawn
        that is drawn otherwise -- indices, the three tensors' index words and float-augmentation parameters, NoisyCover's
        noise counters --, so every stream ends where it ends with the positive; nothing is launched whose only output is
        the positive (the third float-augmentation launch, the positive's share of a scratch augmentation's launch, the
        positive's gather_stacks of a dedup_frames buffer, the positive's walk where it is a launch of its own), and
        ``cpc_kwargs["obs_pos"]`` is None.  Where the positive rides in a launch that runs anyway, that launch is
        unchanged."""
        self._require_cuda()
        idxs, offs = indices if indices is not None else self.draw_indices()
        slot, guard = self._upload_indices(idxs, offs, self.draw_aug(), want_pos)
        obses, next_obses, pos = self._assemble(slot, guard, want_pos)
        if self.prioritized:
            obses.per = self._per_handle(slot, guard)
        actions, rewards, not_dones = slot["scalars"]  # (valid as long as the pixel handles are)
        cpc_kwargs = dict(obs_anchor=obses, obs_pos=pos, time_anchor=None, time_pos=None)
        return obses, actions, rewards, next_obses, not_dones, cpc_kwargs

    def sample_cpc(self, indices=None):
        """utils.py:144-187 with the reference's return types: float32 NCHW tensors
        in [0,255] on the device (materialised by one crop kernel per tensor)."""
        self._require_cuda()
        idxs, offs = indices if indices is not None else self.draw_indices()
        slot, guard = self._upload_indices(idxs, offs, self.draw_aug())
        B = self.batch_size
        c = self.obs_shape[0]
        oh, ow = self.augmentor.output_shape
        src = self._sources(slot)
        shifted = self._scratch_aug(slot, src) if self._kind == "scratch" else None
        outs = []
        for j, (ring, rows) in enumerate(src.tensors):
            t = torch.empty((B, c, oh, ow), dtype=torch.float32, device=self.device)
            if shifted is not None:  # the shifted frames as they are: rows j B .. of the scratch, zero offsets
                z = self._shift_zero[:B]
                ops.crop_nchw(shifted, self._shift_rows[j * B:(j + 1) * B], z, z, B, (oh, ow), out_f32=t)
            elif self._kind == "float":
                ops.nhwc_to_nchw(self._float_augmented(ring, rows, slot["dev"], j), t)
            else:
                ops.crop_nchw(ring, rows, src.off[2 * j], src.off[2 * j + 1], B, (oh, ow), out_f32=t)
            outs.append(t)
        obses, next_obses, pos = outs
        if self.prioritized:  # (the tensor is fresh, the handle is not: valid until the slot is drawn again)
            obses.per = self._per_handle(slot, guard)
        # fresh tensors, like the reference's
        actions, rewards, not_dones = (t.clone() for t in slot["scalars"])
        cpc_kwargs = dict(obs_anchor=obses, obs_pos=pos, time_anchor=None, time_pos=None)
        return obses, actions, rewards, next_obses, not_dones, cpc_kwargs

    # ------------------------------------------------------------------ priorities
    def _per_handle(self, slot, guard):
        B, lay, dev = self.batch_size, self._layout, slot["dev"]
        return PerHandle(self, dev[lay["idx"]:lay["idx"] + 8 * B].view(torch.int64),
                         dev[lay["prob"]:lay["prob"] + 4 * B].view(torch.float32), guard)

    def _require_prioritized(self):
        if not self.prioritized:
            raise RuntimeError("this ReplayBuffer was constructed with prioritized=False")

    def update_priorities(self, rows, values):
        """Store ``values`` (float32 device tensor [n], the stored values themselves, i.e. ``p ** per_alpha``; >= 0) for
        ring rows ``rows`` (int64 device tensor [n]) -- the rule of the critic update: a row named several times takes
        its largest value, and the maximum that new transitions get is raised, never lowered.
        Preconditions, not checked on the device (a check would read the tensors back): every row lies in [0, len_valid)
        -- ``capacity`` once the ring is full, ``idx`` before; a row beyond holds no transition and a positive value would
        make it drawable, one outside [0, capacity) is written out of bounds -- and at least one row of the buffer keeps
        a positive value (a draw from a ring without any mass returns row 0 with probability 0, which the critic update
        gives weight 0).  Values are stored finite and non-negative: a negative one, -0 or a NaN becomes 0 (the row is
        then never drawn), +inf the largest float."""
        self._require_prioritized()
        if not (isinstance(rows, torch.Tensor) and isinstance(values, torch.Tensor) and rows.dtype == torch.int64
                and values.dtype == torch.float32 and rows.dim() == 1 and rows.shape == values.shape and rows.numel()):
            raise ValueError("update_priorities takes an int64 and a float32 device tensor of one shape [n], n >= 1")
        if rows.device != self._per_s.device or values.device != self._per_s.device:
            raise ValueError("update_priorities takes tensors on the buffer's device %s, got %s and %s"
                             % (self._per_s.device, rows.device, values.device))
        ops.per_set(self._per_s, self._per_sums, self._per_max, rows.numel(), rows=rows.contiguous(),
                    values=values.contiguous())

    def priorities(self):
        """The stored values ``p ** per_alpha`` of rows [0, len_valid) -- ``capacity`` once the ring is full, ``idx``
        before -- as a NumPy float32 array (a device-to-host copy: inspection, not the training loop)."""
        self._require_prioritized()
        return self._per_s[:self.capacity if self.full else self.idx].cpu().numpy()

