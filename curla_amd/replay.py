"""Replay buffer of the learner path (reference: utils.py): the class, its constructor and persistence.  Its write
side (``add``, ``add_vec``, ``add_batch``, the continuity rule) is replay_write.py, its read side (the draws, the
minibatch's staging and assembly, graph slots, priorities) replay_sample.py.

``ReplayBuffer`` keeps the reference's constructor, ``add``, ``sample_cpc``, ``save``/``load``, ``idx``/``full`` --
but the ring lives in HBM (uint8, NHWC so a cropped row is one contiguous run) and sampling hands the learner
*references* (frame indices + crop offsets) instead of materialised float tensors: the reference's 3 x B x C x H x W
float32 host->device copy per update (utils.py:161-166) disappears.  Index and crop-offset draws stay on the host in
NumPy's legacy global stream, in the reference's order, so a seeded run samples the same transitions and windows
(bit-exact).

``dedup_frames=True`` stores every RGB frame once: a frame stack of k frames shares k-1 of them with
its successor and ``next_obs[t]`` is ``obs[t+1]`` inside an episode (utils.py:238-268), so an environment step adds
ONE new frame instead of 2k -- 63.5 KB -> 21 KB per transition at 84x84x9, 339 KB -> 85 KB at 168x168x12.  Sharing is
detected from the bytes handed to ``add`` (hash, then full comparison), never assumed, so sampled pixels are the
reference's whatever the caller does.

``staged_aug=True`` (float augmentations: ColorJiggle, NoisyCover, RandomConv) sends the random parameters of a
minibatch's three tensors along in the index block instead of through a pinned block and a copy of their own per
tensor, and lets NoisyCover draw its noise inside the cover kernel: with it -- and for ``dedup_frames`` without it --
the minibatch can be a node of a captured update graph (``graph_supported``).
"""
import os

import numpy as np
import torch

from . import ops
from .replay_sample import PerHandle, _checked_discount, _checked_per, _ReplaySampleMixin  # noqa: F401
from .replay_write import _FrameStore, _ReplayWriteMixin


def _checked_int(name, v, least):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < least:
        raise ValueError("%s must be an int >= %d, got %r" % (name, least, v))
    return int(v)


class ReplayBuffer(_ReplayWriteMixin, _ReplaySampleMixin):
    """Buffer to store environment transitions (utils.py:80-236), HBM-resident.

    ``n_step=n > 1`` (beyond the reference; DrQ-v2 uses 3) makes every sample an n-step transition: reward becomes
    ``sum_{k<m} discount^k r_{t+k}``, not_done ``not_done_{t+m-1} discount^(m-1)`` and next_obs the one of row
    ``t+m-1``, ``m <= n`` being the steps the episode still has from row t on -- so the learner's unchanged
    ``reward + not_done * discount * (...)`` is the n-step TD target.  ``discount`` is then required and must be the
    agent's (``CurlSacAgent.update`` checks it); it is a plain attribute, read at every sample.  Which row continues
    which is detected from the data handed to the write routes (a per-row flag ``cont``; one rule for all of them,
    ``replay_write._Chain``): row i continues into row i + 1 when that was the very next write, ``done`` was false and
    row i's ``next_obs`` equals row i + 1's ``obs`` byte for byte -- a time-limit truncation or a reset breaks the
    chain without a change to ``add``'s signature.  A caller that
    interleaves several environments into one ``n_envs=1`` buffer through ``add`` gets a break at every switch, i.e.
    1-step targets: several environments belong in an ``n_envs=N`` buffer (below), whose chains run per environment.
    ``n_step=1`` (default) is the reference's buffer: nothing is allocated, launched or laid out differently.

    ``prioritized=True`` (beyond the reference; Schaul et al. 2016, the proportional variant) draws row i with
    probability ``s_i / sum_j s_j``, ``s_i = p_i ** per_alpha`` being the value stored for the row in HBM.  A transition
    written by ``add``, ``add_batch`` or ``load`` (a ring wrap included) gets the largest value stored so far (1.0 at
    first); rows never written hold 0 and are never drawn.  The draw is stratified -- the host draws
    ``np.random.random_sample(B)`` where it draws ``randint`` otherwise, sample k looks for ``(k + r_k) / B`` of the total
    -- and happens in a kernel that writes the rows into the minibatch's device block, so ``draw_indices`` returns
    ``(u, offs)`` in this mode and the host never learns the rows.  The obs handle of a sample carries ``per`` (a
    ``PerHandle``): ``CurlSacAgent.update_critic`` weights its loss by ``(min_j P_j / P_k) ** per_beta`` and stores
    ``(0.5 (|q1 - t| + |q2 - t|) + per_eps) ** per_alpha`` for the drawn rows; ``update_priorities`` does the same for user
    code.  ``per_alpha``, ``per_beta`` and ``per_eps`` are plain attributes read at every sample or update (anneal
    ``per_beta`` by assigning it).  Priorities are not part of the reference's ``save`` payload and are NOT persisted:
    ``load`` gives every loaded row the maximum.  Such a buffer is not graph-replayable (``graph_supported``).
    ``prioritized=False`` (default): nothing is allocated, launched or laid out differently.

    ``pos_offset=k >= 1`` (beyond the reference; the temporal contrast of ATC, Stooke et al. 2021) makes the CURL positive
    of a sampled row t an augmentation of the observation up to k steps LATER in the same episode instead of a second
    augmentation of ``obs[t]``: the positive is ``next_obs[r]``, r being t advanced along the continuity flags ``cont``
    (the rule above) at most k - 1 times -- ``r = t; repeat k - 1 times: if not cont[r]: stop; r = (r + 1) % capacity``
    -- i.e. the observation ``min(k, steps the chain still has from t)`` steps after ``obs[t]``.  It never crosses an
    episode end, a truncation, a reset, the write head or an overwritten row; environments interleaved through ``add``
    break the chain at every switch (the positive is then ``next_obs[t]``; ``n_envs=N`` keeps a chain per environment).
    ``k = 1`` gives ``next_obs[t]`` and needs no flag: the flags are kept when ``n_step > 1`` or ``pos_offset > 1``.
    The walk happens on the device, in the staging launch of the minibatch (curla_sample_stage_pos; curla_pos_walk
    where the block travels by copy), so the host draws exactly what it draws with ``pos_offset=0``: a seeded run
    samples the same transitions with the same three augmentation draws, only the positive's pixels differ, and
    ``cpc_kwargs`` keeps ``time_anchor=None, time_pos=None``.  This is ATC's positive SELECTION behind CURL's own
    bilinear head and momentum encoder -- not ATC's residual predictor.  Read-only after construction (it decides the
    block layout).  ``pos_offset=0`` (default): nothing is allocated, launched or laid out differently.

    ``n_envs=N > 1`` (beyond the reference) stores the steps of N environments that act side by side: ``add_vec`` takes one
    step of all of them -- N observations, actions, rewards, next observations and dones -- and writes it in one launch.
    Environment e at vector step t owns ring row ``(t * N + e) % capacity``, so each environment is a lane of stride N,
    ``capacity`` must be a multiple of N and ``idx`` always is one (a vector step never straddles the ring's end).
    ``cont[r] == 1`` then means that row ``(r + N) % capacity`` continues row r's episode, and the n-step composition and
    the positive's walk advance by N rows: ``n_step`` and ``pos_offset`` work per environment.  The rule is the same
    one, per lane, against the vector step written directly before -- an auto-resetting vector environment hands back a
    reset stack and so breaks the chain by itself, as a time-limit truncation does.  The newest N rows always carry 0.
    ``add`` refuses such a buffer; ``add_batch`` and ``load`` take whole vector steps in row order (step-major,
    environment-minor).  Not combined with ``dedup_frames`` (its match of recent frames is per stream).  Read-only after
    construction.  ``n_envs=1`` (default): nothing is allocated, launched or laid out differently.

    ``aug_views=2`` (beyond the reference; DrQ, Kostrikov et al. 2021, K = M = 2) makes a minibatch of B positions hold
    B / 2 transitions, each at positions b and b + B / 2: ``draw_indices`` draws ``randint(0, n, size=B // 2)`` where it
    draws B rows otherwise and returns them tiled twice.  Everything behind the rows is per position and unchanged -- the
    augmentation's words, ``draw_aug``, the block, the launches --, so the two positions of a transition get independent
    augmentations of obs, next_obs and the positive, and share action, reward, not_done (and the n-step composition and
    the positive's walk, which start from the same row).  ``batch_size`` must be even; not with ``prioritized=True``.
    Injected ``indices=`` are taken as they are.  The learner's half is ``CurlSacAgent(aug_views=2)``, which checks that
    the two agree.  Read-only after construction.  ``aug_views=1`` (default): the draws are the ones above."""

    N_SAMPLE_SLOTS = 2  # minibatches whose references may be alive at once (the current one + one drawn ahead)
    EVENT_EVERY = 8     # index uploads per recorded event (16 pinned slots)
    # The block of a captured update graph carries GRAPH_TAIL bytes of per-update control values behind the indices:
    # u64[4] (seed, critic-noise offset, seed, actor-noise offset) | f64[2] log_alpha | f32[8] four Adams
    GRAPH_TAIL = 80
    GUARD, GUARD_BYTE = 256, 0xA5  # around a graph slot's minibatch buffers (_guarded)

    def __init__(self, obs_shape, action_shape, capacity, batch_size, device, augmentor, transform=None,
                 dedup_frames=False, frame_capacity=None, staged_aug=False, n_step=1, discount=None,
                 prioritized=False, per_alpha=0.6, per_beta=0.4, per_eps=1e-6, pos_offset=0, n_envs=1, aug_views=1):
        self._aug_views = _checked_int("aug_views", aug_views, 1)
        if self._aug_views > 2:
            raise ValueError("aug_views must be 1 or 2, got %r" % (aug_views,))
        if self._aug_views == 2:
            if isinstance(batch_size, bool) or not isinstance(batch_size, (int, np.integer)) or batch_size % 2 != 0:
                raise ValueError("aug_views = 2 puts the two views of a transition at positions b and b + batch_size / 2: "
                                 "batch_size = %r is not an even int" % (batch_size,))
            if prioritized:
                raise ValueError("aug_views = 2 is not combined with prioritized=True: a prioritized buffer's rows are "
                                 "drawn on the device from per-position targets, so two positions cannot be told to "
                                 "draw one transition")
        self._n_envs = _checked_int("n_envs", n_envs, 1)
        if capacity % n_envs != 0:
            raise ValueError("capacity = %d is not a multiple of n_envs = %d" % (capacity, n_envs))
        if n_envs > 1 and dedup_frames:
            raise ValueError("n_envs > 1 is not combined with dedup_frames=True (the frame store matches recent frames "
                             "per stream)")
        self._pos_offset = _checked_int("pos_offset", pos_offset, 0)
        self.n_step = _checked_int("n_step", n_step, 1)
        self.discount = _checked_discount(discount) if self.n_step > 1 else discount
        # the continuity flags serve both chain walks: the n-step composition and a positive more than one step ahead
        self._keep_cont = self.n_step > 1 or self._pos_offset > 1
        self.prioritized = bool(prioritized)
        if self.prioritized:
            _checked_per(per_alpha, per_beta, per_eps)
        self.per_alpha, self.per_beta, self.per_eps = per_alpha, per_beta, per_eps
        self.capacity = capacity
        self.batch_size = batch_size
        self.device = torch.device(device)
        self.augmentor = augmentor
        self.transform = transform
        if len(obs_shape) != 3:
            raise NotImplementedError("curla_amd.ReplayBuffer stores pixel observations (C, H, W) only")
        c, h, w = obs_shape
        self.obs_shape = tuple(obs_shape)
        self._frame = frame = c * h * w
        self._n_act = A = int(np.prod(action_shape))
        self.dedup_frames = bool(dedup_frames)
        # How a minibatch of this augmentation is sampled -- "ring", "scratch" or "float" -- and the int32 words it draws
        # per sample and tensor: the object says (the protocol at IdentityAugmentation).  None: an object that says nothing
        # (draw_indices raises).
        self._kind = getattr(augmentor, "sample_kind", None)
        self._index_rows = augmentor.index_rows if self._kind else 0
        assert self._kind in ("ring", "scratch", "float", None) and self._index_rows in (0, 2, 4, 6)
        # float augmentations only: the parameters travel in the index block, NoisyCover's noise is drawn in the kernel
        self.staged_aug = bool(staged_aug) and self._kind == "float"
        if self.staged_aug:
            augmentor.check_staged(c * h * w * batch_size, self._noise_generator)
        if self.dedup_frames:
            if c % 3 != 0:
                raise ValueError("dedup_frames needs stacked RGB frames (channels a multiple of 3)")
            self._k = c // 3
            if frame_capacity is None:  # one new frame per step + one extra per episode start, with headroom
                frame_capacity = capacity + capacity // 16 + 4 * self._k + 8
            self.frame_capacity = int(frame_capacity)
            total_bytes = self.frame_capacity * 3 * h * w + capacity * (8 * self._k + 4 * A + 8) \
                + self.N_SAMPLE_SLOTS * (3 if self._pos_offset else 2) * batch_size * frame
        else:
            total_bytes = 2 * capacity * frame + capacity * (4 * A + 8)
        if self._kind == "scratch":  # the augmented minibatches (obs | next_obs | pos) of the sample slots
            total_bytes += self.N_SAMPLE_SLOTS * (3 * batch_size * self._scratch_frame() + 32)
        if self._keep_cont:  # the continuity flags
            total_bytes += capacity
        if self.prioritized:  # the stored values and their chunk sums
            total_bytes += 4 * capacity + 8 * ops.per_chunks(capacity)
        if self.device.type == "cuda":
            free, _ = torch.cuda.mem_get_info(self.device)
            if total_bytes > free:
                raise ValueError('Replay buffer size exceeds available memory')  # utils.py:112-113
        self._alloc_storage(action_shape)
        self._alloc_add_slots()
        self._alloc_sample_slots()

    def _alloc_storage(self, action_shape):
        """The transitions themselves: the rings (or the frame store and its frame-id rows), the scalar rows and, for a
        prioritized buffer, the stored values; the write head."""
        (c, h, w), frame, A = self.obs_shape, self._frame, self._n_act
        capacity, dev = self.capacity, self.device
        if self.dedup_frames:
            # every RGB frame once: uint8 [F][H][W][3] (+32 B slack like a ring); a transition keeps 2k frame ids
            f3 = 3 * h * w
            self._frame_store = torch.zeros(self.frame_capacity * f3 + 32, dtype=torch.uint8, device=dev)
            self.frames = self._frame_store[:self.frame_capacity * f3].view(self.frame_capacity, h, w, 3)
            self._fid = torch.zeros((capacity, 2, self._k), dtype=torch.int32, device=dev)
            self._fid_h = np.full((capacity, 2, self._k), -1, dtype=np.int32)
            self._store = _FrameStore(self.frame_capacity, recent=2 * self._k + 2)
            self.obses = self.next_obses = None  # stacks are assembled per minibatch (stack(i) materialises one)
        else:
            # ring storage: NHWC uint8 frames (+32 B slack: the aligning loader reads whole 16-byte runs plus a dword).
            # Both rings live in ONE allocation, next_obs behind obs, so that slot i of next_obs is also frame
            # capacity + i of a single [2 * capacity] ring: a minibatch's obs and next_obs can then be read by one
            # first-layer launch (ObsRef.pair) -- both go through the same online conv weights in the critic phase.
            # (only when the second half then starts on a dword, which the first-layer loader needs of a ring base)
            self._both = None
            if (capacity * frame) % 4 == 0:
                self._ring_store = torch.zeros(2 * capacity * frame + 32, dtype=torch.uint8, device=dev)
                self._obs_store = self._ring_store[:capacity * frame]
                self._next_store = self._ring_store[capacity * frame:2 * capacity * frame]
                self._both = self._ring_store[:2 * capacity * frame].view(2 * capacity, h, w, c)
                self.obses = self._both[:capacity]
                self.next_obses = self._both[capacity:]
            else:
                self._obs_store = torch.zeros(capacity * frame + 32, dtype=torch.uint8, device=dev)
                self._next_store = torch.zeros(capacity * frame + 32, dtype=torch.uint8, device=dev)
                self.obses = self._obs_store[:capacity * frame].view(capacity, h, w, c)
                self.next_obses = self._next_store[:capacity * frame].view(capacity, h, w, c)
        # action | reward | not_done of a transition sit in one row, so add() writes them with one small copy;
        # the three reference attributes are column views of it
        self._sc = torch.empty((capacity, A + 2), dtype=torch.float32, device=dev)
        self.actions = self._sc[:, :A].unflatten(1, tuple(action_shape)) if len(action_shape) != 1 else self._sc[:, :A]
        self.rewards = self._sc[:, A:A + 1]
        self.not_dones = self._sc[:, A + 1:A + 2]
        if self.prioritized:
            # stored values p^alpha, one float64 sum per chunk of ops.PER_CHUNK rows, the largest value given so far
            self._per_s = torch.zeros(capacity, dtype=torch.float32, device=dev)
            self._per_sums = torch.zeros(ops.per_chunks(capacity), dtype=torch.float64, device=dev)
            self._per_max = torch.ones(1, dtype=torch.float32, device=dev)
        self.idx = 0
        self.last_save = 0
        self.full = False

    @property
    def pos_offset(self):
        """k of the temporal positive (class docstring); fixed at construction: it decides the block layout."""
        return self._pos_offset

    @property
    def n_envs(self):
        """Environments that share the ring (class docstring); fixed at construction: it decides the row layout."""
        return self._n_envs

    @property
    def aug_views(self):
        """Augmented views per drawn transition, 1 or 2 (class docstring); fixed at construction."""
        return self._aug_views

    # ------------------------------------------------------------------ persistence
    def stacks(self, lo, hi, which=0):
        """Transitions [lo, hi) as the reference stores them: a (hi-lo, C, H, W) uint8 NumPy array of obs
        (which=0) or next_obs (which=1) stacks."""
        c, h, w = self.obs_shape
        n = hi - lo
        if n <= 0:
            return np.empty((0, c, h, w), dtype=np.uint8)
        if self.dedup_frames:
            rows = torch.arange(lo, hi, device=self.device, dtype=torch.int64)
            buf = torch.zeros(n * self._frame + 32, dtype=torch.uint8, device=self.device)
            out = buf[:n * self._frame].view(n, h, w, c)
            ops.gather_stacks(self.frames, self._fid[:, which, :], rows, n, out)
            ring = out
        else:
            ring = (self.obses, self.next_obses)[which][lo:hi]
        return ring.permute(0, 3, 1, 2).contiguous().cpu().numpy()

    def save(self, save_dir):
        """utils.py:189-202: the transitions added since the last call go to one file ``{start}_{end}.pt`` whose
        payload is the reference's (five arrays, observation stacks as CHW uint8)."""
        lo, hi = self.last_save, self.idx
        if lo == hi:
            return
        payload = [self.stacks(lo, hi, 0), self.stacks(lo, hi, 1)]
        payload += [t[lo:hi].cpu().numpy() for t in (self.actions, self.rewards, self.not_dones)]
        self.last_save = hi
        torch.save(payload, os.path.join(save_dir, '%d_%d.pt' % (lo, hi)))

    def load(self, save_dir):
        """utils.py:204-216: read the ``{start}_{end}.pt`` files of ``save_dir`` back in ascending order of
        ``start``; each file must continue where the previous one ended."""
        def span(name):
            lo, hi = os.path.splitext(name)[0].split('_')
            return int(lo), int(hi)

        for name in sorted(os.listdir(save_dir), key=lambda n: span(n)[0]):
            lo, hi = span(name)
            if lo != self.idx:
                raise AssertionError("chunk %s does not continue the buffer at index %d" % (name, self.idx))
            if lo % self._n_envs or hi % self._n_envs:
                raise ValueError("chunk %s does not hold whole vector steps of n_envs = %d" % (name, self._n_envs))
            obs, nxt, act, rew, nd = torch.load(os.path.join(save_dir, name), weights_only=False)
            if self.dedup_frames:  # (prioritized: every add of the loop gives its row the maximum)
                self.add_batch(obs, act, rew, nxt, 1.0 - np.asarray(nd))
                self.idx = hi  # (the reference's load does not wrap either)
                continue
            if hi > self.capacity or len(obs) != hi - lo:  # (before anything is written)
                raise RuntimeError("chunk %s holds %d transitions for rows %d .. %d of a ring of %d: load() does not wrap"
                                   % (name, len(obs), lo, hi - 1, self.capacity))
            self._write_rows(lo, obs, act, rew, nxt, nd)
            self.idx = hi

    def __len__(self):
        return self.capacity
