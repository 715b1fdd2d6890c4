"""Replay buffer and small helpers of the learner path (reference: utils.py).

``ReplayBuffer`` keeps the reference's constructor, ``add``, ``sample_cpc``,
``save``/``load``, ``idx``/``full`` -- but the ring lives in HBM (uint8, NHWC so
a cropped row is one contiguous run) and sampling hands the learner *references*
(frame indices + crop offsets) instead of materialised float tensors: the
reference's 3 x B x C x H x W float32 host->device copy per update (utils.py:161-166)
disappears.  Index and crop-offset draws stay on the host in NumPy's legacy
global stream, in the reference's order, so a seeded run samples the same
transitions and windows (bit-exact).

``dedup_frames=True`` stores every RGB frame once: a frame
stack of k frames shares k-1 of them with its successor and ``next_obs[t]`` is
``obs[t+1]`` inside an episode (utils.py:238-268), so an environment step adds
ONE new frame instead of 2k -- 63.5 KB -> 21 KB per transition at 84x84x9,
339 KB -> 85 KB at 168x168x12.  Sharing is detected from the bytes handed to
``add`` (hash, then full comparison), never assumed, so sampled pixels are the
reference's whatever the caller does.

``staged_aug=True`` (float augmentations: ColorJiggle, NoisyCover, RandomConv)
sends the random parameters of a minibatch's three tensors along in the index
block instead of through a pinned block and a copy of their own per tensor, and
lets NoisyCover draw its noise inside the cover kernel: with it -- and for ``dedup_frames`` without it -- the
minibatch can be a node of a captured update graph (``graph_supported``).
"""
import collections
import os
import random

import numpy as np
import torch

from . import ops

try:  # 64-bit frame fingerprints for the de-duplicating store (~10 GB/s); zlib is the slower stand-in
    from xxhash import xxh3_64_intdigest as _fingerprint
except ImportError:  # pragma: no cover
    import zlib

    def _fingerprint(buf):
        return zlib.crc32(buf) | (zlib.adler32(buf) << 32)


def _checked_discount(d):
    """``discount`` of an n-step ReplayBuffer as a float; ValueError unless it is a number in (0, 1]."""
    if isinstance(d, bool) or not isinstance(d, (int, float, np.floating, np.integer)) or not 0.0 < float(d) <= 1.0:
        raise ValueError("n_step > 1 needs discount, a float in (0, 1] (the agent's), got %r" % (d,))
    return float(d)


def _lib_tracing():
    from . import _lib
    return _lib._trace_hook is not None


class eval_mode(object):
    """Context manager that puts the given models (anything with ``.training`` and ``.train(bool)``) in
    evaluation mode and restores each one's previous mode on exit (utils.py:21-34)."""

    def __init__(self, *models):
        self.models = models
        self._was_training = None

    def __enter__(self):
        self._was_training = [m.training for m in self.models]
        for m in self.models:
            m.train(False)

    def __exit__(self, *exc):
        for m, mode in zip(self.models, self._was_training):
            m.train(mode)
        return False


def soft_update_params(net, target_net, tau):
    """utils.py:37-41, one fused lerp kernel per tensor.  CurlSacAgent uses the
    flat-buffer form (``soft_update_targets``): two launches for all 24 tensors."""
    for param, target_param in zip(net.parameters(), target_net.parameters()):
        ops.soft_update(param.data.view(-1), target_param.data.view(-1), tau)


def set_seed_everywhere(seed):
    """utils.py:44-49."""
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)
    np.random.seed(seed)
    random.seed(seed)


def make_dir(dir_path):
    """Create ``dir_path`` unless it exists; like the reference (utils.py:61-66) a failure is reported, not raised,
    and the path is returned either way."""
    if not os.path.isdir(dir_path):
        try:
            os.mkdir(dir_path)
        except OSError as e:
            print('Unable to create directory %s (%s)' % (dir_path, e.strerror))
    return dir_path


def module_hash(module):
    """Sum of the sums of a module's state_dict tensors -- the reference's cheap "did the weights change" number
    (utils.py:50-54)."""
    return sum(t.sum().item() for t in module.state_dict().values())


def preprocess_obs(obs, bits=5):
    """Bit-depth reduction with uniform dequantisation noise, arXiv:1807.03039 (utils.py:67-77; unused by the
    learner path, kept so that ``utils.`` resolves every name the reference module has)."""
    assert obs.dtype == torch.float32
    bins = 2 ** bits
    if bits < 8:
        obs = torch.floor(obs / 2 ** (8 - bits))
    return obs / bins + torch.rand_like(obs) / bins - 0.5


class FrameStack(object):
    """Observation wrapper that returns the last ``k`` frames concatenated on the channel axis (utils.py:238-268):
    ``reset`` fills the stack with k copies of the first frame, ``step`` pushes the new frame.  Plain duck-typed
    wrapper (``gymnasium`` is only used for the observation space when it is importable): every other attribute
    is forwarded to the wrapped environment, as ``gym.Wrapper`` does."""

    def __init__(self, env, k):
        self.env = env
        self._k = k
        self._frames = collections.deque([], maxlen=k)
        space = getattr(env, "observation_space", None)
        shp = tuple(getattr(space, "shape", ()))
        if shp:
            stacked = (shp[0] * k,) + shp[1:]
            try:
                import gymnasium
                self.observation_space = gymnasium.spaces.Box(low=0, high=1, shape=stacked, dtype=space.dtype)
            except ImportError:
                self.observation_space = type("Box", (), dict(shape=stacked, dtype=getattr(space, "dtype", np.uint8),
                                                              low=0, high=1))()
        self._max_episode_steps = getattr(env, "_max_episode_steps", None)
        self.curl_driving = False

    def __getattr__(self, name):  # only called for attributes not found on the wrapper itself
        if name in ("env", "_frames"):
            raise AttributeError(name)
        return getattr(self.env, name)

    def reset(self):
        first = self.env.reset()
        self.curl_driving = getattr(self.env, "curl_driving", False)
        self._frames.extend([first] * self._k)
        return self._get_obs()

    def step(self, action):
        frame, reward, done, info = self.env.step(action)
        self.env.curl_driving = self.curl_driving
        self._frames.append(frame)
        return self._get_obs(), reward, done, info

    def _get_obs(self):
        assert len(self._frames) == self._k
        return np.concatenate(list(self._frames), axis=0)


class _FrameStore:
    """Host-side bookkeeping of the de-duplicating frame store: reference counts, a free list and a small cache of
    the most recently interned frames (hash -> (frame id, bytes)) that new frames are matched against."""

    def __init__(self, n_frames, recent):
        self.refs = np.zeros(n_frames, dtype=np.int32)
        self.free = collections.deque(range(n_frames))
        self.recent = collections.OrderedDict()  # fingerprint -> (fid, ndarray copy)
        self.max_recent = recent

    def lookup(self, frame):
        """(fid or None, fingerprint) of a (3, H, W) uint8 frame among the recent ones -- byte-exact."""
        h = _fingerprint(frame)
        hit = self.recent.get(h)
        if hit is not None and np.array_equal(hit[1], frame):
            self.recent.move_to_end(h)
            return hit[0], h
        return None, h

    def allocate(self, frame, h):
        if not self.free:
            raise MemoryError("frame store exhausted: the observations handed to add() share fewer frames than a "
                              "frame-stacked episode does; raise frame_capacity or construct the ReplayBuffer with "
                              "dedup_frames=False")
        fid = self.free.popleft()
        self.recent[h] = (fid, np.array(frame, copy=True))
        while len(self.recent) > self.max_recent:
            self.recent.popitem(last=False)
        return fid

    def release(self, fid):
        self.refs[fid] -= 1
        if self.refs[fid] == 0:
            self.free.append(fid)
            for h, (f, _) in list(self.recent.items()):
                if f == fid:
                    del self.recent[h]


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


class ReplayBuffer(object):
    """Buffer to store environment transitions (utils.py:80-236), HBM-resident.

    ``n_step=n > 1`` (beyond the reference; DrQ-v2 uses 3) makes every sample an n-step transition: reward becomes
    ``sum_{k<m} discount^k r_{t+k}``, not_done ``not_done_{t+m-1} discount^(m-1)`` and next_obs the one of row
    ``t+m-1``, ``m <= n`` being the steps the episode still has from row t on -- so the learner's unchanged
    ``reward + not_done * discount * (...)`` is the n-step TD target.  ``discount`` is then required and must be the
    agent's (``CurlSacAgent.update`` checks it); it is a plain attribute, read at every sample.  Which row continues
    which is detected from the data handed to ``add`` (a per-row flag ``cont``): row i continues into row i + 1 when
    that was the very next add, ``done`` was false and row i's ``next_obs`` equals row i + 1's ``obs`` byte for byte --
    a time-limit truncation or a reset breaks the chain without a change to ``add``'s signature.  A caller that
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
    The walk happens on the device, in the staging launch of the minibatch (curla_sample_stage_pos; curla_pos_walk where the block travels by copy), so the host draws exactly what
    it draws with ``pos_offset=0``: a seeded run samples the same transitions with the same three augmentation draws,
    only the positive's pixels differ, and ``cpc_kwargs`` keeps ``time_anchor=None, time_pos=None``.  This is ATC's
    positive SELECTION behind CURL's own bilinear head and momentum encoder -- not ATC's residual predictor.  Read-only
    after construction (it decides the block layout).  ``pos_offset=0`` (default): nothing is allocated, launched or laid
    out differently.

    ``n_envs=N > 1`` (beyond the reference) stores the steps of N environments that act side by side: ``add_vec`` takes one
    step of all of them -- N observations, actions, rewards, next observations and dones -- and writes it in one launch.
    Environment e at vector step t owns ring row ``(t * N + e) % capacity``, so each environment is a lane of stride N,
    ``capacity`` must be a multiple of N and ``idx`` always is one (a vector step never straddles the ring's end).
    ``cont[r] == 1`` then means that row ``(r + N) % capacity`` continues row r's episode, and the n-step composition and
    the positive's walk advance by N rows: ``n_step`` and ``pos_offset`` work per environment.  The rule stays derived
    from the data, per lane: lane e continues when the previous write was the vector step directly before, that step's
    stored ``not_done[e]`` is 1 and its ``next_obs[e]`` equals the new ``obs[e]`` byte for byte -- an auto-resetting
    vector environment hands back a reset stack and so breaks the chain by itself, as a time-limit truncation does.  The
    newest N rows always carry flag 0.  ``add`` refuses such a buffer; ``add_batch`` and ``load`` take whole vector steps
    in row order (step-major, environment-minor).  Not combined with ``dedup_frames`` (its match of recent frames is
    per stream).  Read-only after construction.  ``n_envs=1`` (default): nothing is allocated, launched or laid out
    differently."""

    N_SAMPLE_SLOTS = 2  # minibatches whose references may be alive at once (the current one + one drawn ahead)
    EVENT_EVERY = 8     # index uploads per recorded event (16 pinned slots)
    # The block of a captured update graph carries GRAPH_TAIL bytes of per-update control values behind the indices:
    # u64[4] (seed, critic-noise offset, seed, actor-noise offset) | f64[2] log_alpha | f32[8] four Adams
    GRAPH_TAIL = 80
    GUARD, GUARD_BYTE = 256, 0xA5  # around a graph slot's minibatch buffers (_guarded)

    def __init__(self, obs_shape, action_shape, capacity, batch_size, device, augmentor, transform=None,
                 dedup_frames=False, frame_capacity=None, staged_aug=False, n_step=1, discount=None,
                 prioritized=False, per_alpha=0.6, per_beta=0.4, per_eps=1e-6, pos_offset=0, n_envs=1):
        if isinstance(n_envs, bool) or not isinstance(n_envs, (int, np.integer)) or n_envs < 1:
            raise ValueError("n_envs must be an int >= 1, got %r" % (n_envs,))
        if capacity % n_envs != 0:
            raise ValueError("capacity = %d is not a multiple of n_envs = %d" % (capacity, n_envs))
        if n_envs > 1 and dedup_frames:
            raise ValueError("n_envs > 1 is not combined with dedup_frames=True (the frame store matches recent frames "
                             "per stream)")
        self._n_envs = N = int(n_envs)
        if isinstance(pos_offset, bool) or not isinstance(pos_offset, (int, np.integer)) or pos_offset < 0:
            raise ValueError("pos_offset must be an int >= 0, got %r" % (pos_offset,))
        self._pos_offset = int(pos_offset)
        if isinstance(n_step, bool) or not isinstance(n_step, (int, np.integer)) or n_step < 1:
            raise ValueError("n_step must be an int >= 1, got %r" % (n_step,))
        self.n_step = int(n_step)
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
        frame = c * h * w
        A = int(np.prod(action_shape))
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
        dev = self.device
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
        self._n_act = A
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
        # staging: pinned host rows for add(), device index buffers for sampling
        pin = self.device.type == "cuda"
        # add(): one pinned block per slot = [frames | pad | frame ids, action, reward, not_done], a few slots
        # guarded by events so that add() never waits for the GPU; one device block receives the copy
        self._frame = frame
        # (n_envs = N > 1, add_vec(): [N obs | N next_obs | pad | N scalar rows | 2N flags], curla_add_vec's block)
        n_stage = 2 * N * frame  # plain: the two stacks; dedup: up to 2k new RGB frames = the same bytes
        self._sc_off = (n_stage + 15) & ~15
        self._hdr = 4 * (2 * self._k) if self.dedup_frames else 0  # frame-id row in front of the scalars
        blk = self._sc_off + self._hdr + 4 * N * (A + 2)
        if self._keep_cont:
            # cont[i] = 1: row (i + 1) % capacity continues row i's episode (class docstring).  The flags of the previous
            # row and of the new one (always 0) ride behind the scalars of the add block; the host keeps a mirror and
            # what it needs of the previous add to evaluate the rule.
            self._cont = torch.zeros(capacity, dtype=torch.uint8, device=dev)
            self._cont_h = np.zeros(capacity, dtype=np.uint8)
            # (n_envs = N > 1: row (i + N) % capacity, and N flags each for the previous vector step and the new one)
            self._cont_off = blk
            blk += (2 * N + 3) & ~3
            self._last_row = None   # the row the latest add wrote (n_envs > 1: the first row of the latest vector step)
            self._last_nd = False   # ... its stored not_done == 1 (bulk writes and add_vec: a bool per lane)
            self._last_next = None  # ... its next_obs bytes (plain ring; the frame store compares frame ids)
        self._n_add, self._add_slot = 4, 0
        self._h_add = torch.empty((self._n_add, blk), dtype=torch.uint8, pin_memory=pin)
        self._h_add_np = self._h_add.numpy()
        self._add_events = [None] * self._n_add
        self._d_add = torch.empty(blk, dtype=torch.uint8, device=dev)
        # the staged frames (plain: the two stacks; frame store: up to 2k RGB frames) as views made once
        self._d_add_frames = self._d_add[:2 * frame].view(-1, 3 * h * w if self.dedup_frames else frame).unbind(0)
        self._d_add_sc = self._d_add[self._sc_off + self._hdr:self._sc_off + self._hdr + 4 * (A + 2)].view(torch.float32)
        B = batch_size
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
        # ``ar2`` = rows 0..2B-1 (frame store; pos_offset > 0: 0..3B-1), ``shift_u8`` the frames of a "scratch" augmentation,
        # ``both_f32`` / ``pos_f32``
        # the float tensors (absent here: allocated per call).  The rotating slots are views of the stores above; a
        # captured update graph has slots of its own with the same keys (graph_block).
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

    @property
    def pos_offset(self):
        """k of the temporal positive (class docstring); fixed at construction: it decides the block layout."""
        return self._pos_offset

    @property
    def n_envs(self):
        """Environments that share the ring (class docstring); fixed at construction: it decides the row layout."""
        return self._n_envs

    # ------------------------------------------------------------------ writing
    def _stage_scalars(self, row, action, reward, done):
        A = self._n_act
        at = self._sc_off + self._hdr
        sc = row[at:at + 4 * (A + 2)].view(np.float32)
        sc[:A] = np.asarray(action, dtype=np.float32).reshape(-1)
        sc[A] = float(reward)
        sc[A + 1] = float(not done)
        return sc

    def _stage_cont(self, row, i, continues, not_done):
        """n-step bookkeeping of an add to row ``i``: ``continues`` = the new obs is the previous add's next_obs, byte
        for byte.  Sets the host flags (previous row by the rule, new row 0), puts the two bytes into the pinned add
        block ``row`` and returns the previous row (None: there is none to re-evaluate)."""
        p = self._last_row
        if p is not None and ((p + 1) % self.capacity != i or p == i):
            p = None
        flag = 0
        if p is not None:
            flag = int(bool(continues) and bool(self._last_nd))
            self._cont_h[p] = flag
        self._cont_h[i] = 0
        row[self._cont_off], row[self._cont_off + 1] = flag, 0
        self._last_row, self._last_nd = i, bool(not_done)
        return p

    def _store_cont(self, i, p):
        """Device side of _stage_cont, stream-ordered behind the add block's copy: one 2-byte copy (two of one byte
        where the pair straddles the ring's end)."""
        o = self._cont_off
        if p is None:
            self._cont[i:i + 1].copy_(self._d_add[o + 1:o + 2])
        elif p + 1 == i:
            self._cont[p:i + 1].copy_(self._d_add[o:o + 2])
        else:
            self._cont[p:p + 1].copy_(self._d_add[o:o + 1])
            self._cont[i:i + 1].copy_(self._d_add[o + 1:o + 2])

    def _next_add_slot(self):
        k = self._add_slot
        self._add_slot = (k + 1) % self._n_add
        if self._add_events[k] is not None:
            self._add_events[k].synchronize()
        return k

    def add(self, obs, action, reward, next_obs, done):
        """utils.py:120-128: store one transition at ``idx``.  The two frames and the scalars travel in one
        pinned block and one async copy; two kernels turn CHW into the ring's HWC, one row copy stores the
        scalars.  Nothing here waits for the GPU (a slot is reused only after its copy has executed)."""
        if self._n_envs > 1:
            raise ValueError("add() stores one transition; a buffer of n_envs = %d takes a whole vector step: add_vec()"
                             % self._n_envs)
        if self.dedup_frames:
            return self._add_dedup(obs, action, reward, next_obs, done)
        i = self.idx
        k = self._next_add_slot()
        fr = self._frame
        row = self._h_add_np[k]
        row[:fr] = np.asarray(obs, dtype=np.uint8).reshape(-1)
        row[fr:2 * fr] = np.asarray(next_obs, dtype=np.uint8).reshape(-1)
        sc = self._stage_scalars(row, action, reward, done)
        prev = None
        if self._keep_cont:  # one comparison of a frame on the host, against the copy kept of the previous next_obs
            same = self._last_next is not None and np.array_equal(row[:fr], self._last_next)
            prev = self._stage_cont(row, i, same, sc[self._n_act + 1] == 1.0)
            if self._last_next is None:
                self._last_next = np.empty(fr, dtype=np.uint8)
            self._last_next[:] = row[fr:2 * fr]
        self._commit_add(k, i, sc, prev, [(self._d_add, self._h_add[k])], [(self.obses, i), (self.next_obses, i)])

    def _commit_add(self, k, i, sc, prev, copies, frames):
        """What add() and _add_dedup() share once pinned block ``k`` is staged for row ``i``: the async ``copies``
        (device view, pinned view) and the event that guards the block, one store_frame per (ring, ring row) of
        ``frames`` -- the j-th staged frame goes to the j-th entry --, the frame-id row (frame store), the scalar row
        ``sc`` and the continuity flags (``prev``: _stage_cont)."""
        if self.device.type == "cuda":
            for dst, src in copies:
                dst.copy_(src, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._add_events[k] = ev
            for j, (ring, row) in enumerate(frames):
                ops.store_frame(self._d_add_frames[j], ring, row)
            if self.dedup_frames:
                self._fid[i].view(-1).copy_(self._d_add[self._sc_off:self._sc_off + self._hdr].view(torch.int32))
            self._sc[i].copy_(self._d_add_sc)
            if self._keep_cont:
                self._store_cont(i, prev)
            if self.prioritized:
                self._per_new_rows(i, 1)
        else:  # host-side bookkeeping only (index logic tests); pixels are still stored, HWC
            h, w = self.obs_shape[1:]
            n = self._d_add_frames[0].numel()
            for j, (ring, row) in enumerate(frames):
                ring[row] = self._h_add[k, j * n:(j + 1) * n].view(-1, h, w).permute(1, 2, 0)
            if self.dedup_frames:
                self._fid[i] = torch.from_numpy(self._fid_h[i].copy())
            self._sc[i] = torch.from_numpy(sc.copy())
            if self._keep_cont:
                for r in (i,) if prev is None else (prev, i):
                    self._cont[r] = int(self._cont_h[r])
            if self.prioritized and _lib_tracing():
                self._per_new_rows(i, 1)
        self._advance(1)

    def _vec_args(self, obs, action, reward, next_obs, done):
        """The five arguments of add_vec as NumPy arrays (N, C H W) uint8 twice, (N, A) float32, (N,) float32 and
        (N,) bool; ValueError when a leading size is not n_envs or a shape does not fit."""
        N, A = self._n_envs, self._n_act
        got = [np.asarray(obs), np.asarray(action), np.asarray(reward), np.asarray(next_obs), np.asarray(done)]
        want = [(N,) + self.obs_shape, (N, A), (N,), (N,) + self.obs_shape, (N,)]
        if not all(g.ndim >= 1 and g.shape[0] == N and g.size == int(np.prod(w)) for g, w in zip(got, want)):
            raise ValueError("add_vec of an n_envs = %d buffer takes obs and next_obs %r uint8, action %r (or (%d,) + "
                             "action_shape), reward and done %r; got %s"
                             % (N, want[0], want[1], N, want[2], ", ".join(str(g.shape) for g in got)))
        o, a, r, n, d = got
        return (np.asarray(o, dtype=np.uint8).reshape(N, -1), np.asarray(a, dtype=np.float32).reshape(N, A),
                np.asarray(r, dtype=np.float32).reshape(N), np.asarray(n, dtype=np.uint8).reshape(N, -1),
                d.reshape(N) != 0)

    def add_vec(self, obs, action, reward, next_obs, done):
        """One step of the buffer's ``n_envs = N`` environments: ``obs`` / ``next_obs`` (N, C, H, W) uint8, ``action``
        (N, A) or (N,) + action_shape, ``reward`` and ``done`` (N,).  Environment e goes to ring row ``idx + e``; the
        continuity flags of the previous vector step are set per lane by the rule of the class docstring.  The 2N
        frames, the N scalar rows and the 2N flag bytes travel in one pinned block and one async copy, and ONE launch
        (curla_add_vec) stores them all; nothing here waits for the GPU (the rotating pinned slots and events of
        ``add``).  On an ``n_envs=1`` buffer this is ``add`` of the one transition."""
        obs, action, reward, next_obs, done = self._vec_args(obs, action, reward, next_obs, done)
        N, A = self._n_envs, self._n_act
        if N == 1:
            return self.add(obs[0].reshape(self.obs_shape), action[0], reward[0], next_obs[0].reshape(self.obs_shape),
                            done[0])
        i, fr, cap = self.idx, self._frame, self.capacity
        k = self._next_add_slot()
        row = self._h_add_np[k]
        row[:N * fr] = obs.reshape(-1)
        row[N * fr:2 * N * fr] = next_obs.reshape(-1)
        sc = row[self._sc_off:self._sc_off + 4 * N * (A + 2)].view(np.float32).reshape(N, A + 2)
        sc[:, :A], sc[:, A], sc[:, A + 1] = action, reward, ~done
        prev = None
        if self._keep_cont:  # N frame comparisons on the host, against the copy kept of the previous step's next_obs
            prev = self._last_row
            if prev is None or (prev + N) % cap != i or prev == i:
                prev = None
            flags = row[self._cont_off:self._cont_off + 2 * N]
            flags[:] = 0
            if prev is not None:
                flags[:N] = (self._last_next.reshape(N, fr) == obs).all(axis=1) & np.reshape(self._last_nd, N)
                self._cont_h[prev:prev + N] = flags[:N]
            self._cont_h[i:i + N] = 0
            self._last_row, self._last_nd, self._last_next = i, sc[:, A + 1] == 1.0, next_obs.reshape(-1).copy()
        if self.device.type == "cuda":
            self._d_add.copy_(self._h_add[k], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._add_events[k] = ev
        else:  # host-side bookkeeping only (index logic tests); pixels are still stored, HWC
            c, h, w = self.obs_shape
            for ring, frames in ((self.obses, obs), (self.next_obses, next_obs)):
                ring[i:i + N] = torch.from_numpy(frames.reshape(N, c, h, w)).permute(0, 2, 3, 1)
            self._sc[i:i + N] = torch.from_numpy(sc.copy())
            if self._keep_cont:
                for r in (i,) if prev is None else (prev, i):
                    self._cont[r:r + N] = torch.from_numpy(self._cont_h[r:r + N].copy())
        if self.device.type == "cuda" or _lib_tracing():
            ops.add_vec(self._d_add, self.obses, self.next_obses, self._sc, self._cont if self._keep_cont else None, i,
                        prev is not None, N)
            if self.prioritized:
                self._per_new_rows(i, N)
        self._advance(N)

    def _per_new_rows(self, first, n):
        """Rows first, first + 1, ... (n of them, modulo capacity) hold new transitions: they get the maximum stored
        value.  One curla_per_set, stream-ordered behind the rows' writes."""
        ops.per_set(self._per_s, self._per_sums, self._per_max, n, first_row=first)

    def _advance(self, n):
        new_idx = self.idx + n
        self.full = self.full or new_idx >= self.capacity
        self.idx = new_idx % self.capacity

    def _add_dedup(self, obs, action, reward, next_obs, done):
        """add() into the frame store: each of the 2k RGB frames of (obs, next_obs) is matched byte for byte
        against the recently stored ones (in a frame-stacked episode 2k-1 of them are), only the new ones are
        uploaded, and the transition records 2k frame ids."""
        c, h, w = self.obs_shape
        K, f3 = self._k, 3 * h * w
        i = self.idx
        st = self._store
        old = self._fid_h[i].reshape(-1)
        slot = self._next_add_slot()
        row = self._h_add_np[slot]
        ids, new = np.empty(2 * K, dtype=np.int32), []
        frames = np.concatenate([np.asarray(obs, dtype=np.uint8).reshape(K, 3, h, w),
                                 np.asarray(next_obs, dtype=np.uint8).reshape(K, 3, h, w)])
        # Room first, nothing touched yet: the frames this transition does not find in the store need a free slot
        # each (a frame repeated inside the transition is counted once per occurrence: an upper bound), and the
        # slots that the transition being overwritten (ring wrap) gives back count as free.  Failing here leaves the
        # store exactly as it was -- a caller that catches the MemoryError (add_batch / load loops) keeps a
        # consistent buffer.
        found = [st.lookup(frames[j])[0] for j in range(2 * K)]
        keeps = collections.Counter(f for f in found if f is not None)
        gives = collections.Counter(int(f) for f in old if f >= 0)
        freed = sum(1 for f, n in gives.items() if st.refs[f] - n + keeps.get(f, 0) == 0)
        if sum(f is None for f in found) > len(st.free) + freed:
            raise MemoryError("frame store exhausted: the observations handed to add() share fewer frames than a "
                              "frame-stacked episode does; raise frame_capacity or construct the ReplayBuffer with "
                              "dedup_frames=False")
        # 1. hold on to the frames that are already there, 2. let the overwritten transition go (frames it shares with
        #    the new one stay: held), 3. store the new frames -- in the slots step 2 may just have freed
        for f in found:
            if f is not None:
                st.refs[f] += 1
        for fid in old:
            if fid >= 0:
                st.release(int(fid))
        for j in range(2 * K):
            fid = found[j]
            if fid is None:
                fid, fp = st.lookup(frames[j])  # (an earlier frame of this transition may have just stored it)
                if fid is None:
                    fid = st.allocate(frames[j], fp)
                    row[len(new) * f3:(len(new) + 1) * f3] = frames[j].reshape(-1)
                    new.append(fid)
                st.refs[fid] += 1
            ids[j] = fid
        if self._keep_cont:  # equal bytes have equal frame ids: the new obs row against the previous next_obs row
            p = self._last_row
            same = p is not None and p != i and np.array_equal(ids[:K], self._fid_h[p, 1])
        self._fid_h[i] = ids.reshape(2, K)
        row[self._sc_off:self._sc_off + self._hdr].view(np.int32)[:] = ids
        sc = self._stage_scalars(row, action, reward, done)
        prev = self._stage_cont(row, i, same, sc[self._n_act + 1] == 1.0) if self._keep_cont else None
        # two partial copies: the new frames (if any), then frame ids | scalars | flags
        n = len(new) * f3
        copies = [(self._d_add[:n], self._h_add[slot, :n])] if n else []
        copies.append((self._d_add[self._sc_off:], self._h_add[slot, self._sc_off:]))
        self._commit_add(slot, i, sc, prev, copies, [(self.frames, fid) for fid in new])

    def _cont_rows(self, first, obs, nxt, not_done):
        """n-step bookkeeping of a bulk write (add_batch, load): transitions ``obs`` / ``nxt`` ((m, C, H, W) uint8 host
        arrays) with ``not_done`` (m values) go to rows first, first + 1, ... (mod capacity), in this order -- the rule
        of add() applied to the arrays, the pair (previous add, first element) included.  With ``n_envs = N`` the rows
        are whole vector steps (m and first multiples of N): element j continues into element j + N, its lane's next
        step, and the pair (previous write, first step of the batch) is evaluated per lane."""
        N = self._n_envs
        m = len(obs)
        if m == 0:
            return
        obs = np.asarray(obs, dtype=np.uint8).reshape(m, -1)
        nxt = np.asarray(nxt, dtype=np.uint8).reshape(m, -1)
        nd = np.asarray(not_done, dtype=np.float32).reshape(m) == 1.0
        cap = self.capacity
        rows = (first + np.arange(m)) % cap
        flags = np.zeros(m, dtype=np.uint8)
        flags[:-N] = (nxt[:-N] == obs[N:]).all(axis=1) & nd[:-N]
        touched = rows
        p = self._last_row
        if p is not None and (p + N) % cap == rows[0] and m < cap:  # (m >= cap: the batch overwrites row p itself)
            prev = p + np.arange(N)
            self._cont_h[prev] = 0
            if self._last_next is not None:
                self._cont_h[prev] = (self._last_next.reshape(N, -1) == obs[:N]).all(axis=1) & np.reshape(self._last_nd, N)
            touched = np.concatenate([prev, rows])
        self._cont_h[rows] = flags  # (a row written twice keeps its last flag)
        self._last_row, self._last_nd = int(rows[-N]), nd[-N:].copy()
        self._last_next = nxt[-N:].reshape(-1).copy()
        touched = np.unique(touched)
        self._cont[torch.from_numpy(touched).to(self.device)] = torch.from_numpy(self._cont_h[touched]).to(self.device)

    def add_batch(self, obses, actions, rewards, next_obses, dones):
        """Bulk fill (benchmarks / buffer load): N transitions, observations as
        (N, C, H, W) uint8 arrays.  Same ring semantics as N add() calls -- with ``n_envs > 1`` as len / n_envs
        add_vec() calls: whole vector steps in row order (step-major, environment-minor)."""
        n = len(obses)
        if n % self._n_envs != 0:
            raise ValueError("add_batch of an n_envs = %d buffer takes whole vector steps, got %d transitions"
                             % (self._n_envs, n))
        chunk = 1024 // self._n_envs * self._n_envs  # whole vector steps per chunk
        if self.dedup_frames:
            for j in range(n):
                self.add(obses[j], actions[j], float(np.asarray(rewards[j]).reshape(-1)[0]), next_obses[j],
                         bool(np.asarray(dones[j]).reshape(-1)[0]))
            return
        for s in range(0, n, chunk):
            e = min(n, s + chunk)
            m = e - s
            o = torch.from_numpy(np.ascontiguousarray(obses[s:e])).to(self.device).permute(0, 2, 3, 1)
            nx = torch.from_numpy(np.ascontiguousarray(next_obses[s:e])).to(self.device).permute(0, 2, 3, 1)
            slots = (torch.arange(m) + self.idx) % self.capacity
            slots_d = slots.to(self.device)
            self.obses[slots_d] = o
            self.next_obses[slots_d] = nx
            self.actions[slots_d] = torch.as_tensor(np.asarray(actions[s:e], dtype=np.float32), device=self.device)
            self.rewards[slots_d] = torch.as_tensor(np.asarray(rewards[s:e], dtype=np.float32).reshape(m, 1),
                                                    device=self.device)
            nd = 1.0 - np.asarray(dones[s:e], dtype=np.float32).reshape(m, 1)
            self.not_dones[slots_d] = torch.as_tensor(nd, device=self.device)
            if self._keep_cont:
                self._cont_rows(self.idx, obses[s:e], next_obses[s:e], nd)
            if self.prioritized and (self.device.type == "cuda" or _lib_tracing()):
                self._per_new_rows(self.idx, m)
            self._advance(m)

    def frames_in_use(self):
        """(dedup_frames) RGB frames currently held / the store's capacity."""
        return self.frame_capacity - len(self._store.free), self.frame_capacity

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
        r % 2): the move's offsets, the box's (y0, x0), its sizes and colours -- or RandomAffine's six words of the map, m00 m01 | m02 m10 | m11 m12.
        ``prioritized``: returns (u, offsets), u float64 [B] the stratified targets (k + r_k) / B with
        r = np.random.random_sample(B) drawn where the rows are drawn otherwise -- the rows themselves are drawn by
        curla_per_sample from u."""
        B = self.batch_size
        if self.prioritized:
            # the stratified targets instead of the rows: u_k = (k + r_k) / B; the rows are drawn on the device
            if not self.full and self.idx == 0:
                raise ValueError("cannot sample an empty prioritized buffer")
            idxs = (np.arange(B) + np.random.random_sample(B)) / B
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
        one launch of n = 3B.  One that draws six -- Compose, RandomAffine -- appends ``cut`` int32 [4][3B]: the third to sixth words, the
        box's y0 | x0 | sizes | colours, or the map's m02 | m10 | m11 | m12.
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
            if self._pos_offset and want_pos:  # ... and so must the positive's rows (behind the draw, which writes the idx run)
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
        """Graph replay covers every minibatch whose per-update values reach the kernels through the block: the uint8-ring
        ones (RandomCrop / RandomShift / RandomCutout / RandomTranslate / RandomFlip / RandomRotate / RandomGrayscale / RandomAffine / identity; plain storage with both rings in one allocation, or ``dedup_frames``, whose stacks
        are gathered into a buffer of the graph's own), and ColorJiggle / NoisyCover / RandomConv constructed with
        ``staged_aug=True`` (either storage).  A ``prioritized`` buffer is not covered (its draw and its priority update are
        not nodes of the captured graphs).  A float augmentation WITHOUT staged_aug draws and uploads its parameters
        through a pinned block of its own per call and stays eager.  Pinned index slots read in place are required."""
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
            g = dict(host=host, host_dev=ops.host_device_pointer(host), dev=torch.zeros(nb, dtype=torch.uint8, device=self.device),
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
        the graph is replayed; three with pos_offset > 0), for RandomShift / RandomCutout / RandomTranslate the shift /
        cutout / translate launch (it
        reads its offsets, boxes and colours from the device block), for a
        staged float augmentation the three jitter / cover / convolution launches (they read their
        parameters from the device block), and the sample_cpc 6-tuple with handles into the slot's buffers.  Nothing
        here draws a random number."""
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
        ``cpc_kwargs["obs_pos"]`` is None.  Where the positive rides in a launch that runs anyway, that launch is unchanged."""
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
            to_ring = lambda a: torch.as_tensor(a).to(self.device).permute(0, 2, 3, 1)  # noqa: E731  CHW -> HWC
            self.obses[lo:hi] = to_ring(obs)
            self.next_obses[lo:hi] = to_ring(nxt)
            for dst, src in ((self.actions, act), (self.rewards, rew), (self.not_dones, nd)):
                dst[lo:hi] = torch.as_tensor(src).to(self.device)
            if self._keep_cont:  # the flags are rebuilt from the payload, never stored
                self._cont_rows(lo, obs, nxt, nd)
            if self.prioritized and hi > lo and (self.device.type == "cuda" or _lib_tracing()):
                self._per_new_rows(lo, hi - lo)  # priorities are not in the payload: the loaded rows get the maximum
            self.idx = hi

    def __len__(self):
        return self.capacity
