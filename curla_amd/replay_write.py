"""Write side of ``ReplayBuffer`` (replay.py): ``add``, ``add_vec`` and ``add_batch`` with their pinned staging slots,
the host bookkeeping of the de-duplicating frame store, and the ONE place that knows which row continues which."""
import collections

import numpy as np
import torch

from . import ops

try:  # 64-bit frame fingerprints for the de-duplicating store (~10 GB/s); zlib is the slower stand-in
    from xxhash import xxh3_64_intdigest as _fingerprint
except ImportError:  # pragma: no cover
    import zlib

    def _fingerprint(buf):
        return zlib.crc32(buf) | (zlib.adler32(buf) << 32)


def _lib_tracing():
    from . import _lib
    return _lib._trace_hook is not None


class _FrameStore:
    """Host-side bookkeeping of the de-duplicating frame store: reference counts, a free list and a small cache of
    the most recently interned frames (hash -> (frame id, bytes)) that new frames are matched against."""

    EXHAUSTED = ("frame store exhausted: the observations handed to add() share fewer frames than a frame-stacked episode "
                 "does; raise frame_capacity or construct the ReplayBuffer with dedup_frames=False")

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
            raise MemoryError(self.EXHAUSTED)
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


class _Chain:
    """The continuity rule (ReplayBuffer's docstring) of every write route, host only: row r continues into row
    ``(r + lanes) % capacity`` when the very next vector step wrote that row, ``not_done[r]`` is 1 and r's ``next_obs``
    key equals that row's ``obs`` key -- the stack's bytes on a plain ring, its k int32 frame ids on the frame store
    (equal bytes have equal ids there).  ``flags`` is the host mirror of ``ReplayBuffer._cont``; ``row``, ``nd`` and
    ``next`` are the last vector step written: its first row and, per lane, its not_done == 1 and its next_obs keys."""

    def __init__(self, capacity, lanes):
        self.capacity, self.lanes = capacity, lanes
        self.flags = np.zeros(capacity, dtype=np.uint8)
        self.row, self.nd, self.next = None, np.zeros(lanes, dtype=bool), None

    def write(self, first, obs, nxt, not_done):
        """Whole vector steps -- keys ``obs`` / ``nxt`` (m, L), ``not_done`` bool (m,) (or one bool for m = 1) -- go to
        rows first, first + 1, ... (mod capacity).  Sets the flags of the step written before, if this write follows it
        directly, and of the m rows: the link into the batch's next step, 0 for the newest step; a row written twice
        (m > capacity) keeps its last writer's.  Returns the first row of the step before if re-evaluated, else None."""
        N, cap, m = self.lanes, self.capacity, len(obs)
        step = m == N  # the common case, one vector step (it never straddles the ring's end): slices, nothing sized by m
        prev = self.row
        if prev is None or (prev + N) % cap != first or m >= cap:  # (m >= cap: the write overwrites that step itself)
            prev = None
        else:
            self.flags[prev:prev + N] = (self.next == (obs if step else obs[:N])).all(axis=1) & self.nd
        if self.next is None:
            self.next = np.empty((N,) + nxt.shape[1:], dtype=nxt.dtype)
        if step:
            self.flags[first:first + N] = 0
            self.row, self.nd[:], self.next[:] = first, not_done, nxt
        else:
            rows = (first + np.arange(m)) % cap
            flags = np.zeros(m, dtype=np.uint8)
            flags[:-N] = (nxt[:-N] == obs[N:]).all(axis=1) & not_done[:-N]
            self.flags[rows] = flags
            self.row, self.nd[:], self.next[:] = int(rows[-N]), not_done[-N:], nxt[-N:]
        return prev


class _ReplayWriteMixin:
    """ReplayBuffer's write routes; the state they use is the buffer's (allocated by ``_alloc_add_slots``)."""

    def _alloc_add_slots(self):
        """One pinned block per slot = [frames | pad | frame ids, action, reward, not_done | flags] (``n_envs = N``:
        [N obs | N next_obs | pad | N scalar rows | 2N flags], curla_add_vec's block), a few slots guarded by events so
        that an add never waits for the GPU; one device block receives the copy."""
        (_, h, w), frame, A, N = self.obs_shape, self._frame, self._n_act, self._n_envs
        dev = self.device
        n_stage = 2 * N * frame  # plain: the two stacks; dedup: up to 2k new RGB frames = the same bytes
        self._sc_off = (n_stage + 15) & ~15
        self._hdr = 4 * (2 * self._k) if self.dedup_frames else 0  # frame-id row in front of the scalars
        blk = self._sc_off + self._hdr + 4 * N * (A + 2)
        if self._keep_cont:
            # cont[i] = 1: row (i + N) % capacity continues row i's episode (_Chain; ``_cont_h`` is its array).  The N
            # flags of the previous vector step and the new one's (always 0) ride behind the scalars of the add block.
            self._cont = torch.zeros(self.capacity, dtype=torch.uint8, device=dev)
            self._chain = _Chain(self.capacity, N)
            self._cont_h = self._chain.flags
            self._cont_off = blk
            blk += (2 * N + 3) & ~3
        self._n_add, self._add_slot = 4, 0
        self._h_add = torch.empty((self._n_add, blk), dtype=torch.uint8, pin_memory=dev.type == "cuda")
        self._h_add_np = self._h_add.numpy()
        if self._keep_cont:
            self._h_add_np[:, self._cont_off:] = 0  # (the new step's flags: _stage_cont)
        self._add_events = [None] * self._n_add
        self._d_add = torch.empty(blk, dtype=torch.uint8, device=dev)
        # the staged frames (plain: the two stacks; frame store: up to 2k RGB frames) as views made once
        self._d_add_frames = self._d_add[:2 * frame].view(-1, 3 * h * w if self.dedup_frames else frame).unbind(0)
        self._d_add_sc = self._d_add[self._sc_off + self._hdr:self._sc_off + self._hdr + 4 * (A + 2)].view(torch.float32)

    def _stage_scalars(self, row, action, reward, done):
        A = self._n_act
        at = self._sc_off + self._hdr
        sc = row[at:at + 4 * (A + 2)].view(np.float32)
        sc[:A] = np.asarray(action, dtype=np.float32).reshape(-1)
        sc[A] = float(reward)
        sc[A + 1] = float(not done)
        return sc

    def _stage_cont(self, row, prev):
        """The previous vector step's N flags as ``_Chain.write`` just set them (``prev``; None: zeros, nothing reads
        them) into the pinned add block ``row``.  The N behind them, the new step's, stay 0 (_alloc_add_slots)."""
        N, o = self._n_envs, self._cont_off
        row[o:o + N] = 0 if prev is None else self._cont_h[prev:prev + N]

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
        """utils.py:120-128: store one transition at ``idx``.  The two frames and the scalars travel in one pinned block
        and one async copy; two kernels turn CHW into the ring's HWC, one row copy stores the scalars.  Nothing here
        waits for the GPU (a slot is reused only after its copy has executed)."""
        if self._n_envs > 1:
            raise ValueError("add() stores one transition; a buffer of n_envs = %d takes a whole vector step: add_vec()"
                             % self._n_envs)
        if self.dedup_frames:
            return self._add_dedup(obs, action, reward, next_obs, done)
        i = self.idx
        k = self._next_add_slot()
        fr = self._frame
        row = self._h_add_np[k]
        px = row[:2 * fr].reshape(2, 1, fr)
        px[0] = np.asarray(obs, dtype=np.uint8).reshape(-1)
        px[1] = np.asarray(next_obs, dtype=np.uint8).reshape(-1)
        sc = self._stage_scalars(row, action, reward, done)
        prev = None
        if self._keep_cont:  # one comparison of a frame on the host, against the chain's copy of the previous next_obs
            prev = self._chain.write(i, px[0], px[1], not done)
            self._stage_cont(row, prev)
        self._commit_add(k, i, sc, prev, [(self._d_add, self._h_add[k])], [(self.obses, i), (self.next_obses, i)])

    def _commit_add(self, k, i, sc, prev, copies, frames):
        """What add() and _add_dedup() share once pinned block ``k`` is staged for row ``i``: the async ``copies``
        (device view, pinned view) and the event that guards the block, one store_frame per (ring, ring row) of
        ``frames`` -- the j-th staged frame goes to the j-th entry --, the frame-id row (frame store), the scalar row
        ``sc`` and the continuity flags (``prev``: what ``_Chain.write`` returned)."""
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
            prev = self._chain.write(i, obs, next_obs, ~done)
            self._stage_cont(row, prev)
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
            raise MemoryError(st.EXHAUSTED)
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
        self._fid_h[i] = ids.reshape(2, K)
        row[self._sc_off:self._sc_off + self._hdr].view(np.int32)[:] = ids
        sc = self._stage_scalars(row, action, reward, done)
        prev = None
        if self._keep_cont:  # equal bytes have equal frame ids: the chain's keys are the two rows of k ids
            prev = self._chain.write(i, self._fid_h[i, :1], self._fid_h[i, 1:], not done)
            self._stage_cont(row, prev)
        # two partial copies: the new frames (if any), then frame ids | scalars | flags
        n = len(new) * f3
        copies = [(self._d_add[:n], self._h_add[slot, :n])] if n else []
        copies.append((self._d_add[self._sc_off:], self._h_add[slot, self._sc_off:]))
        self._commit_add(slot, i, sc, prev, copies, [(self.frames, fid) for fid in new])

    def _cont_rows(self, first, obs, nxt, not_done):
        """Continuity of a bulk write (``obs`` / ``nxt`` (m, C, H, W) uint8 host arrays, ``not_done`` m values):
        ``_Chain.write`` with the bytes as keys, then the rows it touched (the step before, if re-evaluated) to the
        device."""
        m, N = len(obs), self._n_envs
        if m == 0:
            return
        keys = lambda a: np.asarray(a, dtype=np.uint8).reshape(m, -1)  # noqa: E731
        prev = self._chain.write(first, keys(obs), keys(nxt), np.asarray(not_done, dtype=np.float32).reshape(m) == 1.0)
        touched = np.unique((first + np.arange(0 if prev is None else -N, m)) % self.capacity)
        self._cont[torch.from_numpy(touched).to(self.device)] = torch.from_numpy(self._cont_h[touched]).to(self.device)

    def _write_rows(self, first, obs, actions, rewards, nxt, not_dones):
        """A chunk of add_batch() or a file of load(): m transitions (host arrays, whole vector steps) go to rows first,
        first + 1, ... (mod capacity) -- rings and scalar columns by indexed stores, continuity flags, maximum priority."""
        m, dev = len(obs), self.device
        rows = ((torch.arange(m) + first) % self.capacity).to(dev)
        for ring, a in ((self.obses, obs), (self.next_obses, nxt)):  # CHW -> HWC
            ring[rows] = torch.from_numpy(np.ascontiguousarray(a)).to(dev).permute(0, 2, 3, 1)
        nd = np.asarray(not_dones, dtype=np.float32).reshape(m, 1)
        self.actions[rows] = torch.as_tensor(np.asarray(actions, dtype=np.float32), device=dev)
        self.rewards[rows] = torch.as_tensor(np.asarray(rewards, dtype=np.float32).reshape(m, 1), device=dev)
        self.not_dones[rows] = torch.as_tensor(nd, device=dev)
        if self._keep_cont:  # (load: the flags are rebuilt from the payload, never stored)
            self._cont_rows(first, obs, nxt, nd)
        if self.prioritized and m and (dev.type == "cuda" or _lib_tracing()):
            self._per_new_rows(first, m)  # (load: priorities are not in the payload, the loaded rows get the maximum)

    def add_batch(self, obses, actions, rewards, next_obses, dones):
        """Bulk fill (benchmarks / buffer load): N transitions, observations as (N, C, H, W) uint8 arrays.  Same ring
        semantics as N add() calls -- with ``n_envs > 1`` as len / n_envs add_vec() calls: whole vector steps in row
        order (step-major, environment-minor)."""
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
            self._write_rows(self.idx, obses[s:e], actions[s:e], rewards[s:e], next_obses[s:e],
                             1.0 - np.asarray(dones[s:e], dtype=np.float32))
            self._advance(e - s)

    def frames_in_use(self):
        """(dedup_frames) RGB frames currently held / the store's capacity."""
        return self.frame_capacity - len(self._store.free), self.frame_capacity

