"""The continuity rule of the replay buffer's write side on its own (``replay_write._Chain``; NumPy only -- nothing
here touches the library, a tensor or a buffer): scripted streams fed row by row, vector step by vector step and in
bulk give the flags of an oracle written from the script's links, after every write."""
import numpy as np
import pytest

from curla_amd.replay_write import _Chain

STEPS, RING = 12, 7  # vector steps of a script, vector steps the ring holds
# How a lane's episodes end: "done" (not_done = 0, a reset key next), "cut" (a time-limit truncation: not_done = 1, a
# reset key next), "same" (not_done = 0 although the next obs key IS this next_obs key: only not_done breaks the chain)
# and "open" (the stream goes on).  Lane 0 is test_nstep_host's SCRIPT with a "same" in it.
LANES = (((1, 2, 3, 2, 4), ("done", "cut", "same", "done", "open")),
         ((4, 3, 5), ("cut", "done", "open")),
         ((6, 1, 5), ("done", "cut", "open")))


def lane(lengths, ends, width, dtype, seed):
    """obs / next keys (STEPS, width) -- windows over a sequence of ids, as frame stacking makes them --, not_done and
    link: link[t] = 1 when step t + 1 continues step t."""
    ids = iter(range(1 + 40 * seed, 40 * (seed + 1)))  # every id once, below 256: distinct as uint8 too
    obs, nxt, nd, link = [], [], [], []
    carry = None
    for n, end in zip(lengths, ends):
        stack = carry if carry is not None else [next(ids)] * width
        for s in range(n):
            new = stack[1:] + [next(ids)]
            last = s == n - 1
            obs.append(stack), nxt.append(new)
            nd.append(not (last and end in ("done", "same")))
            link.append(0 if last and end != "open" else 1)
            stack = new
        carry = stack if end == "same" else None
    assert len(obs) == STEPS
    return np.array(obs, dtype=dtype), np.array(nxt, dtype=dtype), np.array(nd), np.array(link, dtype=np.uint8)


def script(N, width=4, dtype=np.uint8):
    """N lanes side by side, step-major: obs / nxt (STEPS, N, width), not_done and link (STEPS, N)."""
    return tuple(np.stack(a, axis=1) for a in zip(*(lane(*LANES[e], width, dtype, e) for e in range(N))))


def oracle(link, N, t_last):
    """After steps 0..t_last: a row carries its step's link, the newest step's rows 0; unwritten rows 0."""
    flags = np.zeros(RING * N, dtype=np.uint8)
    for t in range(t_last + 1):
        r = t * N % (RING * N)
        flags[r:r + N] = link[t] if t < t_last else 0
    return flags


def feed(chain, s, lo, hi):
    """Steps lo..hi-1 of script ``s`` in one write, behind step lo - 1; returns what write() returned."""
    N = chain.lanes
    obs, nxt, nd, _ = (a[lo:hi].reshape(((hi - lo) * N,) + a.shape[2:]) for a in s)
    return chain.write(lo * N % chain.capacity, obs, nxt, nd)


def test_the_script_has_every_kind_of_episode_end():
    obs, nxt, nd, link = script(3)
    assert obs.shape == nxt.shape == (STEPS, 3, 4) and obs.dtype == np.uint8
    assert link[:, 0].tolist() == [0, 1, 0, 1, 1, 0, 1, 0, 1, 1, 1, 1]
    assert link[:, 1].tolist() == [1, 1, 1, 0, 1, 1, 0, 1, 1, 1, 1, 1]
    assert link[:, 2].tolist() == [1, 1, 1, 1, 1, 0, 0, 1, 1, 1, 1, 1]
    same = lambda t, e: np.array_equal(nxt[t, e], obs[t + 1, e])  # noqa: E731
    assert not nd[0, 0] and not same(0, 0)      # done
    assert nd[2, 0] and not same(2, 0)          # truncated: only the bytes tell
    assert not nd[5, 0] and same(5, 0)          # only not_done tells
    assert nd[11].all() and link[11].all()      # still open
    for t in range(STEPS - 1):  # the links are the rule, nothing else
        for e in range(3):
            assert link[t, e] == (nd[t, e] and same(t, e))
    assert not any(np.array_equal(nxt[t, e], obs[t + 1, f]) for t in range(STEPS - 1) for e in range(3)
                   for f in range(3) if e != f)  # no lane continues another one


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("keys", [(4, np.uint8), (3, np.int32)])
def test_every_feeding_gives_the_oracles_flags_after_every_write(N, keys):
    s = script(N, *keys)
    link, cap = s[3], RING * N
    # vector step by vector step
    steps, seen = _Chain(cap, N), []
    for t in range(STEPS):
        prev = feed(steps, s, t, t + 1)
        assert prev == (None if t == 0 else (t - 1) * N % cap)
        assert not steps.flags[t * N % cap:t * N % cap + N].any()
        assert np.array_equal(steps.flags, oracle(link, N, t)), t
        seen.append(steps.flags.copy())
    assert steps.flags.dtype == np.uint8 and steps.flags.shape == (cap,)
    if N == 1:  # row by row: the same thing for one lane, spelled with single rows
        rows = _Chain(cap, 1)
        for t in range(STEPS):
            rows.write(t % cap, s[0][t], s[1][t], s[2][t, 0])  # (one bool for the one row)
            assert np.array_equal(rows.flags, seen[t]), t
    # in bulk: cuts inside an episode (1|2 and 8|9 for lane 0), at an episode end (2|3), a batch across the ring's end
    bulk = _Chain(cap, N)
    for lo, hi in ((0, 2), (2, 3), (3, 9), (9, 12)):
        prev = feed(bulk, s, lo, hi)
        assert prev == (None if lo == 0 else (lo - 1) * N % cap)
        assert np.array_equal(bulk.flags, oracle(link, N, hi - 1)) and np.array_equal(bulk.flags, seen[hi - 1]), (lo, hi)
    # one batch longer than the ring, alone and behind one step (it overwrites that step's rows: nothing to re-evaluate)
    for first in (0, 1):
        once = _Chain(cap, N)
        if first:
            feed(once, s, 0, 1)
        assert feed(once, s, first, STEPS) is None
        assert np.array_equal(once.flags, oracle(link, N, STEPS - 1)) and np.array_equal(once.flags, seen[-1])
    # exactly the ring's length behind one step: the batch's last step lands on that step's rows
    exact = _Chain(cap, N)
    feed(exact, s, 0, 1)
    assert feed(exact, s, 1, 1 + RING) is None and np.array_equal(exact.flags, seen[RING])
    # ... and every feeding leaves the same last write behind: the stream goes on alike
    for chain in (bulk, once, steps):
        last = (STEPS - 1) * N % cap
        assert chain.row == last
        assert chain.write(STEPS * N % cap, s[1][-1], s[1][-1], s[2][-1]) == last
        assert chain.flags[last:last + N].tolist() == [1] * N  # (every lane's last episode is open)


@pytest.mark.parametrize("N", [1, 3])
def test_a_write_that_does_not_follow_the_previous_one_re_evaluates_nothing(N):
    """Step 2 continues step 1 by its keys in every lane, but is written two steps further on (a moved write head):
    write() names no previous step and step 1's flags stay 0; written where it belongs, they are the links."""
    s = script(N)
    assert s[3][1].all()
    moved, inplace = _Chain(RING * N, N), _Chain(RING * N, N)
    for chain, at in ((moved, 3), (inplace, 2)):
        feed(chain, s, 1, 2)
        prev = chain.write(at * N, s[0][2], s[1][2], s[2][2])
        assert prev == (None if chain is moved else N)
    assert not moved.flags.any() and moved.row == 3 * N
    assert inplace.flags[N:2 * N].all() and inplace.flags.sum() == N
    # the same step written twice in place does not continue itself
    again = _Chain(RING * N, N)
    for _ in range(2):
        assert again.write(0, s[1][0], s[1][0], np.ones(N, dtype=bool)) is None
    assert not again.flags.any()
    # a ring of ONE vector step: the previous step is the row being written
    tiny = _Chain(N, N)
    for t in range(3):
        assert tiny.write(0, s[0][t], s[1][t], s[2][t]) is None and not tiny.flags.any()
