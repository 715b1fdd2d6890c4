"""Same launches, in the same order, with the same arguments: the library calls of every write route of the replay
buffer -- ``add``, ``add_vec``, ``add_batch``, ``load`` -- and of one ``sample_cpc_refs(indices=...)`` on CPU buffers
under the launch-trace hook (which computes nothing), against lists recorded before the write side was given one
continuity rule (``python -m tests.test_replay_write_launches_host`` prints them).  Addresses are named by the buffer
attribute they fall into and their offset inside it, so two runs give the same list."""
import numpy as np
import pytest

import curla_amd
from curla_amd.utils import ReplayBuffer
from tests.test_add_vec_host import streams
from tests.test_nstep_host import _relative, _traced

C, HW, A, B = 9, (20, 20), 2, 4
CASES = {
    "nstep_pos": dict(n_step=3, pos_offset=2),
    "per": dict(prioritized=True),
    "vec": dict(n_step=3, pos_offset=2, n_envs=3),
    "all": dict(n_step=3, pos_offset=2, prioritized=True, n_envs=3),
    "store": dict(n_step=3, pos_offset=2, dedup_frames=True),
}


def _buffer(capacity, **kw):
    if kw.get("n_step", 1) > 1:
        kw.setdefault("discount", 0.99)
    return ReplayBuffer((C,) + HW, (A,), capacity, B, "cpu", curla_amd.RandomCrop(HW, (16, 16)), **kw)


def _names(rb, trace):
    """(entry point, arguments): every scalar as it is, every address as (attribute, offset) -- lists, as JSON has them."""
    return [[name, [list(a) if isinstance(a, tuple) else a for a in args]] for name, args in _relative(rb, trace)]


def record(case, tmp_path):
    """The write routes in turn on a ring of 7 vector steps (every route crosses the ring's end once), then the files of
    a ring that holds all 12 steps into a fresh buffer, then one sample."""
    kw = CASES[case]
    N = kw.get("n_envs", 1)
    lanes, vec = streams()
    if N == 1:
        vec = tuple(a[:, 0] for a in vec)
    flat = tuple(a.reshape((12 * N,) + a.shape[1 + (N > 1):]) for a in vec)
    rb = _buffer(7 * N, **kw)
    out = {}
    step = lambda t: tuple(a[t] for a in vec)  # noqa: E731
    if N == 1:
        out["add"] = _names(rb, _traced(lambda: [rb.add(*step(t)) for t in (0, 1)]))
    else:
        with pytest.raises(ValueError, match="add_vec"):
            rb.add(*(a[0] for a in flat))
        _traced(lambda: [rb.add_vec(*step(t)) for t in (0, 1)])
    vstep = step if N > 1 else lambda t: tuple(a[t][None] for a in vec)  # a vector step of one lane
    out["add_vec"] = _names(rb, _traced(lambda: [rb.add_vec(*vstep(t)) for t in (2, 3)]))
    out["add_batch"] = _names(rb, _traced(lambda: rb.add_batch(*(a[4 * N:9 * N] for a in flat))))  # rows 4, 5, 6, 0, 1
    assert rb.idx == 2 * N and rb.full
    # load: two chunks, the cut inside an episode, written by a plain ring (a frame store saves through a kernel)
    saver = _buffer(16 * N, **{k: v for k, v in kw.items() if k in ("n_envs",)})
    for lo, hi in ((0, 5), (5, 12)):
        saver.add_batch(*(a[lo * N:hi * N] for a in flat))
        saver.save(str(tmp_path))
    fresh = _buffer(16 * N, **kw)
    out["load"] = _names(fresh, _traced(lambda: fresh.load(str(tmp_path))))
    assert fresh.idx == 12 * N
    idx = (np.array([0, 5, 11, 3]) if not kw.get("prioritized") else np.array([0.1, 0.3, 0.6, 0.9]),
           np.zeros((6, B), dtype=np.int32))
    out["sample"] = _names(fresh, _traced(lambda: fresh.sample_cpc_refs(indices=idx)))
    if not kw.get("prioritized"):  # the route of a device buffer: the staging launch reads the pinned block in place
        fresh._h_index_dev = [4096 * (k + 1) for k in range(fresh._n_slots)]
        out["sample_staged"] = _names(fresh, _traced(lambda: fresh.sample_cpc_refs(indices=idx)))
    return out


# recorded on the commit before the change (curla_amd/utils.py held the whole buffer)
EXPECTED = {'all': {'add_batch': [['curla_per_set',
                        [['_per_s', 0], ['_per_sums', 0], ['_per_max', 0], 21, None, 12, None, 15, 0]]],
         'add_vec': [['curla_add_vec',
                      [['_d_add', 0], ['_ring_store', 0], ['_ring_store', 75600], ['_sc', 0], ['_cont', 0], 21, 6, 1,
                       3, 9, 20, 20, 2, 0]],
                     ['curla_per_set', [['_per_s', 0], ['_per_sums', 0], ['_per_max', 0], 21, None, 6, None, 3, 0]],
                     ['curla_add_vec',
                      [['_d_add', 0], ['_ring_store', 0], ['_ring_store', 75600], ['_sc', 0], ['_cont', 0], 21, 9, 1,
                       3, 9, 20, 20, 2, 0]],
                     ['curla_per_set', [['_per_s', 0], ['_per_sums', 0], ['_per_max', 0], 21, None, 9, None, 3, 0]]],
         'load': [['curla_per_set', [['_per_s', 0], ['_per_sums', 0], ['_per_max', 0], 48, None, 0, None, 15, 0]],
                  ['curla_per_set', [['_per_s', 0], ['_per_sums', 0], ['_per_max', 0], 48, None, 15, None, 21, 0]]],
         'sample': [['curla_per_sample', [['_per_s', 0], ['_per_sums', 0], 48, ['_d_index', 0], 256, 288, 4, 0]],
                    ['curla_gather_transition_scalars',
                     [['_sc', 0], ['_d_index', 0], 4, 2, ['_d_scal', 0], ['_d_scal', 32], ['_d_scal', 48], 0]],
                    ['curla_nstep_compose_strided',
                     [['_d_index', 0], 160, ['_sc', 0], ['_cont', 0], 48, 3, 3, 0.99, 4, 2, ['_d_scal', 0],
                      ['_d_scal', 32], ['_d_scal', 48], 0]],
                    ['curla_pos_walk_strided', [['_d_index', 0], 192, -1, 160, ['_cont', 0], 48, 3, 2, 3, 4, 0]]]},
 'nstep_pos': {'add': [],
               'add_batch': [],
               'add_vec': [],
               'load': [],
               'sample': [['curla_gather_transition_scalars',
                           [['_sc', 0], ['_d_index', 0], 4, 2, ['_d_scal', 0], ['_d_scal', 32], ['_d_scal', 48], 0]],
                          ['curla_nstep_compose',
                           [['_d_index', 0], 160, ['_sc', 0], ['_cont', 0], 16, 3, 0.99, 4, 2, ['_d_scal', 0],
                            ['_d_scal', 32], ['_d_scal', 48], 0]],
                          ['curla_pos_walk', [['_d_index', 0], 192, -1, 160, ['_cont', 0], 16, 2, 3, 4, 0]]],
               'sample_staged': [['curla_sample_stage_pos',
                                  [8192, ['_d_index', 256], 256, 160, 192, -1, ['_sc', 0], ['_cont', 0], 16, 3, 0.99,
                                   2, 4, 2, ['_d_scal', 64], ['_d_scal', 96], ['_d_scal', 112], 0]]]},
 'per': {'add': [['curla_per_set', [['_per_s', 0], ['_per_sums', 0], ['_per_max', 0], 7, None, 0, None, 1, 0]],
                 ['curla_per_set', [['_per_s', 0], ['_per_sums', 0], ['_per_max', 0], 7, None, 1, None, 1, 0]]],
         'add_batch': [['curla_per_set', [['_per_s', 0], ['_per_sums', 0], ['_per_max', 0], 7, None, 4, None, 5, 0]]],
         'add_vec': [['curla_per_set', [['_per_s', 0], ['_per_sums', 0], ['_per_max', 0], 7, None, 2, None, 1, 0]],
                     ['curla_per_set', [['_per_s', 0], ['_per_sums', 0], ['_per_max', 0], 7, None, 3, None, 1, 0]]],
         'load': [['curla_per_set', [['_per_s', 0], ['_per_sums', 0], ['_per_max', 0], 16, None, 0, None, 5, 0]],
                  ['curla_per_set', [['_per_s', 0], ['_per_sums', 0], ['_per_max', 0], 16, None, 5, None, 7, 0]]],
         'sample': [['curla_per_sample', [['_per_s', 0], ['_per_sums', 0], 16, ['_d_index', 0], 160, 192, 4, 0]],
                    ['curla_gather_transition_scalars',
                     [['_sc', 0], ['_d_index', 0], 4, 2, ['_d_scal', 0], ['_d_scal', 32], ['_d_scal', 48], 0]]]},
 'store': {'add': [],
           'add_batch': [],
           'add_vec': [],
           'load': [],
           'sample': [['curla_gather_transition_scalars',
                       [['_sc', 0], ['_d_index', 0], 4, 2, ['_d_scal', 0], ['_d_scal', 32], ['_d_scal', 48], 0]],
                      ['curla_nstep_compose',
                       [['_d_index', 0], 160, ['_sc', 0], ['_cont', 0], 16, 3, 0.99, 4, 2, ['_d_scal', 0],
                        ['_d_scal', 32], ['_d_scal', 48], 0]],
                      ['curla_pos_walk', [['_d_index', 0], 192, -1, 160, ['_cont', 0], 16, 2, 3, 4, 0]],
                      ['curla_gather_stacks',
                       [['_frame_store', 0], ['_fid', 0], 6, ['_d_index', 0], 4, 3, 20, 20, ['_mb_store', 0], 0]],
                      ['curla_gather_stacks',
                       [['_frame_store', 0], ['_fid', 12], 6, ['_d_index', 160], 4, 3, 20, 20, ['_mb_store', 14400],
                        0]],
                      ['curla_gather_stacks',
                       [['_frame_store', 0], ['_fid', 12], 6, ['_d_index', 192], 4, 3, 20, 20, ['_mb_store', 28800],
                        0]]],
           'sample_staged': [['curla_sample_stage_pos',
                              [8192, ['_d_index', 256], 256, 160, 192, -1, ['_sc', 0], ['_cont', 0], 16, 3, 0.99, 2,
                               4, 2, ['_d_scal', 64], ['_d_scal', 96], ['_d_scal', 112], 0]],
                             ['curla_gather_stacks',
                              [['_frame_store', 0], ['_fid', 0], 6, ['_d_index', 256], 4, 3, 20, 20,
                               ['_mb_store', 43232], 0]],
                             ['curla_gather_stacks',
                              [['_frame_store', 0], ['_fid', 12], 6, ['_d_index', 416], 4, 3, 20, 20,
                               ['_mb_store', 57632], 0]],
                             ['curla_gather_stacks',
                              [['_frame_store', 0], ['_fid', 12], 6, ['_d_index', 448], 4, 3, 20, 20,
                               ['_mb_store', 72032], 0]]]},
 'vec': {'add_batch': [],
         'add_vec': [['curla_add_vec',
                      [['_d_add', 0], ['_ring_store', 0], ['_ring_store', 75600], ['_sc', 0], ['_cont', 0], 21, 6, 1,
                       3, 9, 20, 20, 2, 0]],
                     ['curla_add_vec',
                      [['_d_add', 0], ['_ring_store', 0], ['_ring_store', 75600], ['_sc', 0], ['_cont', 0], 21, 9, 1,
                       3, 9, 20, 20, 2, 0]]],
         'load': [],
         'sample': [['curla_gather_transition_scalars',
                     [['_sc', 0], ['_d_index', 0], 4, 2, ['_d_scal', 0], ['_d_scal', 32], ['_d_scal', 48], 0]],
                    ['curla_nstep_compose_strided',
                     [['_d_index', 0], 160, ['_sc', 0], ['_cont', 0], 48, 3, 3, 0.99, 4, 2, ['_d_scal', 0],
                      ['_d_scal', 32], ['_d_scal', 48], 0]],
                    ['curla_pos_walk_strided', [['_d_index', 0], 192, -1, 160, ['_cont', 0], 48, 3, 2, 3, 4, 0]]],
         'sample_staged': [['curla_sample_stage_pos_strided',
                            [8192, ['_d_index', 256], 256, 160, 192, -1, ['_sc', 0], ['_cont', 0], 48, 3, 3, 0.99, 2,
                             4, 2, ['_d_scal', 64], ['_d_scal', 96], ['_d_scal', 112], 0]]]}}


@pytest.mark.parametrize("case", sorted(CASES))
def test_every_write_route_and_a_sample_launch_what_they_launched(case, tmp_path):
    got = record(case, tmp_path)
    assert sorted(got) == sorted(EXPECTED[case])
    for route in got:
        assert got[route] == EXPECTED[case][route], (case, route)


def test_utils_still_hands_out_the_buffer():
    import curla_amd.replay
    import curla_amd.replay_sample
    import curla_amd.utils
    assert curla_amd.utils.ReplayBuffer is curla_amd.replay.ReplayBuffer is curla_amd.ReplayBuffer is ReplayBuffer
    assert curla_amd.utils.PerHandle is curla_amd.replay_sample.PerHandle


if __name__ == "__main__":
    import pathlib
    import pprint
    import tempfile
    table = {}
    for name in sorted(CASES):
        with tempfile.TemporaryDirectory() as d:
            table[name] = record(name, pathlib.Path(d))
    print("EXPECTED = " + pprint.pformat(table, width=118, compact=True))
