"""The staging kernels of a minibatch, driven through their six entry points: the six instantiations of
``sample_stage_kernel<HOST, NSTEP, POS>`` and ``pos_walk_kernel`` (csrc/sample_stage.h) against the NumPy restatements
of the n-step composition (tests/test_gpu_nstep.py) and of the positive's walk (tests/test_gpu_temporal_pos.py), bit
for bit.

The single-writer rule is tested once for all of them: every word of the pinned block is a sentinel of its own (only
the B start rows are real), so afterwards every word a walk owns must hold the walk's value, which no sentinel equals,
and every other word the pinned block's; the device block ends at ``nbytes``, directly in front of a guard.  A
device-source form (gather / compose / walk on a block copied beforehand, in the copy route's order) is held to the
same expectation as the host-source form of its case, so the two agree word for word and scalar for scalar."""
import numpy as np
import pytest
import torch

from tests.test_gpu_nstep import GUARD_BYTE, _guarded, walk_all
from tests.test_gpu_temporal_pos import rows_of

pytestmark = pytest.mark.gpu

CAP, GAMMA = 7, 0.99
#     row  0  1  2  3  4  5  6     chains: 6 -> 0 -> 1 -> 2 -> 3 -> 4 (5 links, across the ring's end); 3 -> 4 (1 link: a
CONT = [1, 1, 1, 1, 0, 0, 1]     # break inside the reach of n = 3 and k = 3); none from 4 and 5
SENTINEL = 0x5A5A000000000000    # | the word's number: no ring row, no capacity + row
WORDS = dict(nr=1, pos=2, run=3)  # a region's length in units of B words: next_row, pos_row, pos_run

KERNELS = {  # what a test calls: block read from the pinned slot, composition (None: both), the positive's walk
    "gather_transition_scalars": (False, False, False),  # <0,0,0>
    "sample_stage": (True, False, False),                # <1,0,0>
    "nstep_compose": (False, True, False),               # <0,1,0>
    "sample_stage_nstep": (True, True, False),           # <1,1,0>
    "pos_walk": (False, None, True),                     # pos_walk_kernel, behind the gather and behind the composition
    "sample_stage_pos": (True, False, True),             # <1,0,1>
    "sample_stage_pos_nstep": (True, True, True),        # <1,1,1>: curla_sample_stage_pos with a next_row region
}
# pad: words between the index words and the first region (the crop offsets' place).  own: the block holds only the
# regions of the kernel under test (the smallest block its entry point accepts where pad is 0); otherwise all of them,
# and those that belong to no walk of the kernel must arrive as the host wrote them.
CASES = {
    "more_words_than_scalars": dict(B=5, A=2, pad=15, n=3, k=3, run=True, own=False, idx=[6, 3, 0, 5, 2]),
    "more_scalars_than_words": dict(B=3, A=9, pad=0, n=2, k=4, run=False, own=True, idx=[6, 3, 4]),
    # 280 scalar threads; the first region starts at word 230 and straddles the workgroup boundary at thread 256
    "two_workgroups": dict(B=70, A=2, pad=90, n=3, k=3, run=True, own=True, idx=[(3 * b + 6) % CAP for b in range(70)]),
    "no_flags": dict(B=5, A=2, pad=15, n=1, k=1, run=True, own=False, idx=[6, 3, 0, 5, 2], cont=None),  # cont = NULL
}
PAIRS = [(kernel, name) for name, case in CASES.items() for kernel, (_, nstep, pos) in KERNELS.items()
         if "cont" not in case or (pos and nstep is not None) or kernel == "pos_walk"]


def _block(case, kernel):
    """The pinned block of ``case`` for ``kernel`` as int64 words, and its layout in words: idx [2B] | pad | the regions."""
    _, nstep, pos = KERNELS[kernel]
    B = case["B"]
    regions = ("nr", "pos") + (("run",) if case["run"] else ())
    if case["own"]:
        regions = tuple(r for r in regions if (r == "nr" and nstep is not False) or (r != "nr" and pos))
    at = (2 * B if regions else B) + case["pad"]  # without a region the B start rows are a whole block
    lay = {}
    for r in regions:
        lay[r], at = at, at + WORDS[r] * B
    lay["nwords"] = at
    host = SENTINEL | np.arange(at, dtype=np.int64)
    host[:B] = case["idx"]
    return host, lay


def _expected(case, lay, host, sc, composed, pos):
    """(block, mask of the words a walk owns, action, reward, not_done) by the restatements."""
    B, A, cont = case["B"], case["A"], case.get("cont", CONT)
    idx = host[:B].copy()
    want, owned = host.copy(), np.zeros(len(host), dtype=bool)
    if composed:
        rew, nd, last = walk_all(sc[:, A], sc[:, A + 1], cont, CAP, case["n"], GAMMA, idx)
        want[B:2 * B], want[lay["nr"]:lay["nr"] + B] = CAP + last, last
        owned[B:2 * B] = owned[lay["nr"]:lay["nr"] + B] = True
    else:
        rew, nd, last = sc[idx, A], sc[idx, A + 1], idx
    if pos:
        r = rows_of(cont, CAP, case["k"], idx)
        want[lay["pos"]:lay["pos"] + 2 * B] = np.concatenate([r, CAP + r])
        owned[lay["pos"]:lay["pos"] + 2 * B] = True
        if "run" in lay:
            want[lay["run"]:lay["run"] + 3 * B] = np.concatenate([idx, CAP + last, CAP + r])
            owned[lay["run"]:lay["run"] + 3 * B] = True
    return want, owned, sc[idx, :A], rew, nd


def _scalars(A):
    return np.random.RandomState(7).randn(CAP, A + 2).astype(np.float32)


def _flavours(kernel, case):
    """With and without the composition in front for pos_walk (the composition needs the flags), else the kernel's own."""
    nstep = KERNELS[kernel][1]
    return (bool(nstep),) if nstep is not None else (False, True) if "cont" not in case else (False,)


def test_the_cases_hold_every_edge():
    runs = []
    for r0 in range(CAP):
        r, L = r0, 0
        while CONT[r]:
            r, L = (r + 1) % CAP, L + 1
        runs.append(L)
    assert runs == [4, 3, 2, 1, 0, 0, 5]  # row 3: a break inside the reach; rows 6 and 0: longer than n = 3 and k = 3
    for name, case in CASES.items():
        B, A, idx = case["B"], case["A"], np.array(case["idx"])
        assert len(idx) == B and CAP - 1 in idx and len(set(idx.tolist())) >= 3  # the wrap; not all rows equal
        for kernel in (k for k, n in PAIRS if n == name):
            host_src, _, pos = KERNELS[kernel]
            host, lay = _block(case, kernel)
            for composed in _flavours(kernel, case):
                want, owned, _, rew, nd = _expected(case, lay, host, _scalars(A), composed, bool(pos))
                assert owned.any() == bool(composed or pos) and (want[owned] != host[owned]).all()
                assert np.array_equal(want[~owned], host[~owned]) and (host[B:] >= SENTINEL).all()
                if "cont" in case:
                    continue  # n = k = 1: every walk stays on its start row
                if composed:
                    last = want[lay["nr"]:lay["nr"] + B]
                    assert (last != idx).any() and (last == idx).any() and (last < idx).any()  # some across the wrap
                    assert (rew != _scalars(A)[idx, A]).any()
                if pos:
                    r = want[lay["pos"]:lay["pos"] + B]
                    assert (r != idx).any() and (r == idx).any() and (r < idx).any()
                    if composed and case["n"] != case["k"]:
                        assert (r != last).any()  # the two walks are independent
            if name == "more_words_than_scalars" and host_src:
                assert lay["nwords"] > B * (A + 2)
            if name == "more_scalars_than_words":
                assert B * (A + 2) > lay["nwords"]
            if name == "two_workgroups":
                assert B * (A + 2) > 256 and (not host_src or not owned.any() or (owned[255] and owned[256]))
    assert {k for k, _ in PAIRS} == set(KERNELS) and CASES["more_scalars_than_words"]["n"] != CASES["more_scalars_than_words"]["k"]
    assert any(c["run"] for c in CASES.values()) and not all(c["run"] for c in CASES.values())


@pytest.mark.parametrize("kernel,name", PAIRS)
def test_kernel_against_the_restatements(kernel, name):
    from curla_amd import ops
    case = CASES[name]
    host_src, _, pos = KERNELS[kernel]
    B, A, k = case["B"], case["A"], case["k"]
    host, lay = _block(case, kernel)
    nbytes = 8 * lay["nwords"]
    sc = _scalars(A)
    sc_d = torch.from_numpy(sc).cuda()
    cont_d = torch.tensor(CONT, dtype=torch.uint8, device="cuda") if "cont" not in case else None

    def off(region):
        return 8 * lay[region] if region in lay else None

    for composed in _flavours(kernel, case):
        (blk, act, rew, nd), guards = _guarded([nbytes, 4 * B * A, 4 * B, 4 * B])
        out = [t.view(torch.float32) for t in (act, rew, nd)]
        n, nr = (case["n"], off("nr")) if composed else (1, None)  # without the composition next_row is nobody's
        if host_src:
            hp = ops.host_device_pointer(torch.from_numpy(host.view(np.uint8).copy()).pin_memory())
            if pos:
                ops.sample_stage_pos(hp, blk, nbytes, nr, off("pos"), off("run"), sc_d, cont_d, CAP, n, GAMMA, k, B, A, *out)
            elif composed:
                ops.sample_stage_nstep(hp, blk, nbytes, nr, sc_d, cont_d, CAP, n, GAMMA, B, A, *out)
            else:
                ops.sample_stage(hp, blk, nbytes, sc_d, B, A, *out)
        else:  # the copy route's launches on a block copied beforehand
            blk.copy_(torch.from_numpy(host.view(np.uint8)))
            if composed:
                ops.nstep_compose(blk, nr, sc_d, cont_d, CAP, n, GAMMA, B, A, *out)
            else:
                ops.gather_transition_scalars(sc_d, blk[:8 * B].view(torch.int64), B, A, *out)
            if pos:
                ops.pos_walk(blk, off("pos"), off("run"), nr, cont_d, CAP, k, n, B)
        torch.cuda.synchronize()
        want, owned, w_act, w_rew, w_nd = _expected(case, lay, host, sc, composed, bool(pos))
        got = blk.cpu().numpy().view(np.int64)
        assert np.array_equal(got[owned], want[owned])    # every word a walk owns holds the walk's value
        assert np.array_equal(got[~owned], host[~owned])  # every other word is the pinned block's
        assert np.array_equal(out[0].cpu().numpy().reshape(B, A), w_act)
        assert np.array_equal(out[1].cpu().numpy(), w_rew) and np.array_equal(out[2].cpu().numpy(), w_nd)
        assert all(bool((g == GUARD_BYTE).all()) and g.numel() >= 256 for g in guards)  # nothing behind nbytes
