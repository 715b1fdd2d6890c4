"""The launch schedule of every sampling route of ``ReplayBuffer``, without a GPU, against a recorded table.

``sample_cpc_refs``, ``sample_cpc`` and ``graph_block`` + ``graph_write`` + ``graph_refs`` are run on CPU buffers under
the launch-trace hook (nothing is computed) over storage x augmentation x n_step x staging, and every launch is compared,
argument for argument, with a recorded table.  The table is two files, each written once and never regenerated:
``tests/sample_route_launches.json`` (``OLD_AUGS``) from the commit BEFORE the three routes were folded into one assembly
function, so an equal trace says that the fold launches what the three hand-written copies launched; and
``tests/sample_route_launches_aug.json`` (``NEW_AUGS``: cutout, translate, RandomConv, which came later) by ``record()``
(``python -m tests.test_sample_routes_host``) from the commit BEFORE the augmentation classes began to describe their own
sampling path to the buffer, so an equal trace says that the protocol launches what the buffer's class tests launched.

A pointer argument is recorded as (ordinal of its allocation by first appearance, byte offset inside it): ``a3+128``.
The allocations are whatever tensors the buffer holds, found by walking its attributes through lists, tuples and dicts
(graph slots included) -- no attribute name enters the normal form.  A pointer inside none of them is a tensor made
during the call: ``t0``, ``t1``, ...  The stand-ins for the pinned slots' device addresses are ``s<k>``.  Behind a
call's launches come its handles, one ``handle:<name>`` entry each (obs, next_obs, pos, pair) with the source, index
and offset pointers in the same normal form: the ring handles launch nothing, so this is what pins their rows and
offsets.

The one difference the fold was allowed: on the copy route (``_h_index_dev = None``) with ``n_step = 1`` the launch
``curla_gather_transition_scalars`` moved from the end of sampling to directly behind the block copy, i.e. to the front
of the call's launches (the copy is no launch); there the first table's entry is compared after that move (the second
table was recorded behind the fold: the move leaves its entries as they are).
"""
import contextlib
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import curla_amd
from curla_amd import _lib, ops
from curla_amd.utils import ReplayBuffer

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sample_route_launches.json")
TABLE_AUG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sample_route_launches_aug.json")
B = 4
# c6: capacity * C * H * W is a multiple of 4 (both rings in one allocation); c3: 7 * 429 bytes is not (two allocations)
GEOMS = {"c6": ((6, 12, 16), 16), "c3": ((3, 11, 13), 7)}
OLD_AUGS = ("identity", "crop", "shift", "jiggle", "jiggle_staged", "cover", "cover_staged")  # TABLE
NEW_AUGS = ("cutout", "cutout_color", "translate", "conv", "conv_staged")  # TABLE_AUG
AUGS = OLD_AUGS + NEW_AUGS
SLOT0, GRAPH_SLOT = 1 << 60, 100  # stand-in device addresses of the pinned slots: SLOT0 + 4096 k
GATHER = "curla_gather_transition_scalars"


class FakeDeviceGenerator:
    """Stands in for the HIP device's torch generator (tests/test_graph_aug_host.py)."""

    def __init__(self):
        self.seed, self.offset = 0xDEADBEEF12345, 40

    def get_offset(self):
        return self.offset

    def set_offset(self, v):
        self.offset = int(v)

    def initial_seed(self):
        return self.seed


@contextlib.contextmanager
def _device_generator():
    gen, real = FakeDeviceGenerator(), ReplayBuffer._noise_generator
    ReplayBuffer._noise_generator = lambda self: gen
    try:
        yield gen
    finally:
        ReplayBuffer._noise_generator = real


def _augmentor(name, hw):
    h, w = hw
    if name == "identity":
        return curla_amd.IdentityAugmentation(hw)
    if name == "crop":
        return curla_amd.RandomCrop(hw, (h - 2, w - 4))
    if name == "shift":
        return curla_amd.RandomShift(hw, pad=2)
    if name.startswith("cutout"):
        return curla_amd.RandomCutout(hw, 2, 5, color=name == "cutout_color")
    if name == "translate":
        return curla_amd.RandomTranslate(hw, (h + 3, w + 4))  # an odd and an even margin
    if name.startswith("conv"):
        return curla_amd.RandomConv(hw, 0.5)  # p < 1: both generator calls of draw_weights
    return (curla_amd.ColorJiggle if name.startswith("jiggle") else curla_amd.NoisyCover)(hw)


def _buffer(geom, dedup, aug, n_step, in_place):
    (c, h, w), cap = GEOMS[geom]
    rb = ReplayBuffer((c, h, w), (2,), cap, B, "cpu", _augmentor(aug, (h, w)), dedup_frames=dedup,
                      staged_aug=aug.endswith("_staged"), n_step=n_step, discount=0.99 if n_step > 1 else None)
    k, n = c // 3, 6
    rgb = np.random.RandomState(3).randint(0, 256, (n + k, 3, h, w), dtype=np.uint8)
    for t in range(n):  # a frame-stacked episode that ends at t = 3
        rb.add(rgb[t:t + k].reshape(c, h, w), [0.1, -0.2], 0.5, rgb[t + 1:t + 1 + k].reshape(c, h, w), t == 3)
    # a CPU buffer has no pinned slots; stand-ins for their device addresses select the route of a device buffer
    rb._h_index_dev = [SLOT0 + 4096 * j for j in range(rb._n_slots)] if in_place else None
    return rb


def _graphable(rb):
    """graph_supported() but for the device type: what it would say of this buffer on the HIP device."""
    if rb._h_index_dev is None:
        return False
    if isinstance(rb.augmentor, (curla_amd.ColorJiggle, curla_amd.NoisyCover, curla_amd.RandomConv)):
        return rb.staged_aug
    return rb.dedup_frames or rb._both is not None


def _allocations(obj, out):
    if torch.is_tensor(obj):
        s = obj.untyped_storage()
        if s.nbytes():
            out.add((s.data_ptr(), s.nbytes()))
    elif isinstance(obj, dict):
        for v in obj.values():
            _allocations(v, out)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            _allocations(v, out)
    return out


def _renumber(calls):
    """Allocation and temporary ordinals by first appearance (again, after launches have been moved)."""
    seen = {"a": {}, "t": {}}

    def tok(v):
        if isinstance(v, str) and v[0] in "at":
            n, plus, off = v[1:].partition("+")
            return v[0] + str(seen[v[0]].setdefault(n, len(seen[v[0]]))) + plus + off
        return v
    return [[[tok(v) for v in launch] for launch in call] for call in calls]


def _normalise(calls, rb):
    allocs = sorted(_allocations(vars(rb), set()))

    def tok(v):
        if isinstance(v, bool) or not isinstance(v, int):
            return v
        if v >= SLOT0 and (v - SLOT0) % 4096 == 0 and (v - SLOT0) // 4096 <= GRAPH_SLOT:
            return "s%d" % ((v - SLOT0) // 4096)
        for base, size in allocs:
            if base <= v < base + size:
                return "a%d+%d" % (base, v - base)
        return "t%d" % v if v >= 2 ** 32 else v
    return _renumber([[[name] + [tok(v) for v in args] for name, args in call] for call in calls])


@contextlib.contextmanager
def _tracing(calls, keep):
    """Launches go to ``calls``; every tensor whose pointer is taken stays alive in ``keep``, so that no two tensors
    made during the call share an address."""
    real = ops.ptr

    def ptr(t):
        keep.append(t)
        return real(t)
    ops.ptr = ptr
    _lib.set_trace_hook(lambda name, args: calls.append((name, args)))
    try:
        yield
    finally:
        _lib.set_trace_hook(None)
        ops.ptr = real


def _digests(gen):
    s = np.random.get_state()
    return [hashlib.sha1(s[1].tobytes() + repr(s[2:]).encode()).hexdigest()[:16],
            hashlib.sha1(torch.get_rng_state().numpy().tobytes()).hexdigest()[:16], gen.offset]


def _handle_facts(rb, obs, nxt, pos, graph):
    """What the table keeps of the handles; what must hold of them whatever the table says is asserted here."""
    facts = []
    for ref in (obs, nxt, pos):
        assert isinstance(ref, ops.ObsRef) and ref.B == B
        if graph or ref.is_u8 != 1:
            assert ref.guard is None
        else:  # the slot's generation triple: valid now, the slot being the one just drawn
            gens, s, gen = ref.guard
            assert s == rb._sample_slot and len(gens) == rb.N_SAMPLE_SLOTS and gens[s] == gen
            assert ref.check() is ref
        facts.append([ref.is_u8, ref.B, ref.guard is not None])
    assert nxt.pair is None and pos.pair is None
    if obs.pair is not None:
        assert obs.pair[1] is nxt and obs.pair[0].B == 2 * B and obs.pair[0].is_u8 == obs.is_u8
        assert (obs.pair[0].guard is None) == (obs.guard is None)
    facts.append(obs.pair is not None)
    return facts


def _handle_entries(obs, nxt, pos):
    """Where every handle points, as entries behind the call's launches (normalised with them): source, index and
    offset pointers, minibatch size and window -- for the ring handles, which launch nothing, the only trace."""
    refs = [("obs", obs), ("next_obs", nxt), ("pos", pos)] + ([("pair", obs.pair[0])] if obs.pair is not None else [])
    return [("handle:" + name, (ops.ptr(r.src), ops.ptr(r.idx), ops.ptr(r.h1), ops.ptr(r.w1), r.B, r.C, r.Hs, r.Ws,
                                r.Hc, r.Wc)) for name, r in refs]


def run_route(geom, dedup, aug, n_step, in_place, route):
    """One route on a fresh buffer: {"launches": one list per call, "handles": ..., "rng": ...}, or None where the
    route does not exist (a graph slot on a buffer that graph_supported() refuses)."""
    with _device_generator() as gen:
        rb = _buffer(geom, dedup, aug, n_step, in_place)
        if route == "graph" and not _graphable(rb):
            return None
        np.random.seed(7)
        torch.manual_seed(7)
        calls, keep, handles = [], [], []
        for _ in range(2 if route == "refs" else 1):
            calls.append([])
            with _tracing(calls[-1], keep):
                if route == "refs":
                    obs, act, rew, nxt, nd, kw = rb.sample_cpc_refs()
                    handles.append(_handle_facts(rb, obs, nxt, kw["obs_pos"], False))
                    calls[-1].extend(_handle_entries(obs, nxt, kw["obs_pos"]))
                elif route == "cpc":
                    obs, act, rew, nxt, nd, kw = rb.sample_cpc()
                    handles.append([list(t.shape) for t in (obs, nxt, kw["obs_pos"])])
                else:
                    g = rb.graph_block(0)
                    g["host_dev"] = SLOT0 + 4096 * GRAPH_SLOT
                    idxs, offs = rb.draw_indices()
                    rb.graph_write(0, idxs, offs, bytes(range(80)), rb.draw_aug())
                    obs, act, rew, nxt, nd, kw = rb.graph_refs(0)
                    handles.append(_handle_facts(rb, obs, nxt, kw["obs_pos"], True))
                    calls[-1].extend(_handle_entries(obs, nxt, kw["obs_pos"]))
                assert kw["obs_anchor"] is obs and kw["time_anchor"] is None and kw["time_pos"] is None
                assert tuple(act.shape) == (B, 2) and tuple(rew.shape) == tuple(nd.shape) == (B, 1)
        return dict(launches=_normalise(calls, rb), handles=handles, rng=_digests(gen))


CONFIGS = [(geom, dedup, aug, n_step, in_place) for geom in GEOMS for dedup in (False, True) for aug in AUGS
           for n_step in (1, 3) for in_place in (True, False)]
ROUTES = ("refs", "cpc", "graph")


def _key(geom, dedup, aug, n_step, in_place, route):
    return "/".join((geom, "store" if dedup else "rings", aug, "n%d" % n_step, "inplace" if in_place else "copy", route))


def record():
    """Write the NEW_AUGS table -- from the commit whose launches are the yardstick.  (TABLE is never written again.)"""
    table = {_key(*cfg, route): run_route(*cfg, route) for cfg in CONFIGS if cfg[2] in NEW_AUGS for route in ROUTES}
    with open(TABLE_AUG, "w") as f:
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":")))
                                   for k, v in table.items()) + "\n}\n")
    return table


@pytest.fixture(scope="module")
def table():
    with open(TABLE) as f, open(TABLE_AUG) as f_aug:
        old, new = json.load(f), json.load(f_aug)
    assert {k.split("/")[2] for k in old} == set(OLD_AUGS) and {k.split("/")[2] for k in new} == set(NEW_AUGS)
    return {**old, **new}


def test_the_table_covers_the_matrix(table):
    assert sorted(table) == sorted(_key(*cfg, route) for cfg in CONFIGS for route in ROUTES)  # both files, exactly
    assert len(table) == 576
    assert {_key(*cfg, "x").split("/")[1] for cfg in CONFIGS} == {"rings", "store"}
    rings = {g: _buffer(g, False, "identity", 1, True)._both is not None for g in GEOMS}
    assert rings == {"c6": True, "c3": False}  # one allocation, two allocations
    with _device_generator():
        for cfg in CONFIGS:
            assert (table[_key(*cfg, "graph")] is not None) == _graphable(_buffer(*cfg))
            assert table[_key(*cfg, "refs")] is not None and table[_key(*cfg, "cpc")] is not None


def _gather_behind_the_block_copy(calls):
    out = []
    for call in calls:
        (at,) = [i for i, launch in enumerate(call) if launch[0] == GATHER]
        out.append([call[at]] + call[:at] + call[at + 1:])
    return _renumber(out)


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda cfg: _key(*cfg, "")[:-1])
def test_every_route_launches_what_the_table_says(table, cfg):
    geom, dedup, aug, n_step, in_place = cfg
    for route in ROUTES:
        want, got = table[_key(*cfg, route)], run_route(*cfg, route)
        if want is None:
            assert got is None, route
            continue
        # (through JSON: tuples and lists, ints and floats compare as the table stores them)
        got = json.loads(json.dumps(got))
        launches = want["launches"]
        if not in_place and n_step == 1:
            launches = _gather_behind_the_block_copy(launches)
        assert len(got["launches"]) == len(launches) == (2 if route == "refs" else 1)
        for call_got, call_want in zip(got["launches"], launches):
            assert [l[0] for l in call_got] == [l[0] for l in call_want], route
            for l_got, l_want in zip(call_got, call_want):
                assert l_got == l_want, (route, l_got, l_want)
        assert got["handles"] == want["handles"], route
        assert got["rng"] == want["rng"], route


if __name__ == "__main__":
    print("%d entries -> %s" % (len(record()), TABLE_AUG))
