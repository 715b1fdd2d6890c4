"""The strip planner of the stride-1 convolutions (csrc/conv_plan.h), on the CPU: the header is host-only code, so a small
program (tests/capi/conv_plan_probe.cpp, built with the address and undefined-behaviour sanitizers, its own process)
prints the plan of every form at every extent 1 <= Ho <= 40, 1 <= Wo <= 140.  Two things are checked on those lines:
the planner's invariants, and that the geometry lists of the GPU sweep (tests/test_gpu_conv_s1_edges.py) contain every
regime of the plan that occurs anywhere in that range -- per operation and per form, because one list runs under every
form of its operation."""
import os
import subprocess

import pytest

from tests.test_gpu_conv_s1_edges import (BWD_GEOMS, DGRAD_GEOMS, FWD2_GEOMS, FWD_GEOMS, STACK_GEOMS, TINY, WGRAD_GEOMS,
                                          batch_of)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "curla_amd", "csrc")
PROBE = os.path.join(ROOT, "tests", "capi", "conv_plan_probe.cpp")
HMAX, WMAX = 40, 140
MAX_GEOMS = 40

# form -> (column units of a row of Wo pixels, lane groups per strip, rows of Ho image rows), as the plan functions of
# conv_plan.h define them
FORMS = {
    "s1": (lambda Wo: (Wo + 1) // 2, 16, lambda Ho: Ho),            # rw::plan / rwb::plan: pixel pairs
    "f43": (lambda Wo: (Wo + 3) // 4, 16, lambda Ho: Ho),           # rw43::plan: pixel quads
    "wgrad_x": (lambda Wo: (Wo + 1) // 2, 4, lambda Ho: Ho),        # rw::plan4
    "wgrad_xy": (lambda Wo: (Wo + 1) // 2, 4, lambda Ho: (Ho + 1) // 2),  # rw::plan4p: rows are row pairs
}
# operation -> (its geometry list, the forms it runs under, the smallest planned extent, the fixed small shapes).  The
# data gradient plans its OUTPUT, two larger than the gradient it reads: the entry point's 1 x 1, 1 x N, N x 1 and 2 x 2
# are planned extents 3 x 3, 3 x N, N x 3 and 4 x 4.
OPERATIONS = {
    "forward": (FWD_GEOMS, ("s1", "f43"), 1),
    "data gradient": (DGRAD_GEOMS, ("s1", "f43"), 3),
    "weight gradient": (WGRAD_GEOMS, ("wgrad_x", "wgrad_xy"), 1),
}


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """{(form, Ho, Wo): (nfull, brem, nr, nseg, ntr, steps)} over the whole range, from one run of the probe"""
    exe = str(tmp_path_factory.mktemp("conv_plan") / "conv_plan_probe")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", CSRC, PROBE, "-o", exe])
    keys = [(f, Ho, Wo) for f in FORMS for Ho in range(1, HMAX + 1) for Wo in range(1, WMAX + 1)]
    r = subprocess.run([exe], input="".join(f"{f} {Ho} {Wo}\n" for f, Ho, Wo in keys), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(keys)
    return {k: tuple(int(v) for v in ln.split()) for k, ln in zip(keys, lines)}


def test_plan_header_is_host_only_code():
    """conv_plan.h through the probe, which includes nothing else of the library: plain C++17, no warnings, nothing from
    ROCm on the include path, no device builtin; and the conv headers take their plans from it."""
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", CSRC, PROBE], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr
    with open(os.path.join(CSRC, "conv_plan.h")) as f:
        code = "\n".join(ln.split("//")[0] for ln in f.read().splitlines())
    for word in ("hip", "__builtin", "__device__", "__global__", "#include"):
        assert word not in code, word
    for name in ("Geom", "plan_units", "plan", "plan4", "plan4p"):
        assert f" {name}(" in code or f"struct {name} " in code, name
    for header in ("conv_rw.h", "conv_rw43.h", "conv_rwb.h", "conv_rw_wgrad.h", "conv_rw_wgrad2.h"):
        with open(os.path.join(CSRC, header)) as f:
            text = "\n".join(ln.split("//")[0] for ln in f.read().splitlines())
        assert "plan_units(" not in text and "struct Geom" not in text, header
    with open(os.path.join(CSRC, "conv_rw.h")) as f:
        assert '#include "conv_plan.h"' in f.read()


def test_planner_invariants(plans):
    bad = []
    for (form, Ho, Wo), (nfull, brem, nr, nseg, ntr, steps) in plans.items():
        units, per, rows_of = FORMS[form]
        cols, rows = units(Wo), rows_of(Ho)
        ok = nfull * per + brem == cols and 0 <= brem < per and steps == nfull * rows + ntr * nr
        if brem == 0:
            ok = ok and nr == nseg == ntr == 0
        else:
            ok = ok and 1 <= nr <= rows and (nseg - 1) * nr < rows <= nseg * nr
            ok = ok and (ntr - 1) * per < brem * nseg <= ntr * per
        if not ok:
            bad.append(((form, Ho, Wo), (nfull, brem, nr, nseg, ntr, steps)))
    assert not bad, bad[:10]
    # the worked example of the header comment: one full strip, two remainder columns, seven segments of five rows
    assert plans[("s1", 35, 35)] == (1, 2, 5, 7, 1, 40)


def regimes(form, Ho, Wo, plan):
    """the regime attributes of one plan: {(attribute, value)}"""
    nfull, brem, nr, nseg, ntr, _ = plan
    _, per, rows_of = FORMS[form]
    rows = rows_of(Ho)
    a = {("min(nfull, 2)", min(nfull, 2)), ("Ho mod 2", Ho % 2), ("Wo mod 2", Wo % 2),
         ("brem", "0" if brem == 0 else "1" if brem == 1 else "per - 1" if brem == per - 1 else "in between")}
    if form == "f43":
        a.add(("Wo mod 4", Wo % 4))
    if brem:
        if rows == 1:
            seg = "nr == 1 == Ho"
        elif nr == 1:
            seg = "nr == 1"
        elif nr == rows:
            seg = "nr == Ho"
        else:
            seg = "1 < nr < Ho, Ho % nr == 0" if rows % nr == 0 else "1 < nr < Ho, short last segment"
        a |= {("segments", seg), ("min(ntr, 2)", min(ntr, 2)),
              ("last remainder strip", "full" if (brem * nseg) % per == 0 else "partly filled")}
        if ntr >= 2:
            a.add(("nfull with ntr >= 2", "nfull == 0" if nfull == 0 else "nfull >= 1"))
    return a


@pytest.mark.parametrize("operation", list(OPERATIONS))
def test_sweep_covers_every_regime(plans, operation):
    geoms, forms, lo = OPERATIONS[operation]
    assert len(geoms) == len(set(geoms)) <= MAX_GEOMS
    assert all(lo <= Ho <= HMAX and lo <= Wo <= WMAX for Ho, Wo in geoms), geoms
    # the fixed small shapes: 1 x 1, 1 x N, N x 1, 2 x 2 (the data gradient: of the gradient it reads)
    assert (lo, lo) in geoms and (lo + 1, lo + 1) in geoms
    assert any(Ho == lo and Wo > lo for Ho, Wo in geoms) and any(Wo == lo and Ho > lo for Ho, Wo in geoms)
    for form in forms:
        everywhere = {}
        for Ho in range(lo, HMAX + 1):
            for Wo in range(lo, WMAX + 1):
                for a in regimes(form, Ho, Wo, plans[(form, Ho, Wo)]):
                    everywhere.setdefault(a, (Ho, Wo))
        listed = set()
        for Ho, Wo in geoms:
            listed |= regimes(form, Ho, Wo, plans[(form, Ho, Wo)])
        missing = {a: hw for a, hw in everywhere.items() if a not in listed}
        assert not missing, f"{operation} [{form}]: regimes no listed geometry has (and one that does): {missing}"
        # (both combinations exist in the range, so the line above already demands them; stated for the reader)
        assert {("nfull with ntr >= 2", "nfull == 0"), ("nfull with ntr >= 2", "nfull >= 1")} <= listed
        assert {("Ho mod 2", 0), ("Ho mod 2", 1), ("Wo mod 2", 0), ("Wo mod 2", 1)} <= listed


def test_derived_case_lists_stay_inside_the_sweeps():
    """the cases that name sweep geometries name real ones, and the one-launch backward's data gradients are the data
    gradient sweep's (same extents, same batch): held to float64 there"""
    assert set(FWD2_GEOMS) <= set(FWD_GEOMS) and len(FWD2_GEOMS) == 3
    assert set(STACK_GEOMS) <= set(FWD_GEOMS) and len(STACK_GEOMS) <= 8
    assert all(Ho + 2 >= 7 and Wo + 2 >= 7 and (Ho + 2) * (Wo + 2) <= 1000 for Ho, Wo in STACK_GEOMS)
    assert len(BWD_GEOMS) == 4
    for Ho, Wo in BWD_GEOMS:
        assert (Ho, Wo) in WGRAD_GEOMS and (Ho + 2, Wo + 2) in DGRAD_GEOMS
        assert batch_of(Ho, Wo) == batch_of(Ho + 2, Wo + 2)
    assert TINY in FWD_GEOMS and TINY in WGRAD_GEOMS and (TINY[0] + 2, TINY[1] + 2) in DGRAD_GEOMS
    assert all(batch_of(Ho, Wo) in (2, 3) for Ho in range(1, HMAX + 1) for Wo in range(1, WMAX + 1))
    # the largest tensor of the sweeps: 3 x 40 x 140 x 32 floats
    assert max((Ho + 2) * (Wo + 2) for Ho, Wo in FWD_GEOMS + WGRAD_GEOMS) <= 40 * 140
    assert max(Ho * Wo for Ho, Wo in DGRAD_GEOMS) <= 40 * 140
