"""The plans of the first conv layer (csrc/conv1_plan.h), on the CPU: the header is host-only code, so the probe
(tests/capi/conv_plan_probe.cpp, built with the address and undefined-behaviour sanitizers, its own process) prints every
plan of every crop of the range below.  Checked on those lines: the invariants of the band plans and of the row walks'
strips and shares, and that the geometry lists of the GPU sweep (tests/test_gpu_conv1_edges.py) contain every regime
that occurs anywhere in the range -- per operation, source and form, because one list runs under every form of its
operation.  As in tests/test_conv_plan_host.py a regime is an (attribute, value) pair of one form's plan -- the full
product of the attributes has more cells than 40 geometries can hold -- with the pairs that share code joined: (bands,
last band), (tiles < 8, pixels mod 16)."""
import os
import subprocess

import pytest

from tests.test_gpu_conv1_edges import (F32_FWD_GEOMS, F32_SOURCES, F32_WGRAD_GEOMS, FWD2_GEOMS, NAN_GEOMS, U8_FORMS,
                                        U8_FWD_GEOMS, U8_WGRAD_FORMS, U8_WGRAD_GEOMS, WIDE_GEOM, WRAP_GEOM, batch_of, out_hw,
                                        ring_of, u8_rw_grid, wrap_batch)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "curla_amd", "csrc")
PROBE = os.path.join(ROOT, "tests", "capi", "conv_plan_probe.cpp")
MAX_GEOMS = 40
CHANNELS = (3, 6, 9, 12)
# The range: every crop height up to 40 and every seventh up to 180, every width up to 72 and every fifth up to 320, the
# shapes the project trains on -- and the strip of crops 676..690 wide (C = 12, 3 to 12 rows) where a band's first
# staging pass is exactly its 7 x 512 runs, which no crop up to 320 wide reaches.
HEIGHTS = sorted(set(range(3, 41)) | set(range(40, 181, 7)) | {76, 84, 100, 168})
WIDTHS = sorted(set(range(3, 73)) | set(range(75, 321, 5)) | {76, 84, 135, 168})
RANGE = [(C, Hc, Wc) for C in CHANNELS for Hc in HEIGHTS for Wc in WIDTHS] + \
        [(12, Hc, Wc) for Hc in range(3, 13) for Wc in range(676, 691)]
FIELDS = ("Ho Wo RSb RSf th nbands lds f_auto f_hybrid f_band f_rw f_rwb w_auto w_f32 w_b16 wth wnbands wlds_f32 wlds_b16 "
          "fth flds gth glds s_nhwc_rw s_nhwc_band s_nchw_rw").split()
U8_FORM_NAMES = ("rwb", "rw", "hybrid", "band")  # conv1::Conv1U8Form
U8_BUDGET, F32_FWD_BUDGET, F32_WGRAD_BUDGET, MAX_LDS = 76 * 1024, 76 * 1024, 150 * 1024, 160 * 1024
CU_COUNTS = (256, 304, 8)


def build_probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("conv1_plan") / "conv_plan_probe")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", CSRC, PROBE, "-o", exe])
    return exe


def ask(exe, lines):
    r = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return [tuple(int(v) for v in ln.split()) for ln in out]


def plans_of(exe, geoms):
    """{(C, Hc, Wc): {field: value, "p16": plan_units over Wo on 16 lane groups, "p4": on 4}}"""
    found = {}
    for g, v in zip(geoms, ask(exe, [f"c1 {C} {Hc} {Wc}" for C, Hc, Wc in geoms])):
        assert len(v) == len(FIELDS) + 12
        found[g] = dict(zip(FIELDS, v), p16=v[len(FIELDS):len(FIELDS) + 6], p4=v[len(FIELDS) + 6:])
    return found


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return build_probe(tmp_path_factory)


@pytest.fixture(scope="module")
def plans(probe):
    listed = set(U8_FWD_GEOMS + F32_FWD_GEOMS + NAN_GEOMS + (WIDE_GEOM, WRAP_GEOM)) | \
        {g[:3] for g in U8_WGRAD_GEOMS + F32_WGRAD_GEOMS}
    return plans_of(probe, sorted(set(RANGE) | listed))


def test_plan_header_is_host_only_code():
    """conv1_plan.h through the probe, which includes nothing else of the library: plain C++17, no warnings, nothing from
    ROCm on the include path, no device builtin; and conv.hip takes its first-layer plans from it."""
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", CSRC, PROBE], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr
    with open(os.path.join(CSRC, "conv1_plan.h")) as f:
        code = "\n".join(ln.split("//")[0] for ln in f.read().splitlines())
    for word in ("hip", "__builtin", "__device__", "__global__", "curla_opt(", "curla_cu_count"):
        assert word not in code, word
    with open(os.path.join(CSRC, "conv.hip")) as f:
        text = "\n".join(ln.split("//")[0] for ln in f.read().splitlines())
    assert '#include "conv1_plan.h"' in text
    for name in ("u8_row_bytes", "f32_row_floats", "u8_band_rows", "plan_u8_bands", "plan_band_conv1", "conv1_u8_band_lds",
                 "wgrad1_u8_lds", "conv1_u8_rw_grid", "select_conv1_u8_form", "select_conv1_f32_form",
                 "select_wgrad1_u8_form"):
        assert f" {name}(" in code, name
        assert name in ("f32_row_floats", "u8_band_rows") or f"conv1::{name}(" in text, name  # (those two: the header's own)
    for arithmetic in ("& ~15) + 16", "& ~3) + 4", "best_eff", "1LL << 28"):  # (what moved has left)
        assert arithmetic not in text, arithmetic


# ------------------------------------------------------------------------------------------------- band invariants
def bands_of(Ho, th, nbands):
    """rows of every band"""
    return [min(th, Ho - k * th) for k in range(nbands)]


def test_band_invariants(plans):
    bad = []
    for (C, Hc, Wc), p in plans.items():
        Ho, Wo = p["Ho"], p["Wo"]
        ok = (Ho, Wo) == out_hw(Hc, Wc) and p["RSb"] >= Wc * C + 16 and p["RSb"] % 16 == 0
        ok = ok and p["RSf"] >= Wc * C + 4 and p["RSf"] % 4 == 0
        # uint8 bands (forward and weight gradient: one budget): tile Ho exactly, none empty, within budget and launch
        for th, nb, launch in ((p["th"], p["nbands"], (p["lds"],)), (p["wth"], p["wnbands"], (p["wlds_f32"], p["wlds_b16"]))):
            rows = bands_of(Ho, th, nb)
            ok = ok and th >= 1 and nb >= 1 and sum(rows) == Ho and min(rows) >= 1 and max(rows) == th
            band = (2 * th + 1) * p["RSb"]
            ok = ok and (band <= U8_BUDGET or th == 1) and all(band <= b <= MAX_LDS for b in launch)
            # (near-equal bands: no plan with fewer bands fits, and the last band is at most nbands - 1 rows short)
            ok = ok and (nb == 1 or (2 * (-(-Ho // (nb - 1))) + 1) * p["RSb"] > U8_BUDGET) and th - rows[-1] < nb
        # float bands
        for th, launch, budget in ((p["fth"], p["flds"], F32_FWD_BUDGET), (p["gth"], p["glds"], F32_WGRAD_BUDGET)):
            nb = -(-Ho // th)
            rows = bands_of(Ho, th, nb)
            band = (2 * th + 1) * p["RSf"] * 4
            ok = ok and 1 <= th <= Ho and sum(rows) == Ho and min(rows) >= 1
            ok = ok and (band <= budget or th == 1) and band <= launch <= MAX_LDS
        # the hybrid: one band, rows of at most 64 16-byte runs
        if U8_FORM_NAMES[p["f_hybrid"]] == "hybrid":
            ok = ok and p["nbands"] == 1 and Wc * C <= 1024
        ok = ok and U8_FORM_NAMES[p["f_band"]] == "band" and U8_FORM_NAMES[p["f_rw"]] == "rw"
        ok = ok and U8_FORM_NAMES[p["f_auto"]] == U8_FORM_NAMES[p["f_rwb"]] == ("rwb" if C <= 10 else "rw")
        ok = ok and p["w_f32"] == 1 and p["w_auto"] == p["w_b16"] == (0 if Wo >= 8 and C <= 10 else 1)
        ok = ok and (p["s_nhwc_rw"], p["s_nhwc_band"], p["s_nchw_rw"]) == (0, 1, 1)
        if not ok:
            bad.append(((C, Hc, Wc), p))
    assert not bad, bad[:5]
    # the shapes the comments of conv.hip and the issue name
    assert (plans[(9, 84, 84)]["th"], plans[(9, 84, 84)]["nbands"]) == (41, 1)
    assert (plans[(9, 76, 135)]["th"], plans[(9, 76, 135)]["nbands"]) == (19, 2)


# --------------------------------------------------------------------------------------------- row-walk invariants
def test_row_walk_strip_invariants(plans):
    """rw::plan_units over Wo output columns: 16 lane groups (the forward walks), 4 (wgrad1_rw)"""
    bad = []
    for (C, Hc, Wc), p in plans.items():
        for per, (nfull, brem, nr, nseg, ntr, steps) in ((16, p["p16"]), (4, p["p4"])):
            rows, cols = p["Ho"], p["Wo"]
            ok = nfull * per + brem == cols and 0 <= brem < per and steps == nfull * rows + ntr * nr
            if brem == 0:
                ok = ok and nr == nseg == ntr == 0
            else:
                ok = ok and 1 <= nr <= rows and (nseg - 1) * nr < rows <= nseg * nr
                ok = ok and (ntr - 1) * per < brem * nseg <= ntr * per
            if not ok:
                bad.append(((C, Hc, Wc), per, p["p16"], p["p4"]))
    assert not bad, bad[:10]


def shares(pool, grid, nw):
    """[lo, hi) of every wave of every workgroup of the uint8 row walk (conv1_u8_body / conv1_u8b_body): a workgroup an
    equal contiguous share of the pool, its waves equal shares of that"""
    per, rem = divmod(pool, grid)
    out = []
    for bid in range(grid):
        g0, ln = bid * per + min(bid, rem), per + (1 if bid < rem else 0)
        out += [(g0 + ln * w // nw, g0 + ln * (w + 1) // nw) for w in range(nw)]
    return out


def longest_piece(lo, hi, strip_rows):
    """the longest run of consecutive rows of ONE strip inside [lo, hi) of a pool of strips of strip_rows steps"""
    best, g = 0, lo
    while g < hi:
        n = min(hi - g, strip_rows - g % strip_rows)
        best, g = max(best, n), g + n
    return best


def test_row_walk_grid_and_shares(probe, plans):
    """the grid rule (pool, share of 8 steps per wave, cap -> grid) and the waves' shares: a partition of the pool, for
    small, medium and capped pools on every CU count; the copy of the rule the GPU tests derive their batch from"""
    pools = [1, 7, 8, 9, 63, 64, 65, 1000, 4095, 4096, 4097, 50000, 69632, 70001, 1 << 20]
    asks = [(b16, pool, cus) for b16 in (0, 1) for pool in pools for cus in CU_COUNTS]
    for (b16, pool, cus), (grid, nw) in zip(asks, ask(probe, [f"grid {b} {p} {c}" for b, p, c in asks])):
        assert (grid, nw) == u8_rw_grid(pool, bool(b16), cus)
        assert nw == (4 if b16 else 8) and 1 <= grid <= (3 if b16 else 2) * cus
        assert grid == (3 if b16 else 2) * cus or grid * 8 * nw >= pool > (grid - 1) * 8 * nw
        s = shares(pool, grid, nw)
        assert s[0][0] == 0 and s[-1][1] == pool and all(a[1] == b[0] for a, b in zip(s, s[1:]))
        assert all(lo <= hi for lo, hi in s)


def test_rotation_wrap_case_really_wraps(probe, plans):
    """the GPU test's batch for the rotation wrap: on 256 CUs (and the other counts) the capped grid leaves every wave at
    least 17 steps, and a wave a piece of at least 16 consecutive rows of the one 34-row strip -- past the 15 unrolled
    steps; one sample fewer per CU ... the batch is the smallest with that share"""
    C, Hc, Wc = WRAP_GEOM
    p = plans[WRAP_GEOM]
    assert (p["Ho"], p["Wo"]) == (34, 16) and p["p16"] == (1, 0, 0, 0, 0, 34)
    assert U8_FORM_NAMES[p["f_rw"]] == "rw" and U8_FORM_NAMES[p["f_rwb"]] == "rwb"
    for cus in CU_COUNTS:
        for b16 in (False, True):
            B = wrap_batch(b16, cus)
            (grid, nw), = ask(probe, [f"grid {int(b16)} {B * 34} {cus}"])
            assert grid == (3 if b16 else 2) * cus
            s = shares(B * 34, grid, nw)
            assert min(hi - lo for lo, hi in s) >= 17
            assert max(longest_piece(lo, hi, 34) for lo, hi in s) >= 17
            (grid1, _), = ask(probe, [f"grid {int(b16)} {(B - 1) * 34} {cus}"])
            assert min(hi - lo for lo, hi in shares((B - 1) * 34, grid1, nw)) < 17
    # (8 steps per wave below the cap: what every other test of the walks runs)
    assert wrap_batch(False, 256) == 2048 and wrap_batch(True, 256) == 1536


# ------------------------------------------------------------------------------------------------------- coverage
def wo_class(Wo):
    return "1" if Wo == 1 else "2-7" if Wo < 8 else "8-15" if Wo < 16 else "16" if Wo == 16 else "17-128" if Wo <= 128 \
        else "> 128"


def band_regimes(Ho, Wo, th, nbands):
    """bands and the tiles of 16 pixels (8 waves a pass) of the first and the last band"""
    last = Ho - (nbands - 1) * th
    a = {("bands", (min(nbands, 3), "full" if last == th else "one row" if last == 1 else "short"))}
    for rows in {th, last}:
        npix = rows * Wo
        a.add(("tiles", ("< 8" if (npix + 15) // 16 < 8 else ">= 8", "npix mod 16 = 0" if npix % 16 == 0 else "ragged")))
    return a


def strip_regimes(rows, per, plan):
    """the regime attributes of tests/test_conv_plan_host.py for one plan_units plan"""
    nfull, brem, nr, nseg, ntr, _ = plan
    a = {("min(nfull, 2)", min(nfull, 2)),
         ("brem", "0" if brem == 0 else "1" if brem == 1 else "per - 1" if brem == per - 1 else "in between")}
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


def regimes(operation, form, geom, p):
    """{(attribute, value)} of one geometry under one form of one operation"""
    C, Hc, Wc = geom
    Ho, Wo = p["Ho"], p["Wo"]
    a = {("C", C), ("Wo", wo_class(Wo)), ("Ho mod 2", Ho % 2), ("crop", (Hc % 2, Wc % 2))}
    if operation == "u8 forward":
        chosen = U8_FORM_NAMES[p["f_" + form]]
        a.add(("form", chosen))
        pitch = ring_of(C, Hc, Wc)[2] * C
        if chosen == "band":
            a |= band_regimes(Ho, Wo, p["th"], p["nbands"])
            runs = (2 * p["th"] + 1) * ((Wc * C + 15) // 16)
            a.add(("first staging pass", "< 3584 runs" if runs < 3584 else "= 3584 runs" if runs == 3584 else "> 3584 runs"))
        else:
            a |= strip_regimes(Ho, 16, p["p16"])
            a.add(("row pitch mod 4", "0 (aligned walk)" if pitch % 4 == 0 else "not 0"))
            if chosen == "hybrid":
                a.add(("row bytes mod 16", "0" if (Wc * C) % 16 == 0 else "not 0"))
    elif operation == "u8 weight gradient":
        chosen = ("b16", "f32")[p["w_" + form]]
        a |= {("form", chosen), ("form, Wo", (chosen, wo_class(Wo)))} | band_regimes(Ho, Wo, p["wth"], p["wnbands"])
        if Wo in (7, 8):
            a.add(("Wo at the bf16 form's limit", Wo))
        if chosen == "f32" and C == 9:
            a.add(("tail column (9 C mod 16 = 1), Wo", wo_class(Wo)))
    else:
        a.add(("NHWC row floats mod 4", (Wc * C) % 4))
        if form == "nhwc rw":
            a |= strip_regimes(Ho, 16, p["p16"]) if operation == "f32 forward" else strip_regimes(Ho, 4, p["p4"])
        else:
            th = p["fth"] if operation == "f32 forward" else p["gth"]
            a |= band_regimes(Ho, Wo, th, -(-Ho // th))
    return a


OPERATIONS = {
    "u8 forward": (U8_FWD_GEOMS, U8_FORMS),
    "f32 forward": (F32_FWD_GEOMS, F32_SOURCES),
    "u8 weight gradient": (tuple(g[:3] for g in U8_WGRAD_GEOMS), U8_WGRAD_FORMS),
    "f32 weight gradient": (tuple(g[:3] for g in F32_WGRAD_GEOMS), F32_SOURCES),
}


def everywhere(operation, form, plans, geoms=RANGE):
    """{regime: the smallest geometry of the range that has it}"""
    found = {}
    for g in sorted(geoms, key=lambda g: (g[0] * g[1] * g[2], g)):
        for a in regimes(operation, form, g, plans[g]):
            found.setdefault(a, g)
    return found


@pytest.mark.parametrize("operation", list(OPERATIONS))
def test_sweep_covers_every_regime(plans, operation):
    geoms, forms = OPERATIONS[operation]
    assert len(geoms) == len(set(geoms)) <= MAX_GEOMS
    assert all(batch_of(Hc, Wc) in (2, 3) for _, Hc, Wc in geoms)
    for form in forms:
        want = everywhere(operation, form, plans)
        listed = set()
        for g in geoms:
            listed |= regimes(operation, form, g, plans[g])
        missing = {a: g for a, g in want.items() if a not in listed}
        assert not missing, f"{operation} [{form}]: regimes no listed geometry has (and one that does): {missing}"
    # (all of these occur in the range, so the loop above already demands them; stated for the reader)
    if operation == "u8 forward":
        band = set().union(*(regimes(operation, "band", g, plans[g]) for g in geoms))
        assert {("bands", (3, "one row")), ("bands", (2, "short")), ("bands", (1, "full")), ("Wo", "1"), ("Wo", "16"),
                ("Wo", "> 128"), ("first staging pass", "= 3584 runs"), ("first staging pass", "> 3584 runs")} <= band
        assert any(regimes(operation, "hybrid", g, plans[g]) >= {("form", "band")} for g in geoms)
    if operation == "u8 weight gradient":
        b16 = set().union(*(regimes(operation, "b16", g, plans[g]) for g in geoms))
        assert {("form, Wo", ("f32", "2-7")), ("form, Wo", ("b16", "8-15"))} <= b16
        assert any(plans[g]["Wo"] == 7 for g in geoms) and any(plans[g]["Wo"] == 8 for g in geoms)


def test_listed_band_counts_and_derived_cases(plans):
    """what the GPU module states about its geometries holds by the plans: the band counts behind the slab counts, the
    two-problem cases, the wide-row case"""
    for C, Hc, Wc, nbands in U8_WGRAD_GEOMS:
        assert nbands == plans[(C, Hc, Wc)]["wnbands"], (C, Hc, Wc)
    for C, Hc, Wc, nbands in F32_WGRAD_GEOMS:
        p = plans[(C, Hc, Wc)]
        assert nbands == -(-p["Ho"] // p["gth"]), (C, Hc, Wc)
    assert len(FWD2_GEOMS) == 3 and set(FWD2_GEOMS) <= set(U8_FWD_GEOMS)
    for g in FWD2_GEOMS:  # (3 + 2 samples: under both walks a wave's share straddles the two problems' border)
        steps = plans[g]["p16"][5]
        for b16 in (False, True):
            grid, nw = u8_rw_grid(5 * steps, b16, 256)
            assert any(lo < 3 * steps < hi for lo, hi in shares(5 * steps, grid, nw)), (g, b16)
    assert len({g[0] for g in FWD2_GEOMS}) == 3
    p = plans[WIDE_GEOM]
    assert (p["th"], p["nbands"], p["wth"], p["wnbands"]) == (6, 2, 6, 2) and U8_FORM_NAMES[p["f_hybrid"]] == "band"
    assert (2 * 10 + 1) * p["RSb"] <= U8_BUDGET < (2 * 11 + 1) * p["RSb"] and p["Ho"] == 11  # (ten rows fit: 6 + 5)
    # one band in every form: the small crops of the NaN, second-item and alignment tests
    for g in NAN_GEOMS + ((3, 5, 7), (3, 5, 19), (12, 9, 11), (9, 10, 13)):
        p = plans[g]
        assert p["nbands"] == p["wnbands"] == 1 and p["fth"] == p["gth"] == p["Ho"], g
    assert ("b16", "f32")[plans[(3, 5, 19)]["w_b16"]] == "b16" and ("b16", "f32")[plans[(3, 5, 7)]["w_b16"]] == "f32"
    assert {g[0] for g in NAN_GEOMS} == set(CHANNELS)
