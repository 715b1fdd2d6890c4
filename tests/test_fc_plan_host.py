"""Which kernel an encoder-fc product takes (csrc/fc_plan.h), on the CPU: the header is host-only code, so a small
program (tests/capi/fc_plan_probe.cpp, built with the address and undefined-behaviour sanitizers, its own process)
prints the plan and the kernels' walk numbers of every shape that tests/test_gpu_fc_edges.py launches (tests/_fc_cases.py
holds the lists for both modules).  Two assertions:

* every line equals EXPECTED below.  EXPECTED was recorded from the code as it stood before the decisions moved into the
  header -- the conditions of curla_fc_fwd_multi, fc_bwd_check / curla_fc_dx, fc_dw_impl, fc_bwd_impl and launch_fc_bwd
  copied out of gemm.hip into a scratch program, the walk numbers from the kernels' own loops run on the host -- not from
  the header;
* taken together, the shapes reach every instantiation, walk regime, fallback and refusal of REQUIRED: removing a
  shape that is the last witness of one of them fails here, without a GPU."""
import os
import re
import subprocess

import pytest

from tests import _fc_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "curla_amd", "csrc")
PROBE = os.path.join(ROOT, "tests", "capi", "fc_plan_probe.cpp")


# ------------------------------------------------------------------------------------------ the probe's lines, rebuilt
def fwd(nt, b3, grid, nrg, slices, mod4, chunks, odd_start):
    """fc_fwd_kernel<nt, 2 if nt == 3 else 0, b3>; mod4: which (s1 - s0) mod 4 occur, digit m for remainder m"""
    return f"fwd rc=0 fc_fwd_kernel<{nt},{2 if nt == 3 else 0},{'true' if b3 else 'false'}> grid={grid} lds=67584 " \
           f"nrg={nrg} slices={slices[0]}..{slices[1]} mod4={mod4} chunks={chunks[0]}..{chunks[1]} odd_start={odd_start}"


def dx(ks, grid, btiles, last):
    return f"dx rc=0 fc_dx_kernel<{ks}> grid={grid} lds=0 btiles={btiles[0]}..{btiles[1]} last={last}"


def dw(nt, grid, ksteps, last):
    """fc_dw_kernel<nt>: 16 KB of LDS per feature tile; no case here carries deferred LayerNorm sums into it"""
    return f"dw rc=0 fc_dw_kernel<{nt}> grid={grid} lds={16384 * nt} ln_launch=0 ksteps={ksteps[0]}..{ksteps[1]} last={last}"


def one_pass(entry, nt, with_dx, grid, btiles, last):
    """fc_bwd_kernel<13, nt, 2 if nt == 3 else 0, with_dx> from curla_fc_bwd* (entry "bwd") or curla_fc_dw* ("dw")"""
    return f"{entry} rc=0 fc_bwd_kernel<13,{nt},{2 if nt == 3 else 0},{'true' if with_dx else 'false'}> grid={grid} " \
           f"lds=65536 btiles={btiles[0]}..{btiles[1]} last={last}"


def two(dx_line, dw_line):
    return f"bwd rc=0 two {dx_line} {dw_line}"


def refused(entry):
    return f"{entry} rc=-3"  # CURLA_ERR_UNSUPPORTED


# launch shape (tests/_fc_cases.plan_cases) -> the probe's line, recorded as the module docstring says
EXPECTED = {
    "fwd 128x50x32 np1 ns1 [auto]": fwd(3, 1, 1, 1, (1, 1), "0100", (1, 1), 0),
    "fwd 128x50x32 np1 ns1 [f32]": fwd(3, 0, 1, 1, (1, 1), "0100", (1, 1), 0),
    "fwd 128x52x64 np2 ns1 [auto]": fwd(4, 1, 2, 1, (2, 2), "0010", (1, 1), 0),
    "fwd 128x52x64 np2 ns1 [f32]": fwd(4, 0, 2, 1, (2, 2), "0010", (1, 1), 0),
    "fwd 256x54x96 np3 ns1 [auto]": fwd(4, 1, 6, 2, (3, 3), "0001", (1, 1), 0),
    "fwd 256x54x96 np3 ns1 [f32]": fwd(4, 0, 6, 2, (3, 3), "0001", (1, 1), 0),
    "fwd 128x58x128 np4 ns1 [auto]": fwd(4, 1, 4, 1, (4, 4), "1000", (1, 1), 0),
    "fwd 128x58x128 np4 ns1 [f32]": fwd(4, 0, 4, 1, (4, 4), "1000", (1, 1), 0),
    "fwd 128x62x160 np1 ns1 [auto]": fwd(4, 1, 1, 1, (5, 5), "0100", (2, 2), 0),
    "fwd 128x62x160 np1 ns1 [f32]": fwd(4, 0, 1, 1, (5, 5), "0100", (2, 2), 0),
    "fwd 128x64x288 np2 ns1 [auto]": fwd(4, 1, 2, 1, (9, 9), "0100", (3, 3), 0),
    "fwd 128x64x288 np2 ns1 [f32]": fwd(4, 0, 2, 1, (9, 9), "0100", (3, 3), 0),
    "fwd 128x50x64 np2 ns1 [auto]": fwd(3, 1, 2, 1, (2, 2), "0010", (1, 1), 0),
    "fwd 128x50x64 np2 ns1 [f32]": fwd(3, 0, 2, 1, (2, 2), "0010", (1, 1), 0),
    "fwd 128x50x96 np1 ns1 [auto]": fwd(3, 1, 1, 1, (3, 3), "0001", (1, 1), 0),
    "fwd 128x50x96 np1 ns1 [f32]": fwd(3, 0, 1, 1, (3, 3), "0001", (1, 1), 0),
    "fwd 256x50x128 np1 ns1 [auto]": fwd(3, 1, 2, 2, (4, 4), "1000", (1, 1), 0),
    "fwd 256x50x128 np1 ns1 [f32]": fwd(3, 0, 2, 2, (4, 4), "1000", (1, 1), 0),
    "fwd 128x50x160 np4 ns1 [auto]": fwd(3, 1, 4, 1, (5, 5), "0100", (2, 2), 0),
    "fwd 128x50x160 np4 ns1 [f32]": fwd(3, 0, 4, 1, (5, 5), "0100", (2, 2), 0),
    "fwd 128x50x288 np3 ns1 [auto]": fwd(3, 1, 3, 1, (9, 9), "0100", (3, 3), 0),
    "fwd 128x50x288 np3 ns1 [f32]": fwd(3, 0, 3, 1, (9, 9), "0100", (3, 3), 0),
    "fwd 256x50x352 np2 ns3 [auto]": fwd(3, 1, 12, 2, (3, 4), "1001", (1, 1), 1),
    "fwd 256x50x352 np2 ns3 [f32]": fwd(3, 0, 12, 2, (3, 4), "1001", (1, 1), 1),
    "fwd 128x54x352 np1 ns3 [auto]": fwd(4, 1, 3, 1, (3, 4), "1001", (1, 1), 1),
    "fwd 128x54x352 np1 ns3 [f32]": fwd(4, 0, 3, 1, (3, 4), "1001", (1, 1), 1),
    "fwd 128x50x416 np1 ns13 [auto]": fwd(3, 1, 13, 1, (1, 1), "0100", (1, 1), 1),
    "fwd 128x50x416 np1 ns13 [f32]": fwd(3, 0, 13, 1, (1, 1), "0100", (1, 1), 1),
    "fwd 128x64x416 np1 ns13 [auto]": fwd(4, 1, 13, 1, (1, 1), "0100", (1, 1), 1),
    "fwd 128x64x416 np1 ns13 [f32]": fwd(4, 0, 13, 1, (1, 1), "0100", (1, 1), 1),
    "fwd 128x52x1184 np1 ns5 [auto]": fwd(4, 1, 5, 1, (7, 8), "1001", (2, 2), 1),
    "fwd 128x52x1184 np1 ns5 [f32]": fwd(4, 0, 5, 1, (7, 8), "1001", (2, 2), 1),
    "fwd 128x50x1184 np1 ns5 [auto]": fwd(3, 1, 5, 1, (7, 8), "1001", (2, 2), 1),
    "fwd 128x50x1184 np1 ns5 [f32]": fwd(3, 0, 5, 1, (7, 8), "1001", (2, 2), 1),
    "dx 1x1x4": dx(4, 1, (0, 1), "one"),
    "dx 16x1x64": dx(4, 1, (0, 1), "full"),
    "dx 67x1x68": dx(4, 2, (1, 2), "one"),
    "dx 200x1x252": dx(4, 4, (3, 4), "part"),
    "dx 17x4x4": dx(4, 1, (0, 1), "one"),
    "dx 130x4x64": dx(4, 1, (2, 3), "full"),
    "dx 1x4x68": dx(4, 2, (0, 1), "one"),
    "dx 16x4x252": dx(4, 4, (0, 1), "part"),
    "dx 200x5x4": dx(4, 1, (3, 4), "one"),
    "dx 3x5x64": dx(4, 1, (0, 1), "full"),
    "dx 17x5x68": dx(4, 2, (0, 1), "one"),
    "dx 130x5x252": dx(4, 4, (2, 3), "part"),
    "dx 16x16x4": dx(4, 1, (0, 1), "one"),
    "dx 67x16x64": dx(4, 1, (1, 2), "full"),
    "dx 200x16x68": dx(4, 2, (3, 4), "one"),
    "dx 3x16x252": dx(4, 4, (0, 1), "part"),
    "dx 130x17x4": dx(8, 1, (2, 3), "one"),
    "dx 1x17x64": dx(8, 1, (0, 1), "full"),
    "dx 16x17x68": dx(8, 2, (0, 1), "one"),
    "dx 67x17x252": dx(8, 4, (1, 2), "part"),
    "dx 3x32x4": dx(8, 1, (0, 1), "one"),
    "dx 17x32x64": dx(8, 1, (0, 1), "full"),
    "dx 130x32x68": dx(8, 2, (2, 3), "one"),
    "dx 1x32x252": dx(8, 4, (0, 1), "part"),
    "dx 67x33x4": dx(13, 1, (1, 2), "one"),
    "dx 200x33x64": dx(13, 1, (3, 4), "full"),
    "dx 3x33x68": dx(13, 2, (0, 1), "one"),
    "dx 17x33x252": dx(13, 4, (0, 1), "part"),
    "dx 1x52x4": dx(13, 1, (0, 1), "one"),
    "dx 16x52x64": dx(13, 1, (0, 1), "full"),
    "dx 67x52x68": dx(13, 2, (1, 2), "one"),
    "dx 200x52x252": dx(13, 4, (3, 4), "part"),
    "dx 17x53x4": dx(16, 1, (0, 1), "one"),
    "dx 130x53x64": dx(16, 1, (2, 3), "full"),
    "dx 1x53x68": dx(16, 2, (0, 1), "one"),
    "dx 16x53x252": dx(16, 4, (0, 1), "part"),
    "dx 200x64x4": dx(16, 1, (3, 4), "one"),
    "dx 3x64x64": dx(16, 1, (0, 1), "full"),
    "dx 17x64x68": dx(16, 2, (0, 1), "one"),
    "dx 130x64x252": dx(16, 4, (2, 3), "part"),
    "dx 130x52x196": dx(13, 4, (2, 3), "one"),
    "dx 200x64x196": dx(16, 4, (3, 4), "one"),
    "dw 1x7x4": dw(1, 1, (0, 1), "one"),
    "dw 5x7x64": dw(1, 1, (0, 1), "full"),
    "dw 13x7x68": dw(1, 2, (1, 1), "one"),
    "dw 30x7x252": dw(1, 4, (2, 2), "part"),
    "dw 30x16x4": dw(1, 1, (2, 2), "one"),
    "dw 32x16x64": dw(1, 1, (2, 2), "full"),
    "dw 36x16x68": dw(1, 2, (2, 3), "one"),
    "dw 116x16x252": dw(1, 4, (7, 8), "part"),
    "dw 116x17x4": dw(2, 1, (7, 8), "one"),
    "dw 130x17x64": dw(2, 1, (8, 9), "full"),
    "dw 131x17x68": dw(2, 2, (8, 9), "one"),
    "dw 260x17x252": dw(2, 4, (16, 17), "part"),
    "dw 260x24x4": dw(2, 1, (16, 17), "one"),
    "dw 1x24x64": dw(2, 1, (0, 1), "full"),
    "dw 5x24x68": dw(2, 2, (0, 1), "one"),
    "dw 13x24x252": dw(2, 4, (1, 1), "part"),
    "dw 13x32x4": dw(2, 1, (1, 1), "one"),
    "dw 30x32x64": dw(2, 1, (2, 2), "full"),
    "dw 32x32x68": dw(2, 2, (2, 2), "one"),
    "dw 36x32x252": dw(2, 4, (2, 3), "part"),
    "dw 36x33x4": dw(3, 1, (2, 3), "one"),
    "dw 116x33x64": dw(3, 1, (7, 8), "full"),
    "dw 130x33x68": dw(3, 2, (8, 9), "one"),
    "dw 131x33x252": dw(3, 4, (8, 9), "part"),
    "dw 131x48x4": dw(3, 1, (8, 9), "one"),
    "dw 260x48x64": dw(3, 1, (16, 17), "full"),
    "dw 1x48x68": dw(3, 2, (0, 1), "one"),
    "dw 5x48x252": dw(3, 4, (0, 1), "part"),
    "dw 5x50x4": dw(4, 1, (0, 1), "one"),
    "dw 13x50x64": dw(4, 1, (1, 1), "full"),
    "dw 30x50x68": dw(4, 2, (2, 2), "one"),
    "dw 36x50x252": dw(4, 4, (2, 3), "part"),
    "dw 32x64x4": dw(4, 1, (2, 2), "one"),
    "dw 36x64x64": dw(4, 1, (2, 3), "full"),
    "dw 116x64x68": dw(4, 2, (7, 8), "one"),
    "dw 130x64x252": dw(4, 4, (8, 9), "part"),
    "dw 260x50x68": dw(4, 2, (16, 17), "one"),
    "dw 131x50x196": dw(4, 4, (8, 9), "one"),
    "dw 32x64x196": dw(4, 4, (2, 2), "one"),
    "dw 116x7x64": dw(1, 1, (7, 8), "full"),
    "dw 1x33x4": dw(3, 1, (0, 1), "one"),
    "bwd 16x49x4": one_pass("bwd", 4, 1, 1, (0, 1), "one"),
    "bwd 64x49x64": one_pass("bwd", 4, 1, 1, (1, 1), "full"),
    "bwd 128x49x68": one_pass("bwd", 4, 1, 2, (2, 2), "one"),
    "bwd 192x49x252": one_pass("bwd", 4, 1, 4, (3, 3), "part"),
    "bwd 128x50x4": one_pass("bwd", 3, 1, 1, (2, 2), "one"),
    "dw 128x50x4": one_pass("dw", 3, 0, 1, (2, 2), "one"),
    "bwd 192x50x64": one_pass("bwd", 3, 1, 1, (3, 3), "full"),
    "dw 192x50x64": one_pass("dw", 3, 0, 1, (3, 3), "full"),
    "bwd 16x50x68": one_pass("bwd", 3, 1, 2, (0, 1), "one"),
    "dw 16x50x68": one_pass("dw", 3, 0, 2, (0, 1), "one"),
    "bwd 64x50x252": one_pass("bwd", 3, 1, 4, (1, 1), "part"),
    "dw 64x50x252": one_pass("dw", 3, 0, 4, (1, 1), "part"),
    "bwd 192x51x4": one_pass("bwd", 4, 1, 1, (3, 3), "one"),
    "bwd 16x51x64": one_pass("bwd", 4, 1, 1, (0, 1), "full"),
    "bwd 64x51x68": one_pass("bwd", 4, 1, 2, (1, 1), "one"),
    "bwd 128x51x252": one_pass("bwd", 4, 1, 4, (2, 2), "part"),
    "bwd 48x52x4": one_pass("bwd", 4, 1, 1, (0, 1), "one"),
    "bwd 80x52x64": one_pass("bwd", 4, 1, 1, (1, 2), "full"),
    "bwd 144x52x68": one_pass("bwd", 4, 1, 2, (2, 3), "one"),
    "bwd 208x52x252": one_pass("bwd", 4, 1, 4, (3, 4), "part"),
    "bwd 16x50x196": one_pass("bwd", 3, 1, 4, (0, 1), "one"),
    "dw 16x50x196": one_pass("dw", 3, 0, 4, (0, 1), "one"),
    "bwd 80x50x64": one_pass("bwd", 3, 1, 1, (1, 2), "full"),
    "dw 80x50x64": one_pass("dw", 3, 0, 1, (1, 2), "full"),
    "bwd 144x50x68": one_pass("bwd", 3, 1, 2, (2, 3), "one"),
    "dw 144x50x68": one_pass("dw", 3, 0, 2, (2, 3), "one"),
    "bwd 208x50x252": one_pass("bwd", 3, 1, 4, (3, 4), "part"),
    "dw 208x50x252": one_pass("dw", 3, 0, 4, (3, 4), "part"),
    "bwd 192x50x4": one_pass("bwd", 3, 1, 1, (3, 3), "one"),
    "dw 192x50x4": one_pass("dw", 3, 0, 1, (3, 3), "one"),
    "bwd 128x51x196": one_pass("bwd", 4, 1, 4, (2, 2), "one"),
    "bwd 208x49x64": one_pass("bwd", 4, 1, 1, (3, 4), "full"),
    "bwd 144x52x4": one_pass("bwd", 4, 1, 1, (2, 3), "one"),
    "bwd 16x50x196 ln": one_pass("bwd", 3, 1, 5, (0, 1), "one"),
    "dw 16x50x196 ln": one_pass("dw", 3, 0, 5, (0, 1), "one"),
    "bwd 80x50x64 ln": one_pass("bwd", 3, 1, 2, (1, 2), "full"),
    "dw 80x50x64 ln": one_pass("dw", 3, 0, 2, (1, 2), "full"),
    "bwd 208x50x252 ln": one_pass("bwd", 3, 1, 5, (3, 4), "part"),
    "dw 208x50x252 ln": one_pass("dw", 3, 0, 5, (3, 4), "part"),
    "bwd 128x51x196 ln": one_pass("bwd", 4, 1, 5, (2, 2), "one"),
    "bwd 208x49x64 ln": one_pass("bwd", 4, 1, 2, (3, 4), "full"),
    "bwd 144x52x4 ln": one_pass("bwd", 4, 1, 2, (2, 3), "one"),
    "bwd 16x50x196 ln2": one_pass("bwd", 3, 1, 5, (0, 1), "one"),
    "bwd 208x49x64 ln2": one_pass("bwd", 4, 1, 2, (3, 4), "full"),
    "bwd 80x50x64 ln2": one_pass("bwd", 3, 1, 2, (1, 2), "full"),
    "bwd 144x52x4 ln2": one_pass("bwd", 4, 1, 2, (2, 3), "one"),
    "bwd 32x48x68 fallback": two(dx(13, 2, (0, 1), "one"), dw(3, 2, (2, 2), "one")),
    "dw 32x48x68 fallback": dw(3, 2, (2, 2), "one"),
    "bwd 32x53x64 fallback": two(dx(16, 1, (0, 1), "full"), dw(4, 1, (2, 2), "full")),
    "dw 32x53x64 fallback": dw(4, 1, (2, 2), "full"),
    "bwd 24x50x196 fallback": two(dx(13, 4, (0, 1), "one"), dw(4, 4, (1, 2), "one")),
    "dw 24x50x196 fallback": dw(4, 4, (1, 2), "one"),
    "bwd 40x51x64 fallback": two(dx(13, 1, (0, 1), "full"), dw(4, 1, (2, 3), "full")),
    "dw 40x51x64 fallback": dw(4, 1, (2, 3), "full"),
    "bwd 17x13x4 fallback": two(dx(4, 1, (0, 1), "one"), dw(1, 1, (1, 2), "one")),
    "dw 17x13x4 fallback": dw(1, 1, (1, 2), "one"),
    "bwd 40x50x252 fallback": two(dx(13, 4, (0, 1), "part"), dw(4, 4, (2, 3), "part")),
    "dw 40x50x252 fallback": dw(4, 4, (2, 3), "part"),
    "bwd 64x64x64 fallback": two(dx(16, 1, (1, 1), "full"), dw(4, 1, (4, 4), "full")),
    "dw 64x64x64 fallback": dw(4, 1, (4, 4), "full"),
    "fwd 128x50x96 chain [auto]": fwd(3, 1, 1, 1, (3, 3), "0001", (1, 1), 0),
    "fwd 128x50x96 chain [f32]": fwd(3, 0, 1, 1, (3, 3), "0001", (1, 1), 0),
    "bwd 128x50x96 chain": one_pass("bwd", 3, 1, 3, (2, 2), "part"),
    "fwd 128x52x96 chain [auto]": fwd(4, 1, 1, 1, (3, 3), "0001", (1, 1), 0),
    "fwd 128x52x96 chain [f32]": fwd(4, 0, 1, 1, (3, 3), "0001", (1, 1), 0),
    "bwd 128x52x96 chain": one_pass("bwd", 4, 1, 3, (2, 2), "part"),
    "fwd refused: F odd": refused("fwd"),
    "fwd refused: F below 50": refused("fwd"),
    "fwd refused: F above 64": refused("fwd"),
    "fwd refused: B % 128 != 0": refused("fwd"),
    "fwd refused: K % 32 != 0": refused("fwd"),
    "fwd refused: nsplit above K / 32": refused("fwd"),
    "fwd refused: odd split stride": refused("fwd"),
    "dx refused: F above 64": refused("dx"),
    "dw refused: F above 64": refused("dw"),
    "bwd refused: F above 64": refused("bwd"),
    "dx refused: K % 4 != 0": refused("dx"),
    "dw refused: K % 4 != 0": refused("dw"),
    "bwd refused: K % 4 != 0": refused("bwd"),
}


# ------------------------------------------------------------------------------------------------------- coverage
def k_class(K):
    return "K=4" if K == 4 else "K%64==0" if K % 64 == 0 else "K%64==4" if K % 64 == 4 else "K%64==60" if K % 64 == 60 \
        else "K other"


def reached(cases, lines):
    """the attributes of REQUIRED that the cases (name, probe input, kind) with the probe's lines reach"""
    got = set()
    for (name, inp, kind), line in zip(cases, lines):
        entry, B, F, K, nprob, nsplit, _stride, _mfma, _ln = inp.split()
        B, F, K, nprob, nsplit = int(B), int(F), int(K), int(nprob), int(nsplit)
        if kind == "refuse":
            if line == refused(entry):
                got.add(name)
            continue
        m = re.fullmatch(r"fwd rc=0 fc_fwd_kernel<(\d,\d),(\w+)> grid=\d+ lds=\d+ nrg=(\d+) slices=(\d+)\.\.(\d+) "
                         r"mod4=(\d{4}) chunks=(\d+)\.\.(\d+) odd_start=(\d)", line)
        if m:
            form, b3, nrg, smin, smax, mod4, _cmin, _cmax, odd = m.groups()
            got.add(f"fwd<{form}> b3={b3}")
            got.add(f"fwd nprob={nprob}")
            got.update(f"fwd slices={s}" for s in (int(smin), int(smax)) if s <= 5)  # (least and most both occur)
            got.update(f"fwd (s1-s0)%4=={r}" for r in range(4) if mod4[r] == "1")
            if int(smax) >= 9:
                got.add("fwd slices>=9")
            if odd == "1":
                got.add("fwd a split starts off a multiple of 4")
            if nsplit == K // 32 and nsplit > 1:
                got.add("fwd nsplit==K/32")
            if nsplit == 1:
                got.add("fwd nsplit==1")
            if form == "4,0":
                got.add(f"fwd<4,0> F%4=={F % 4}")
            if int(nrg) >= 2:
                got.add("fwd two or more row groups")
            continue
        for kernel, rest in re.findall(r"(fc_\w+_kernel<[\w,]+>) grid=(.*?)(?= dw rc=|$)", line):
            got.add(kernel)
            got.add(f"{kernel} {k_class(K)}")
            bt = re.search(r"btiles=(\d+)\.\.(\d+)", rest)
            if kernel.startswith("fc_dx"):
                if F in (1, 16, 17, 32, 33, 52, 53, 64):
                    got.add(f"fc_dx F={F}")
                got.add("fc_dx B<4" if B < 4 else "fc_dx B%16!=0" if B % 16 else "fc_dx B%16==0")
                ntiles = (B + 15) // 16
                got.update(t for t, n in (("fc_dx more than 4 b-tiles", 4), ("fc_dx more than 8 b-tiles", 8)) if ntiles > n)
            elif kernel.startswith("fc_dw"):
                if F == 50 and B % 16 != 0:
                    got.add(f"{kernel} F=50 B%16!=0" + (" from curla_fc_dw" if entry == "dw" else ""))
                got.add(f"fc_dw B%4=={B % 4}")
                for s in map(int, re.search(r"ksteps=(\d+)\.\.(\d+)", rest).groups()):
                    got.add("fc_dw k-steps>=17" if s >= 17 else f"fc_dw k-steps={s}")
            else:
                got.add(f"{kernel} F={F}")
                got.add(f"fc_bwd b-tiles=({bt.group(1)},{bt.group(2)})")
                extra = int(rest.split()[0]) - (K + 63) // 64
                assert extra in (0, 1)
                got.add("fc_bwd with the LnReduce workgroup" if extra else "fc_bwd without the LnReduce workgroup")
                if name.endswith(" ln2"):
                    assert extra == 1
                    got.add("fc_bwd with the second set of partials")
        if line.startswith("bwd rc=0 two"):
            got.add("curla_fc_bwd two launches: " + ("B%16!=0" if 49 <= F <= 52 else "F outside 49..52"))
    got.update(f"fwd x {'blocked' if b else 'row-major'}" for b in C.LAYOUTS)
    got.update(f"fc_dx {'with' if m else 'without'} mask" for m in C.DX_MASKS)
    return got


K_CLASSES = ("K=4", "K%64==0", "K%64==4", "K%64==60")
BWD_KERNELS = [f"fc_dx_kernel<{k}>" for k in (4, 8, 13, 16)] + [f"fc_dw_kernel<{n}>" for n in (1, 2, 3, 4)] + \
    ["fc_bwd_kernel<13,3,2,true>", "fc_bwd_kernel<13,4,0,true>", "fc_bwd_kernel<13,3,2,false>"]
REQUIRED = set(
    [f"fwd<{form}> b3={b3}" for form in ("3,2", "4,0") for b3 in ("true", "false")] +
    ["fwd x row-major", "fwd x blocked"] + [f"fwd nprob={n}" for n in (1, 2, 3, 4)] +
    [f"fwd slices={s}" for s in (1, 2, 3, 4, 5)] + ["fwd slices>=9"] + [f"fwd (s1-s0)%4=={r}" for r in range(4)] +
    ["fwd a split starts off a multiple of 4", "fwd nsplit==K/32", "fwd nsplit==1", "fwd<4,0> F%4==0", "fwd<4,0> F%4==2",
     "fwd two or more row groups"] +
    [f"fc_dx F={F}" for F in (1, 16, 17, 32, 33, 52, 53, 64)] +
    ["fc_dx with mask", "fc_dx without mask", "fc_dx B<4", "fc_dx B%16!=0", "fc_dx B%16==0", "fc_dx more than 4 b-tiles",
     "fc_dx more than 8 b-tiles"] +
    ["fc_dw_kernel<4> F=50 B%16!=0", "fc_dw_kernel<4> F=50 B%16!=0 from curla_fc_dw"] + [f"fc_dw B%4=={r}" for r in range(4)] +
    [f"fc_dw k-steps={s}" for s in (0, 1, 7, 8, 9)] + ["fc_dw k-steps>=17"] +
    ["fc_bwd_kernel<13,3,2,true> F=50", "fc_bwd_kernel<13,3,2,false> F=50"] +
    [f"fc_bwd_kernel<13,4,0,true> F={F}" for F in (49, 51, 52)] +
    [f"fc_bwd b-tiles=({a},{b})" for a, b in ((0, 1), (1, 1), (1, 2), (2, 2), (2, 3), (3, 3), (3, 4))] +
    ["fc_bwd with the LnReduce workgroup", "fc_bwd without the LnReduce workgroup", "fc_bwd with the second set of partials"] +
    BWD_KERNELS + [f"{k} {c}" for k in BWD_KERNELS for c in K_CLASSES] +
    ["curla_fc_bwd two launches: B%16!=0", "curla_fc_bwd two launches: F outside 49..52"] +
    [f"fwd refused: {why}" for why in ("F odd", "F below 50", "F above 64", "B % 128 != 0", "K % 32 != 0",
                                       "nsplit above K / 32", "odd split stride")] +
    [f"{e} refused: {why}" for e in ("dx", "dw", "bwd") for why in ("F above 64", "K % 4 != 0")])


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fc_plan") / "fc_plan_probe")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", CSRC, PROBE, "-o", exe])
    return exe


def run_probe(probe, cases):
    r = subprocess.run([probe], input="\n".join(inp for _, inp, _ in cases) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    return lines


def test_plan_header_is_host_only_code():
    """fc_plan.h through the probe, which includes nothing else of the library: plain C++17, no warnings, nothing from
    ROCm on the include path; and it asks neither the options nor the device anything itself."""
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", CSRC, PROBE], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr
    with open(os.path.join(CSRC, "fc_plan.h")) as f:
        code = "\n".join(ln.split("//")[0] for ln in f.read().splitlines())
    for word in ("hip", "curla_opt", "curla_cu_count"):
        assert word not in code.replace("curla_hip.h", ""), word


def test_plans_match_the_recorded_table(probe):
    cases = C.plan_cases()
    names = [n for n, _, _ in cases]
    assert len(set(names)) == len(names)
    assert sorted(EXPECTED) == sorted(names)  # every launch shape of the GPU module, nothing else
    wrong = [(n, g, EXPECTED[n]) for n, g in zip(names, run_probe(probe, cases)) if g != EXPECTED[n]]
    assert not wrong, "\n".join(f"{n}:\n  got  {g}\n  want {w}" for n, g, w in wrong[:10])


def test_every_case_is_accepted_or_meant_to_be_refused(probe):
    """no GPU case can be refused at run time by surprise: a 'run' shape has a kernel, a 'refuse' shape has none -- and
    a refused shape breaks the one condition it is named for, no other"""
    cases = C.plan_cases()
    for (name, _, kind), line in zip(cases, run_probe(probe, cases)):
        assert ("rc=0" in line and "rc=-3" not in line) == (kind == "run"), (name, line)
    for why, B, F, K, nprob, ns, extra in C.FWD_REFUSALS:
        broken = {"F odd": F % 2 != 0 and 50 <= F <= 64, "F below 50": F < 50, "F above 64": F > 64, "B % 128 != 0": B % 128 != 0,
                  "K % 32 != 0": K % 32 != 0, "nsplit above K / 32": ns > K // 32 and K % 32 == 0,
                  "odd split stride": (B * F + extra) % 2 != 0}
        assert [w for w, b in broken.items() if b] == [why], (why, broken)
    for why, B, F, K in C.BWD_REFUSALS:
        assert [w for w, b in (("F above 64", F > 64), ("K % 4 != 0", K % 4 != 0)) if b] == [why]


def test_the_case_lists_reach_every_instantiation_and_walk(probe):
    cases = C.plan_cases()
    got = reached(cases, run_probe(probe, cases))
    assert not REQUIRED - got, sorted(REQUIRED - got)


def test_every_listed_shape_stays_tiny():
    """K from 4 to 288 (the forward: one shape at 1184), B at most 260"""
    for B, F, K, *_ in C.FWD_CASES + C.CHAIN_CASES:
        assert B <= 256 and (K <= 416 or K == 1184)
    for B, F, K, *_ in C.DX_CASES + C.DW_CASES + C.ONE_PASS_CASES + C.FALLBACK_CASES + C.LN2_CASES:
        assert B <= 260 and 4 <= K <= 288
    assert set(C.ONE_PASS_LN_CASES) <= set(C.ONE_PASS_CASES) and {c[:3] for c in C.LN2_CASES} <= set(C.ONE_PASS_CASES)
