"""tools/isa_diff.py on hand-written listings (tests/golden/isa_diff): the parser and the matching, pinned.  CPU only."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "isa_diff")


def run(old, new):
    cmd = [sys.executable, os.path.join(ROOT, "tools", "isa_diff.py")] + [os.path.join(GOLD, f) for f in old] + ["--"]
    return subprocess.run(cmd + [os.path.join(GOLD, f) for f in new], capture_output=True, text=True)


def test_same_kernels_in_other_listings_match():
    """Two kernels of one listing against the same two spread over two listings: other function numbers in the local
    labels, other trailing comments, and the plain C kernel now in an anonymous namespace."""
    r = run(["one.s"], ["two_a.s", "two_b.s"])
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == ("2 kernels against 2: 0 missing, 0 new, 0 differing instruction sequences, "
                                "0 differing descriptors")


def test_differences_are_named_and_fail():
    """One changed instruction and one changed descriptor line in a template instance, one kernel gone, one new."""
    r = run(["one.s"], ["changed.s"])
    assert r.returncode == 1, r.stdout + r.stderr
    out = r.stdout
    assert "only in the first set:  plain_kernel (one.s)" in out
    assert "only in the second set: extra_kernel (changed.s)" in out
    assert "tp_kernel<2>: instructions differ" in out and "+v_add_u32_e32 v1, 2, v1" in out
    assert "tp_kernel<2>: descriptor differ" in out and "+.amdhsa_next_free_vgpr 8" in out
    assert out.strip().endswith("2 kernels against 2: 1 missing, 1 new, 1 differing instruction sequences, "
                                "1 differing descriptors")
