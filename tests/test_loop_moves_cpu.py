"""Register moves inside the traversal loops of the lean quad kernels, counted from the cross-compiled library's disassembly by
tools/loop_moves.py (no GPU).  These kernels are bound by VALU issue, and a plain `v_mov_b32 vA, vB`
inside a traversal loop is an instruction every lane of a step pays for a register layout, not for a result: before the leaf /
instance step was reordered (kernels/trace.h GBL_FUSE_LEAF_FIRST) the ray's twelve registers were copied to temporaries and back at
every such step.  A ratchet like the spill pin of tests/test_kernel_resources_cpu.py, not a tolerance: the counts may only go down.

Which loops: a kernel's queries each have a one-ray-per-lane loop and a quad loop (the exact_ties kernels also the exact loops
behind them).  In the disassembly they are the loops of TRAVERSAL_VALU[0] ... [1] VALU instructions that lie in no other loop of
that size: the shading and regeneration loops are larger, the triangle and item loops smaller or inside one of these.  The band is
wide on purpose (the loops in question have 280 to 540 instructions): a small loop of the shading code that falls into it only adds
its moves to the sum, and the test first checks that it found at least as many loops as the kernel has queries' loops, so a compiler
that moves one out of the band fails the test instead of emptying it.
"""
import json
import os
import re
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "goblin_amd", "lib", "libgoblin_hip.so")
TRAVERSAL_VALU = (200, 600)

# kernel: (loops found at least, plain moves inside them at most, plain moves in the whole kernel at most)   # the parent's moves: loops / kernel
BOUNDS = {
    r"path_trace_kernel<0, false, false, true, false, false>": (8, 129, 251),                  # 208 / 330
    r"path_trace_kernel<0, false, false, true, false, true>": (5, 71, 256),                    # 148 / 333   (the headline kernel)
    r"path_trace_kernel<0, false, false, true, true, false>": (10, 183, 337),                  # 341 / 495
    r"path_trace_kernel<0, false, false, true, true, true>": (7, 125, 343),                    # 278 / 496
    r"ao_kernel<0, false, false, true, false>": (4, 70, 163),                                  # 151 / 244
    r"ao_kernel<0, false, false, true, true>": (6, 124, 252),                                  # 291 / 419
}


@pytest.fixture(scope="module")
def rows():
    assert os.path.exists(LIB), "build the HIP library first (__graft_entry__.build())"
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "loop_moves.py"), "--json", "--kernel",
                          r"(path_trace_kernel|ao_kernel)<0, false, false, true", LIB], capture_output=True, text=True, check=True).stdout
    return json.loads(out)


def _kernel(rows, want):
    hits = [r for r in rows if re.search(r"\b" + re.escape(want) + r"\(", r["name"])]
    assert len(hits) == 1, (want, [r["name"] for r in hits])
    return hits[0]


def traversal_loops(row):
    loops = row["loops"]

    def in_band(lp):
        return TRAVERSAL_VALU[0] <= lp["valu"] <= TRAVERSAL_VALU[1]

    out = []
    for lp in loops:
        p, nested = lp["parent"], False
        while p >= 0:
            nested = nested or in_band(loops[p])
            p = loops[p]["parent"]
        if in_band(lp) and not nested:
            out.append(lp)
    return out


@pytest.mark.parametrize("want", list(BOUNDS))
def test_plain_moves_in_the_traversal_loops_do_not_come_back(rows, want):
    n_loops, loop_moves, kernel_moves = BOUNDS[want]
    row = _kernel(rows, want)
    found = traversal_loops(row)
    print("%-58s %s | %d plain moves in them, %d in the kernel" % (want, [(lp["valu"], lp["mov"]) for lp in found],
                                                                     sum(lp["mov"] for lp in found), row["mov"]))
    assert len(found) >= n_loops, (want, [(lp["start"], lp["valu"]) for lp in found])
    assert sum(lp["mov"] for lp in found) <= loop_moves, (want, [(lp["valu"], lp["mov"]) for lp in found])
    assert row["mov"] <= kernel_moves, (want, row["mov"])


def test_lane_traffic_of_the_headline_kernel_agrees_with_its_spills(rows):
    """The tool's totals against tools/kernel_resources.py: the headline kernel spills no vector register, so it has no scratch
    traffic to hide moves in, and every spilled SGPR is written with v_writelane and read with v_readlane at least once -- the
    v_readlane / v_writelane total cannot be under twice the spilled SGPRs."""
    want = r"path_trace_kernel<0, false, false, true, false, true>"
    row = _kernel(rows, want)
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "--json", LIB], capture_output=True, text=True,
                         check=True).stdout
    res = _kernel(json.loads(out), want)
    assert res["symbol"].replace(".kd", "") == row["symbol"]
    assert res.get("vgpr_spill_count", 0) == 0 and res.get("private_segment_fixed_size", 0) == 0
    assert row["lane"] >= 2 * res.get("sgpr_spill_count", 0), (row["lane"], res.get("sgpr_spill_count"))
    assert row["valu"] >= row["mov"] + row["lane"] + row["cndmask"]
    inside = [lp for lp in row["loops"] if lp["parent"] < 0]
    assert inside and max(lp["valu"] for lp in inside) <= row["valu"]
