"""One fragment per bounce in the two quad path kernels that start at the primary pass's record (kernels/render_kernels.h, the PRIM
vertex step), pinned from the cross-compiled library's disassembly and metadata (tools/loop_moves.py, tools/kernel_resources.py; no
GPU).  A ratchet like tests/test_kernel_resources_cpu.py and tests/test_loop_moves_cpu.py: the counts may only go down.

Before the reorder make_fragment was in these kernels twice, about 310 VALU instructions each -- once for the lanes whose extension
ray returned a hit, once for the lanes that had just fetched a path -- and a wave issued both at almost every iteration, each
with part of its lanes.  These kernels are bound by VALU issue: what counts is the instructions the wave
issues at all.  The single site must not be paid for with a vector spill, nor with spilled-scalar traffic (v_readlane /
v_writelane) inside the traversal loops, which hold 70 % of the waves' ticks (profiles/lazy_draws_ab.txt: that is what made an
earlier form of the sample draws slower); and every instantiation without PRIM has one fragment site already and must come out of the
compiler as it did.
"""
import json
import os
import re
import subprocess
import sys

import pytest

from test_loop_moves_cpu import traversal_loops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "goblin_amd", "lib", "libgoblin_hip.so")

HEADLINE = r"path_trace_kernel<0, false, false, true, false, true>"
TWIN = r"path_trace_kernel<0, false, false, true, true, true>"        # exact_ties
# VALU instructions with both fragment sites: 6929 and 8575; one copy is 310, 60 are allowed for the new control flow
VALU_AT_MOST = {HEADLINE: 6929 - 250, TWIN: 8575 - 250}
# the lean kernels without PRIM: (VALU, plain moves, v_readlane + v_writelane, VGPRs, SGPRs, spilled VGPRs, spilled SGPRs, scratch bytes), as before
UNTOUCHED = {
    r"path_trace_kernel<0, false, false, true, false, false>": (6571, 250, 270, 168, 106, 0, 61, 0),
    r"path_trace_kernel<0, false, false, true, true, false>": (8387, 336, 611, 168, 106, 0, 106, 0),
    r"path_trace_kernel<0, false, false, false, false, false>": (5929, 177, 323, 162, 106, 0, 115, 0),
    r"path_trace_kernel<0, false, false, false, true, false>": (7502, 274, 556, 168, 106, 0, 164, 0),
}
# v_readlane + v_writelane inside the headline kernel's traversal loops, in address order: closest hit one ray per lane, closest hit
# quad, any hit one ray per lane, any hit quad
TRAVERSAL_LANE_OPS_AT_MOST = (3, 3, 3, 3)


def _rows(tool, *args):
    assert os.path.exists(LIB), "build the HIP library first (__graft_entry__.build())"
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", tool), "--json"] + list(args) + [LIB], capture_output=True, text=True, check=True).stdout
    return json.loads(out)


@pytest.fixture(scope="module")
def code():
    return _rows("loop_moves.py", "--kernel", r"path_trace_kernel<0, false, false, (true|false), (true|false), (true|false)>")


@pytest.fixture(scope="module")
def resources():
    return _rows("kernel_resources.py")


def _kernel(rows, want):
    hits = [r for r in rows if re.search(r"\b" + re.escape(want) + r"\(", r["name"])]
    assert len(hits) == 1, (want, [r["name"] for r in hits])
    return hits[0]


@pytest.mark.parametrize("want", [HEADLINE, TWIN])
def test_the_fragment_is_in_the_primary_kernels_once(code, resources, want):
    row, res = _kernel(code, want), _kernel(resources, want)
    print("%-58s %d VALU instructions (at most %d), %d lane operations, %d VGPRs, %d spilled SGPRs" % (
        want, row["valu"], VALU_AT_MOST[want], row["lane"], res.get("vgpr_count", -1), res.get("sgpr_spill_count", 0)))
    assert row["valu"] <= VALU_AT_MOST[want], (want, row["valu"])
    assert res.get("vgpr_count") == 168, (want, res.get("vgpr_count"))
    assert res.get("vgpr_spill_count", 0) == 0, (want, res.get("vgpr_spill_count"))
    assert res.get("private_segment_fixed_size", 0) == 0, (want, res.get("private_segment_fixed_size"))


@pytest.mark.parametrize("want", list(UNTOUCHED))
def test_the_kernels_without_the_pass_are_what_they_were(code, resources, want):
    row, res = _kernel(code, want), _kernel(resources, want)
    now = (row["valu"], row["mov"], row["lane"], res.get("vgpr_count"), res.get("sgpr_count"), res.get("vgpr_spill_count", 0),
           res.get("sgpr_spill_count", 0), res.get("private_segment_fixed_size", 0))
    assert now == UNTOUCHED[want], (want, now)


def test_spilled_scalars_stay_out_of_the_headline_kernels_traversal_loops(code):
    """The loops of tests/test_loop_moves_cpu.py's band, in address order: the closest-hit query's two, the regeneration round
    (which lies between the two queries), the any-hit query's two."""
    found = sorted(traversal_loops(_kernel(code, HEADLINE)), key=lambda lp: lp["start"])
    print([(lp["start"], lp["valu"], lp["lane"]) for lp in found])
    assert len(found) == 5, [(lp["start"], lp["valu"]) for lp in found]
    lanes = tuple(lp["lane"] for lp in found[:2] + found[3:])
    assert all(n <= most for n, most in zip(lanes, TRAVERSAL_LANE_OPS_AT_MOST)), lanes
