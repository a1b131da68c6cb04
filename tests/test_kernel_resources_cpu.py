"""The register budget of the lean quad kernels, read from the cross-compiled library's code-object metadata (no GPU):
with the SLP vectoriser off for their unit (goblin_amd/build.py UNIT_FLAGS) none of them spills a vector register or
touches scratch memory.  A spill in these kernels is VALU and memory work inside the traversal loops of the kernel the
headline step spends nine tenths of its time in."""
import json
import os
import re
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LEAN_QUAD = [r"path_trace_kernel<0, false, false, true, false, false>", r"path_trace_kernel<0, false, false, true, false, true>",
             r"path_trace_kernel<0, false, false, true, true, false>", r"path_trace_kernel<0, false, false, true, true, true>",
             r"ao_kernel<0, false, false, true, false>", r"ao_kernel<0, false, false, true, true>"]


def test_lean_quad_kernels_spill_no_vgpr_and_use_no_scratch():
    lib = os.path.join(REPO, "goblin_amd", "lib", "libgoblin_hip.so")
    assert os.path.exists(lib), "build the HIP library first (__graft_entry__.build())"
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "--json", lib],
                         capture_output=True, text=True, check=True).stdout
    rows = json.loads(out)
    for want in LEAN_QUAD:
        hits = [r for r in rows if re.search(r"\b" + re.escape(want) + r"\(", r["name"])]
        assert len(hits) == 1, (want, [r["name"] for r in hits])
        r = hits[0]
        print("%-60s vgpr %d, spilled vgpr %d, spilled sgpr %d, scratch %d B" % (want, r.get("vgpr_count", -1), r.get("vgpr_spill_count", 0),
                                                                                  r.get("sgpr_spill_count", 0), r.get("private_segment_fixed_size", 0)))
        assert r.get("vgpr_spill_count", 0) == 0, (want, r.get("vgpr_spill_count"))
        assert r.get("private_segment_fixed_size", 0) == 0, (want, r.get("private_segment_fixed_size"))


def test_source_stamp_covers_the_compiler_flags(monkeypatch):
    """The same sources under other flags are another binary: counters collected from one must not be quoted for the other."""
    from goblin_amd import build
    stamp = build.source_stamp()
    assert build.unit_flags("kernels_quad") == build.unit_flags(os.path.join(build.CSRC, "kernels_quad.hip")) == ["-fno-slp-vectorize"]
    monkeypatch.setattr(build, "UNIT_FLAGS", dict(build.UNIT_FLAGS, kernels_quad=[]))
    assert build.source_stamp() != stamp
    monkeypatch.undo()
    monkeypatch.setattr(build, "HIP_FLAGS", build.HIP_FLAGS + ["-DX"])
    assert build.source_stamp() != stamp
    monkeypatch.undo()
    assert build.source_stamp() == stamp
