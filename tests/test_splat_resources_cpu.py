"""The register budget of wf_splat (kernels/wavefront.h), read from the cross-compiled library's code-object metadata (no GPU),
in the style of tests/test_kernel_resources_cpu.py: counts only.

The splat keeps a lane's 25 x 4 sums in registers; with the windowed variants of its fast path beside the 25-cell body the
kernels hold 168 VGPRs under __launch_bounds__(GBL_BLOCK, 3) -- three waves per SIMD, the occupancy the kernel had before the
variants (156 VGPRs).  One register more is a step down to two waves; a spilled VGPR or a byte of scratch is memory traffic
inside the loop over the samples.  Four waves per SIMD (128 VGPRs) spill 200 registers with this compiler and are not forced."""
import json
import os
import re
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_VGPRS = 168   # the value the windowed variants reached; 512 / 168 = 3 waves per SIMD
SPLATS = [r"wf_splat<false, false>", r"wf_splat<false, true>", r"wf_splat<true, false>", r"wf_splat<true, true>"]


def test_splat_kernels_keep_three_waves_and_use_no_scratch():
    lib = os.path.join(REPO, "goblin_amd", "lib", "libgoblin_hip.so")
    assert os.path.exists(lib), "build the HIP library first (__graft_entry__.build())"
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "--json", lib],
                         capture_output=True, text=True, check=True).stdout
    rows = json.loads(out)
    for want in SPLATS:
        hits = [r for r in rows if re.search(r"\b" + re.escape(want) + r"\(", r["name"])]
        assert len(hits) == 1, (want, [r["name"] for r in hits])
        r = hits[0]
        print("%-26s vgpr %d, agpr %d, spilled vgpr %d, scratch %d B" % (want, r.get("vgpr_count", -1), r.get("agpr_count", 0),
                                                                         r.get("vgpr_spill_count", 0), r.get("private_segment_fixed_size", 0)))
        assert r.get("vgpr_count", 1 << 30) + r.get("agpr_count", 0) <= MAX_VGPRS, (want, r.get("vgpr_count"), r.get("agpr_count"))
        assert r.get("vgpr_spill_count", 0) == 0, (want, r.get("vgpr_spill_count"))
        assert r.get("private_segment_fixed_size", 0) == 0, (want, r.get("private_segment_fixed_size"))
