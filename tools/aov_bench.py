#!/usr/bin/env python3
"""Device time of gbl_render_aov (all three films) beside gbl_render of the same configuration in the same process, alternating:
BASELINE configs[1] (bunny 512^2, 256 spp) and the Cornell box at 1024^2 x 64 spp.  HIP events (gbl_stats.kernel_ms), one
warm-up of each, the median and the spread of --calls calls.  Variants of the feature pass, each timed the same way: the packet
kernel against one ray per lane (GBL_AOV_PACKET, read per call), one film against three (what two more splats cost), and the
call in chunks of 64 samples per pixel (GBL_AOV_PASS_SPP).  Prints one JSON line.

    python tools/aov_bench.py [--calls 7] [--configs bunny cornell]

Under `rocprofv3 --kernel-trace --stats -- python tools/aov_bench.py --calls 3` the per-kernel rows give aov_packet_kernel,
aov_kernel and wf_splat on their own.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from goblin_amd import scene as gs  # noqa: E402
from goblin_amd.renderer import HipPathTracer  # noqa: E402

CONFIGS = {"bunny": ("bunny", (512, 512), 256, 8), "cornell": ("cornell", (1024, 1024), 64, 16)}


def summary(times):
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--configs", nargs="+", default=list(CONFIGS))
    a = ap.parse_args()
    result = {"calls": a.calls, "device": torch.cuda.get_device_name(0), "configs": {}}
    for name in a.configs:
        scene, res, spp, depth = CONFIGS[name]
        r = HipPathTracer(gs.load_scene(scene, gs.config_overrides(resolution=res, spp=spp, depth=depth)), 0)
        films = {k: r.new_film() for k in ("albedo", "normal", "depth")}
        beauty = r.new_film()

        def aov(env=None, **kw):
            for k, v in (env or {}).items():
                os.environ[k] = v
            try:
                return r.render_aov(films=None if kw else films, timed=True, **kw)["stats"]["kernel_ms"]
            finally:
                for k in (env or {}):
                    del os.environ[k]

        variants = {
            "aov": lambda: aov(),
            "aov_single_rays": lambda: aov({"GBL_AOV_PACKET": "0"}),
            "aov_exact_ties": lambda: r.render_aov(films=films, timed=True, exact_ties=True)["stats"]["kernel_ms"],
            "aov_one_film": lambda: aov(albedo=False, normal=True, depth=False),
            "aov_records_only": lambda: aov(albedo=False, normal=False, depth=False, want_samples=True),
            "aov_chunks_of_64": lambda: aov({"GBL_AOV_PASS_SPP": "64"}),
            "render": lambda: r.render(film=beauty, timed=True)["stats"]["kernel_ms"],
        }
        times = {k: [] for k in variants}
        for rep in range(a.calls + 1):     # (the first round warms up: buffers, the AUTO pilot, clocks)
            for k, fn in variants.items():
                ms = fn()
                if rep:
                    times[k].append(ms)
        row = {k: summary(v) for k, v in times.items()}
        row["paths"] = r.render_aov(films=films, timed=True)["stats"]["paths"]
        row["aov_over_render"] = row["aov"]["median_ms"] / row["render"]["median_ms"]
        result["configs"][name] = row
        del r
    print(json.dumps(result))


if __name__ == "__main__":
    main()
