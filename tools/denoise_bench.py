#!/usr/bin/env python3
"""Device time of gbl_film_variance + gbl_film_denoise (5 levels, all guides) beside gbl_render and gbl_render_aov of the same
configuration in the same process, alternating: BASELINE configs[1] (bunny 512^2, 256 spp) and the Cornell box at 1024^2 x 64
spp.  HIP events, one warm-up round, the median and the spread of --calls rounds.

Also the level kernel's two builds per stride: the call at 1 .. 4 levels with every level tapping global memory
(GBL_DENOISE_LDS=0) and with every level staging its tile in LDS (=1); the cost of the level at stride 2^(L-1) is the call at L
levels minus the call at L - 1.  Each timing is --batch calls between two events, divided.  Prints one JSON line.

    python tools/denoise_bench.py [--calls 7] [--batch 10] [--configs bunny cornell]
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


def timed(fn, batch=1):
    """Milliseconds per call of fn between two HIP events on the current stream."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(batch):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--configs", nargs="+", default=list(CONFIGS))
    a = ap.parse_args()
    result = {"calls": a.calls, "batch": a.batch, "device": torch.cuda.get_device_name(0), "configs": {}}
    for name in a.configs:
        scene, res, spp, depth = CONFIGS[name]
        r = HipPathTracer(gs.load_scene(scene, gs.config_overrides(resolution=res, spp=spp, depth=depth)), 0)
        films = {k: r.new_film() for k in ("albedo", "normal", "depth")}
        beauty = r.new_film()
        li = r.render(film=beauty, want_li=True)["li"]
        r.render_aov(films=films)
        variance = r.variance(li)
        guides = dict(albedo=films["albedo"], normal=films["normal"], depth=films["depth"])

        def levels(n, lds):
            os.environ["GBL_DENOISE_LDS"] = lds
            try:
                return timed(lambda: r.denoise(beauty, variance, iterations=n, **guides), a.batch)
            finally:
                del os.environ["GBL_DENOISE_LDS"]

        variants = {
            "render": lambda: r.render(film=beauty, timed=True)["stats"]["kernel_ms"],
            "aov": lambda: r.render_aov(films=films, timed=True)["stats"]["kernel_ms"],
            "variance": lambda: timed(lambda: r.variance(li)),
            "denoise_5_levels": lambda: timed(lambda: r.denoise(beauty, variance, iterations=5, **guides)),
            "variance_and_denoise": lambda: timed(lambda: r.denoise(beauty, r.variance(li), iterations=5, **guides)),
            "denoise_5_levels_no_guides": lambda: timed(lambda: r.denoise(beauty, iterations=5)),
        }
        for n in range(0, 5):
            for lds in ("0", "1"):
                if n:
                    variants["levels_%d_lds_%s" % (n, lds)] = (lambda n=n, lds=lds: levels(n, lds))
        times = {k: [] for k in variants}
        for rep in range(a.calls + 1):     # (the first round warms up: buffers, the AUTO pilot, clocks)
            for k, fn in variants.items():
                ms = fn()
                if rep:
                    times[k].append(ms)
        row = {k: summary(v) for k, v in times.items()}
        med = {k: v["median_ms"] for k, v in row.items()}
        row["per_stride_ms"] = {}
        for n in range(1, 5):
            prev = {lds: med["levels_%d_lds_%s" % (n - 1, lds)] if n > 1 else None for lds in ("0", "1")}
            row["per_stride_ms"][str(1 << (n - 1))] = {
                "global": med["levels_%d_lds_0" % n] - (prev["0"] or 0.0), "lds": med["levels_%d_lds_1" % n] - (prev["1"] or 0.0),
                "includes_prepare_and_finish": n == 1}
        row["denoise_over_render"] = med["variance_and_denoise"] / med["render"]
        row["pixels"] = res[0] * res[1]
        result["configs"][name] = row
        del r
    print(json.dumps(result))


if __name__ == "__main__":
    main()
