#!/usr/bin/env python3
"""Device time of gbl_film_accumulate, with the variance plane (SPATIAL off) and without it (SPATIAL on), first frame and with a
reprojected history, beside gbl_film_denoise (5 levels, all guides; and 1 level, for the cost of one a-trous level) and
gbl_render of the same configuration in the same process, alternating: BASELINE configs[1] (bunny 512^2, 256 spp) and the Cornell
box at 1024^2 x 64 spp.  HIP events, one warm-up round, the median and the spread of --calls rounds; each film timing is --batch
calls between two events, divided.  Also the host time of gbl_update_camera beside gbl_info.build_ms of the same scene: what
re-creating the context cost per frame.  Prints one JSON line.

    python tools/temporal_bench.py [--calls 7] [--batch 10] [--configs bunny cornell]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from goblin_amd import scene as gs  # noqa: E402
from goblin_amd.renderer import HipPathTracer  # noqa: E402

CONFIGS = {"bunny": ("bunny", (512, 512), 256, 8), "cornell": ("cornell", (1024, 1024), 64, 16)}
# Bytes a pixel moves: the three films (and the variance plane) in, the 36 bytes of prepared planes out and in again, 48 of history
# in (each history pixel counted once: neighbouring lanes share their taps) and 16 + 4 + 48 out
BYTES_PER_PIXEL = {True: (16 + 4 + 16 + 16) + 2 * 36 + 4 + 48 + (16 + 4 + 48), False: (16 + 16 + 16) + 2 * 36 + 48 + (16 + 4 + 48)}


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
        cam0 = r.camera()
        # the previous frame: a camera a little to the side, accumulated once
        r.update_camera(position=(cam0.position[0] - 0.02, cam0.position[1], cam0.position[2]))
        prev = r.camera()
        prev_aov = r.render_aov()
        first = r.accumulate(r.render(want_li=False)["film"], prev_aov["depth"], None, prev_aov["normal"])
        history = first["history"]
        r.update_camera(position=tuple(cam0.position))
        li = r.render(film=beauty, want_li=True)["li"]
        r.render_aov(films=films)
        variance = r.variance(li)
        guides = dict(albedo=films["albedo"], normal=films["normal"], depth=films["depth"])
        share = float((r.accumulate(beauty, films["depth"], variance, films["normal"], history, prev)["history"][0, ..., 3] > 1).float().mean())

        def camera_edit():
            t0 = time.perf_counter()
            for _ in range(100):
                r.update_camera(position=tuple(cam0.position))
            return (time.perf_counter() - t0) * 10.0      # ms per call (with the Python face's gbl_get_camera)

        variants = {
            "render": lambda: r.render(film=beauty, timed=True)["stats"]["kernel_ms"],
            "denoise_5_levels": lambda: timed(lambda: r.denoise(beauty, variance, iterations=5, **guides), a.batch),
            "denoise_1_level": lambda: timed(lambda: r.denoise(beauty, variance, iterations=1, **guides), a.batch),
            "denoise_2_levels": lambda: timed(lambda: r.denoise(beauty, variance, iterations=2, **guides), a.batch),
            "accumulate_variance_plane": lambda: timed(lambda: r.accumulate(beauty, films["depth"], variance, films["normal"], history, prev), a.batch),
            "accumulate_spatial": lambda: timed(lambda: r.accumulate(beauty, films["depth"], None, films["normal"], history, prev), a.batch),
            "accumulate_variance_plane_first_frame": lambda: timed(lambda: r.accumulate(beauty, films["depth"], variance, films["normal"]), a.batch),
            "accumulate_spatial_first_frame": lambda: timed(lambda: r.accumulate(beauty, films["depth"], None, films["normal"]), a.batch),
            "update_camera_host": camera_edit,
        }
        times = {k: [] for k in variants}
        for rep in range(a.calls + 1):     # (the first round warms up: buffers, the AUTO pilot, clocks)
            for k, fn in variants.items():
                ms = fn()
                if rep:
                    times[k].append(ms)
        row = {k: summary(v) for k, v in times.items()}
        med = {k: v["median_ms"] for k, v in row.items()}
        row["one_atrous_level_ms"] = med["denoise_2_levels"] - med["denoise_1_level"]
        row["accumulate_in_atrous_levels"] = {k: med[k] / row["one_atrous_level_ms"] for k in ("accumulate_variance_plane", "accumulate_spatial")}
        row["accumulate_over_render"] = med["accumulate_variance_plane"] / med["render"]
        row["pixels"] = res[0] * res[1]
        row["pixels_with_history"] = share
        row["bytes_per_pixel"] = {"variance_plane": BYTES_PER_PIXEL[True], "spatial": BYTES_PER_PIXEL[False]}
        row["gb_per_s"] = {"variance_plane": BYTES_PER_PIXEL[True] * row["pixels"] / med["accumulate_variance_plane"] * 1e-6,
                           "spatial": BYTES_PER_PIXEL[False] * row["pixels"] / med["accumulate_spatial"] * 1e-6}
        row["build_ms"] = r.info.build_ms
        result["configs"][name] = row
        del r
    print(json.dumps(result))


if __name__ == "__main__":
    main()
