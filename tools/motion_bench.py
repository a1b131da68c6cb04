#!/usr/bin/env python3
"""Device time of gbl_render_motion (no instance moved; every instance moved, with and without a normal film) and of
gbl_film_accumulate_motion (with the variance plane and without it), beside what they are read against: gbl_film_accumulate of the
same frame and a 1-spp gbl_render_aov of the same context, in the same process, alternating.  BASELINE configs[1] (bunny 512^2) and
the Cornell box at 1024^2.  tools/temporal_bench.py's method: HIP events, one warm-up round, the median and the spread of --calls
rounds, each timing --batch calls between two events, divided.  Prints one JSON line.

On the bunny also gbl_render_motion_deform (DESIGN.md 4.8 "Deforming meshes"): the bunny twisted by 10 degrees (tools/refit_bench.py's
twist) with its untwisted positions as the previous pose -- no mesh deformed (the current positions listed), deformed with a normal
film, deformed without one -- beside gbl_render_motion of the same context; and "deform_upload_ms", the host-to-device copy of the
previous positions and the per-mesh table alone, on the same stream.

    python tools/motion_bench.py [--calls 7] [--batch 10] [--configs bunny cornell]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from goblin_amd import _abi  # noqa: E402
from goblin_amd import scene as gs  # noqa: E402
from goblin_amd.renderer import HipPathTracer  # noqa: E402
from refit_bench import twisted  # noqa: E402
from temporal_bench import CONFIGS, summary, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--configs", nargs="+", default=list(CONFIGS))
    a = ap.parse_args()
    result = {"calls": a.calls, "batch": a.batch, "device": torch.cuda.get_device_name(0), "configs": {}}
    for name in a.configs:
        scene, res, _, depth = CONFIGS[name]
        r = HipPathTracer(gs.load_scene(scene, gs.config_overrides(resolution=res, spp=4, depth=depth)), 0)
        one = _abi.gbl_render_setting.from_buffer_copy(r.scene.desc.setting)
        one.sample_per_pixel = 1
        cam0 = r.camera()
        # the previous frame: a camera a little to the side and every instance a little lower, accumulated once
        r.update_camera(position=(cam0.position[0] - 0.02, cam0.position[1], cam0.position[2]))
        prev = r.camera()
        prev_aov = r.render_aov()
        history = r.accumulate(r.render()["film"], prev_aov["depth"], None, prev_aov["normal"])["history"]
        r.update_camera(position=tuple(cam0.position))
        still = r.instances()
        lower = [((p[0], p[1] - 0.01, p[2]), q, s) for p, q, s in still]
        beauty = r.new_film()
        li = r.render(film=beauty, want_li=True)["li"]
        films = r.render_aov()
        variance = r.variance(li)
        planes = r.motion(prev, lower, normal=films["normal"])
        scratch = {k: r.new_film() for k in ("albedo", "normal", "depth")}
        variants = {
            "aov_1spp": lambda: timed(lambda: r.render_aov(films=scratch, setting=one), a.batch),
            "motion_static": lambda: timed(lambda: r.motion(prev, None, normal=films["normal"]), a.batch),
            "motion_all_moved": lambda: timed(lambda: r.motion(prev, lower, normal=films["normal"]), a.batch),
            "motion_all_moved_no_normal": lambda: timed(lambda: r.motion(prev, lower), a.batch),
            "accumulate_variance_plane": lambda: timed(lambda: r.accumulate(beauty, films["depth"], variance, films["normal"], history, prev), a.batch),
            "accumulate_motion_variance_plane": lambda: timed(lambda: r.accumulate(beauty, films["depth"], variance, films["normal"], history, motion=planes), a.batch),
            "accumulate_spatial": lambda: timed(lambda: r.accumulate(beauty, films["depth"], None, films["normal"], history, prev), a.batch),
            "accumulate_motion_spatial": lambda: timed(lambda: r.accumulate(beauty, films["depth"], None, films["normal"], history, motion=planes), a.batch),
        }
        times = {k: [] for k in variants}
        for rep in range(a.calls + 1):     # (the first round warms up: buffers, clocks)
            for k, fn in variants.items():
                ms = fn()
                if rep:
                    times[k].append(ms)
        row = {k: summary(v) for k, v in times.items()}
        med = {k: v["median_ms"] for k, v in row.items()}
        row["motion_over_aov_1spp"] = med["motion_static"] / med["aov_1spp"]
        row["accumulate_motion_over_accumulate"] = {"variance_plane": med["accumulate_motion_variance_plane"] / med["accumulate_variance_plane"],
                                                    "spatial": med["accumulate_motion_spatial"] / med["accumulate_spatial"]}
        if name == "bunny":
            rest = r.vertices(0)
            r.update_vertices(0, twisted(rest, 10.0))
            now = r.vertices(0)
            nbytes = rest.nbytes + 4 * int(r.scene.desc.num_meshes)
            host = np.zeros(nbytes, np.uint8)        # pageable, as the context's staging copy is
            dev = torch.empty(nbytes, dtype=torch.uint8, device=r.device)
            deform = {
                "deform_motion_static": lambda: timed(lambda: r.motion(prev, None, normal=films["normal"]), a.batch),
                "deform_none_deformed": lambda: timed(lambda: r.motion(prev, None, normal=films["normal"], prev_vertices={0: now}), a.batch),
                "deform_deformed": lambda: timed(lambda: r.motion(prev, None, normal=films["normal"], prev_vertices={0: rest}), a.batch),
                "deform_deformed_no_normal": lambda: timed(lambda: r.motion(prev, None, prev_vertices={0: rest}), a.batch),
                "deform_upload": lambda: timed(lambda: dev.copy_(torch.from_numpy(host), non_blocking=True), a.batch),
            }
            dtimes = {k: [] for k in deform}
            for rep in range(a.calls + 1):
                for k, fn in deform.items():
                    ms = fn()
                    if rep:
                        dtimes[k].append(ms)
            row.update({k: summary(v) for k, v in dtimes.items()})
            med = {k: row[k]["median_ms"] for k in deform}
            row["deform_over_motion"] = {k: med[k] / med["deform_motion_static"] for k in ("deform_none_deformed", "deform_deformed", "deform_deformed_no_normal")}
            row["deform_vertices"] = int(len(rest))
            row["deform_upload_bytes"] = int(nbytes)
        row["pixels"] = res[0] * res[1]
        row["instances"] = len(still)
        row["pixels_with_history"] = float((r.accumulate(beauty, films["depth"], variance, films["normal"], history, motion=planes)["history"][0, ..., 3] > 1).float().mean())
        result["configs"][name] = row
        del r
    print(json.dumps(result))


if __name__ == "__main__":
    main()
