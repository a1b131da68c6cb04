#!/usr/bin/env python3
"""What a vertex edit costs through the host entry and through the device entry.  bunny.json's bunny
alternates between its own pose and the pose twisted by 10 degrees (tools/refit_bench.py's twist), so every edit changes
every vertex; for both BVH builders, medians of --calls wall times, the four kinds of call alternating in one process:

  host_ms            gbl_update_vertices with the pose in host memory (the yardstick)
  device_ms          gbl_update_vertices_device with the pose in device memory, the tie order made in the call
  deferred_ms        ... with GBL_VERTICES_DEFER_ORDER
  first_exact_ms     the first exact_ties render (64 x 64, 1 spp) after a deferred edit, which makes the order, beside
  exact_ms           the same render again, with nothing pending
  frame_host_ms      one frame of README's loop in its host form: vertices() to numpy, the edit from numpy, a --resolution x --spp
                     render, render_aov and motion with the previous pose from numpy, and
  frame_device_ms    in its device form: vertices(device=True), the deferred edit from a tensor, the same three calls with
                     the previous pose a tensor.

Prints one JSON line.

    python tools/vertices_device_bench.py [--calls 7] [--resolution 512] [--spp 16]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from goblin_amd import _abi  # noqa: E402
from goblin_amd import scene as gs  # noqa: E402
from goblin_amd.renderer import HipPathTracer  # noqa: E402
from refit_bench import mesh_positions, twisted, wall_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--spp", type=int, default=16)
    a = ap.parse_args()
    with open(gs.scene_path("bunny")) as f:
        doc = json.load(f)
    gs._merge(doc, gs.config_overrides(resolution=(a.resolution, a.resolution), spp=a.spp, depth=8))
    scene = gs.load_scene_text(json.dumps(doc), gs.SCENE_DIR)
    small = _abi.gbl_render_setting.from_buffer_copy(scene.desc.setting)
    small.sample_per_pixel = 1
    window = (0, 64, 0, 64)
    P = [mesh_positions(scene, 0)]
    P.append(twisted(P[0], 10.0))
    result = {"device": torch.cuda.get_device_name(0), "calls": a.calls, "resolution": a.resolution, "spp": a.spp,
              "triangles": int(scene.desc.meshes[0].tri_count), "vertices": len(P[0]), "builders": {}}
    for bvh in ("host", "device"):
        r = HipPathTracer(scene, 0, bvh=bvh)
        D = [torch.from_numpy(p).to(r.device) for p in P]
        film = r.new_film()
        cam = r.camera()
        exact = lambda: r.render(setting=small, window=window, exact_ties=True, schedule="megakernel")   # noqa: E731
        r.update_vertices(0, P[1])   # warm-up: the plan, the kernels' code objects, the buffers
        r.update_vertices(0, D[0], defer_order=True)
        exact()
        r.render(film=film, schedule="megakernel")
        r.render_aov()
        r.motion(cam, None, prev_vertices={0: D[1]})
        t = {k: [] for k in ("host_ms", "device_ms", "deferred_ms", "first_exact_ms", "exact_ms", "frame_host_ms", "frame_device_ms")}
        pose = 0
        for _ in range(a.calls):
            pose ^= 1
            t["host_ms"].append(wall_ms(lambda: r.update_vertices(0, P[pose])))
            pose ^= 1
            t["device_ms"].append(wall_ms(lambda: r.update_vertices(0, D[pose])))
            pose ^= 1
            t["deferred_ms"].append(wall_ms(lambda: r.update_vertices(0, D[pose], defer_order=True)))
            assert r.order_pending(0) == 1
            t["first_exact_ms"].append(wall_ms(exact))
            assert r.order_pending(0) == 0
            t["exact_ms"].append(wall_ms(exact))

            def frame_host():
                prev = r.vertices(0)
                r.update_vertices(0, P[pose ^ 1])
                r.render(film=film, schedule="megakernel")
                aov = r.render_aov()
                r.motion(cam, None, normal=aov["normal"], prev_vertices={0: prev})

            def frame_device():
                prev = r.vertices(0, device=True)
                r.update_vertices(0, D[pose ^ 1], defer_order=True)
                r.render(film=film, schedule="megakernel")
                aov = r.render_aov()
                r.motion(cam, None, normal=aov["normal"], prev_vertices={0: prev})
            t["frame_host_ms"].append(wall_ms(frame_host))
            pose ^= 1
            t["frame_device_ms"].append(wall_ms(frame_device))
            pose ^= 1
            assert r.order_pending(0) == 1   # (the frame's three calls are lean: nobody asked for the order)
        row = {k: statistics.median(v) for k, v in t.items()}
        row.update({k + "_min_max": [min(v), max(v)] for k, v in t.items()})
        result["builders"][bvh] = row
        del r
    print(json.dumps(result))


if __name__ == "__main__":
    main()
