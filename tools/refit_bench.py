#!/usr/bin/env python3
"""What a vertex edit costs and what the refitted tree costs to trace.  bunny.json's bunny (69 122
triangles) is twisted about its vertical axis, by --angles degrees over the mesh's height; for both BVH builders and every
angle:

  update_ms    wall time of update_vertices with the twisted positions: the median of --calls calls after one warm-up (the call
               synchronises the device), beside
  create_ms    the wall time of creating a context of the twisted scene afresh, and that context's gbl_info.build_ms;
  kernel_ms    of a render (--resolution, --spp) on the refitted tree and on the fresh context's, the median of --calls, alternating;
  nodes, tris  the traversal counters of a collect_stats render (4 spp) on either tree; and whether the two trees' per-sample
               radiance is the same tensor (exact_ties).

Prints one JSON line.

    python tools/refit_bench.py [--angles 0 5 20 60] [--calls 7] [--resolution 512] [--spp 16]
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from goblin_amd import _abi  # noqa: E402
from goblin_amd import scene as gs  # noqa: E402
from goblin_amd.renderer import HipPathTracer  # noqa: E402


def twisted(V, degrees):
    """V turned about the y axis by `degrees` x (height above the lowest vertex / the mesh's height), in float32."""
    y0, y1 = float(V[:, 1].min()), float(V[:, 1].max())
    a = np.radians(degrees) * (V[:, 1].astype(np.float64) - y0) / (y1 - y0)
    c, s = np.cos(a), np.sin(a)
    x, z = V[:, 0].astype(np.float64), V[:, 2].astype(np.float64)
    return np.stack([c * x + s * z, V[:, 1].astype(np.float64), -s * x + c * z], axis=1).astype(np.float32)


def twisted_scene(doc, degrees, workdir):
    """bunny.json loaded from a directory whose models/bunny.obj is the twisted mesh."""
    models = os.path.join(gs.SCENE_DIR, "models")
    d = os.path.join(workdir, "twist_%g" % degrees, "models")
    os.makedirs(d)
    shutil.copy(os.path.join(models, "plane.obj"), os.path.join(d, "plane.obj"))
    lines = open(os.path.join(models, "bunny.obj")).read().split("\n")
    at = [i for i, l in enumerate(lines) if l.startswith("v ")]
    V = twisted(np.array([[float(x) for x in lines[i].split()[1:4]] for i in at], np.float32), degrees)
    for i, v in zip(at, V):
        lines[i] = "v %.9g %.9g %.9g" % (float(v[0]), float(v[1]), float(v[2]))
    with open(os.path.join(d, "bunny.obj"), "w") as f:
        f.write("\n".join(lines))
    return gs.load_scene_text(json.dumps(doc), os.path.dirname(d))


def mesh_positions(scene, m):
    d = scene.desc
    gm = d.meshes[m]
    P = np.ctypeslib.as_array(d.positions, shape=(d.num_vertices * 3,)).reshape(-1, 3)
    return P[gm.vertex_offset:gm.vertex_offset + gm.vertex_count].astype(np.float32)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--angles", type=float, nargs="+", default=[0.0, 5.0, 20.0, 60.0])
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--spp", type=int, default=16)
    a = ap.parse_args()
    with open(gs.scene_path("bunny")) as f:
        doc = json.load(f)
    gs._merge(doc, gs.config_overrides(resolution=(a.resolution, a.resolution), spp=a.spp, depth=8))
    result = {"device": torch.cuda.get_device_name(0), "calls": a.calls, "resolution": a.resolution, "spp": a.spp, "builders": {}}
    with tempfile.TemporaryDirectory() as work:
        scenes = {deg: twisted_scene(doc, deg, work) for deg in a.angles}
        base = gs.load_scene_text(json.dumps(doc), gs.SCENE_DIR)
        few = _abi.gbl_render_setting.from_buffer_copy(base.desc.setting)
        few.sample_per_pixel = 4
        for bvh in ("host", "device"):
            rows = {}
            for deg in a.angles:
                sc = scenes[deg]
                assert sc.desc.num_triangles == base.desc.num_triangles and sc.desc.num_vertices == base.desc.num_vertices
                P = mesh_positions(sc, 0)
                edited = HipPathTracer(base, 0, bvh=bvh)
                edited.update_vertices(0, P)   # warm-up: the plan is built here
                update = [wall_ms(lambda: edited.update_vertices(0, P)) for _ in range(a.calls)]
                made = []
                create = [wall_ms(lambda: made.append(HipPathTracer(sc, 0, bvh=bvh))) for _ in range(3)]
                fresh = made[-1]
                del made[:-1]
                films = {"refit": edited.new_film(), "fresh": fresh.new_film()}
                kernel = {"refit": [], "fresh": []}
                for r in (edited, fresh):
                    r.render(schedule="megakernel")   # warm-up
                for _ in range(a.calls):
                    for key, r in (("refit", edited), ("fresh", fresh)):
                        kernel[key].append(r.render(film=films[key], timed=True, schedule="megakernel")["stats"]["kernel_ms"])
                counted = {key: r.render(setting=few, stats=True, schedule="megakernel")["stats"] for key, r in (("refit", edited), ("fresh", fresh))}
                same = torch.equal(edited.render(setting=few, want_li=True, exact_ties=True)["li"], fresh.render(setting=few, want_li=True, exact_ties=True)["li"])
                rows["%g" % deg] = {
                    "update_ms": statistics.median(update), "update_ms_min_max": [min(update), max(update)],
                    "create_ms": statistics.median(create), "create_build_ms": fresh.info.build_ms,
                    "kernel_ms_refit": statistics.median(kernel["refit"]), "kernel_ms_fresh": statistics.median(kernel["fresh"]),
                    "nodes_refit": counted["refit"]["nodes"], "nodes_fresh": counted["fresh"]["nodes"],
                    "tris_refit": counted["refit"]["tris"], "tris_fresh": counted["fresh"]["tris"],
                    "radiance_identical": bool(same)}
                del edited, fresh
            result["builders"][bvh] = rows
    print(json.dumps(result))


if __name__ == "__main__":
    main()
