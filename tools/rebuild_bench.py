#!/usr/bin/env python3
"""What rebuilding a deformed mesh's tree costs and what it buys.  tools/refit_bench.py's scene:
bunny.json's bunny (69 120 triangles) twisted about its vertical axis by --angles degrees over the mesh's height.  For both
builders of the edited context and every angle, three trees over the same positions -- `refit` (update_vertices only),
`rebuilt` (update_vertices, then rebuild_mesh) and `fresh` (a device-built context of the twisted scene):

  rebuild_ms   wall time of rebuild_mesh: the median of --calls calls after one warm-up (which makes the slot and the scratch;
               the call synchronises the device), beside the fresh context's gbl_info.build_ms;
  first_ms     the wall time of that first call, which allocates;
  kernel_ms    of a render (--resolution, --spp) on each tree, the median of --calls, the three alternating;
  nodes, tris  the traversal counters of a collect_stats render (4 spp) on each tree;
  node_cost, tri_cost   tree_stats' two ratios of each tree;
  break_even   renders after which the rebuild has paid: rebuild_ms / (kernel_ms_refit - kernel_ms_rebuilt), null if the
               rebuilt tree is not faster;
  and whether the rebuilt and the fresh tree's per-sample radiance is the same tensor, with and without exact_ties.

Prints one JSON line.

    python tools/rebuild_bench.py [--angles 0 5 20 60] [--calls 7] [--resolution 512] [--spp 16]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from goblin_amd import _abi  # noqa: E402
from goblin_amd import scene as gs  # noqa: E402
from goblin_amd.renderer import HipPathTracer  # noqa: E402
from refit_bench import mesh_positions, twisted_scene, wall_ms  # noqa: E402

TREES = ("refit", "rebuilt", "fresh")


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
                r = {"refit": HipPathTracer(base, 0, bvh=bvh), "rebuilt": HipPathTracer(base, 0, bvh=bvh), "fresh": HipPathTracer(sc, 0, bvh="device")}
                r["refit"].update_vertices(0, P)
                r["rebuilt"].update_vertices(0, P)
                first = wall_ms(lambda: r["rebuilt"].rebuild_mesh(0))
                rebuild = [wall_ms(lambda: r["rebuilt"].rebuild_mesh(0)) for _ in range(a.calls)]
                films = {k: r[k].new_film() for k in TREES}
                kernel = {k: [] for k in TREES}
                for k in TREES:
                    r[k].render(schedule="megakernel")   # warm-up
                for _ in range(a.calls):
                    for k in TREES:
                        kernel[k].append(r[k].render(film=films[k], timed=True, schedule="megakernel")["stats"]["kernel_ms"])
                counted = {k: r[k].render(setting=few, stats=True, schedule="megakernel")["stats"] for k in TREES}
                cost = {k: r[k].tree_stats(0) for k in TREES}
                same = {"exact_ties": torch.equal(r["rebuilt"].render(setting=few, want_li=True, exact_ties=True)["li"],
                                                  r["fresh"].render(setting=few, want_li=True, exact_ties=True)["li"]),
                        "lean": torch.equal(r["rebuilt"].render(setting=few, want_li=True)["li"], r["fresh"].render(setting=few, want_li=True)["li"])}
                row = {"rebuild_ms": statistics.median(rebuild), "rebuild_ms_min_max": [min(rebuild), max(rebuild)], "first_ms": first,
                       "fresh_build_ms": r["fresh"].info.build_ms, "radiance_identical": {k: bool(v) for k, v in same.items()}}
                for k in TREES:
                    row["kernel_ms_" + k] = statistics.median(kernel[k])
                    row["nodes_" + k], row["tris_" + k] = counted[k]["nodes"], counted[k]["tris"]
                    row["node_cost_" + k], row["tri_cost_" + k] = cost[k]["node_cost"], cost[k]["tri_cost"]
                    row["tree_nodes_" + k] = cost[k]["nodes"]
                gain = row["kernel_ms_refit"] - row["kernel_ms_rebuilt"]
                row["break_even_renders"] = row["rebuild_ms"] / gain if gain > 0 else None
                rows["%g" % deg] = row
                del r
            result["builders"][bvh] = rows
    print(json.dumps(result))


if __name__ == "__main__":
    main()
