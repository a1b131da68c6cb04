#!/usr/bin/env python3
"""What an instance edit costs through the host entry and through the device entry, and what the device-built TLAS costs to
trace.  Scenes of --counts instances of tests/meshes.py's few5 on a seeded jittered grid; every edit
moves all of them (two seeded sets of transforms alternate).  In one process, after a warm-up of every kind, alternating, each
window closed by a device synchronise, medians with min and max over --edits edits each:

  list_ms            update_instances(list of tuples): the Python face of gbl_update_instances, marshalling included
  host_entry_ms      gbl_update_instances itself, its gbl_trs array prepared beforehand (the yardstick for the entries)
  device_host_ms     gbl_update_instances_device, flags 0: compose on the device, TLAS on the host
  device_device_ms   ... with GBL_INSTANCES_DEVICE_TLAS: TLAS on the device
  render_host_ms     a --resolution x --spp megakernel render on the host-built TLAS of a set of transforms, and
  render_device_ms   on the device-built TLAS of the same set; --renders each, in alternating groups of three
  breakeven_renders  (host_entry_ms - device_device_ms) / (render_device_ms - render_host_ms): renders per edit above which
                     the host-built tree is the cheaper frame; null when the device tree does not trace slower

Prints one JSON line and, with --out, writes it there.

    python tools/instances_ab.py [--counts 300 10000 100000] [--edits 20] [--renders 9] [--resolution 512] [--spp 16] [--out FILE]
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import meshes  # noqa: E402
from goblin_amd import _abi  # noqa: E402
from goblin_amd import scene as gs  # noqa: E402
from goblin_amd.renderer import HipPathTracer  # noqa: E402
from refit_bench import wall_ms  # noqa: E402

PITCH, SCALE = 1.0, 0.3


def grid_rows(n, seed):
    """n transforms on a jittered square grid in the plane y = 0: (n, 10) float32 rows of gbl_trs."""
    rng = np.random.default_rng(seed)
    side = int(math.ceil(math.sqrt(n)))
    k = np.arange(n)
    T = np.zeros((n, 10), np.float32)
    T[:, 0] = PITCH * (k % side - 0.5 * (side - 1) + 0.35 * rng.uniform(-1, 1, n))
    T[:, 1] = 0.25 * PITCH * rng.uniform(-1, 1, n)
    T[:, 2] = PITCH * (k // side - 0.5 * (side - 1) + 0.35 * rng.uniform(-1, 1, n))
    T[:, 3:7] = np.array(meshes.TILT, np.float32)
    T[:, 7:] = (SCALE * (1.0 + 0.3 * rng.uniform(-1, 1, n)))[:, None]
    return T


def tuples(T):
    return [(tuple(map(float, r[:3])), tuple(map(float, r[3:7])), tuple(map(float, r[7:]))) for r in T]


def grid_doc(n, T, resolution, spp):
    side = int(math.ceil(math.sqrt(n)))
    half = 0.5 * PITCH * side + 1.0
    doc = meshes._base_doc([0, 0, 0], 0.5 * half, -1.0, half, None, (resolution, resolution), spp, 5, None)
    doc["geometries"].append({"name": "few5", "type": "mesh", "file": "few5.obj"})
    doc["primitives"].append({"type": "model", "name": "m0", "geometry": "few5", "material": "white"})
    doc["primitives"].append({"type": "model", "name": "m1", "geometry": "few5", "material": "glass"})
    for k, (pos, quat, scale) in enumerate(tuples(T)):
        doc["primitives"].append({"type": "instance", "name": "i%d" % k, "model": "m%d" % (k % 2), "position": list(pos), "orientation": list(quat),
                                  "scale": list(scale)})
    return doc


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def measure(n, a, scene_dir):
    sets = [grid_rows(n, 1000 + n), grid_rows(n, 2000 + n)]
    scene = gs.load_scene_text(json.dumps(grid_doc(n, sets[0], a.resolution, a.spp)), scene_dir)
    r = HipPathTracer(scene, 0)
    lists = [tuples(T) for T in sets]
    tensors = [torch.from_numpy(T).to(r.device) for T in sets]
    arrays = []
    for T in sets:
        arr = (_abi.gbl_trs * n)()
        C.memmove(arr, np.ascontiguousarray(T).ctypes.data, T.nbytes)
        arrays.append(arr)

    def host_entry(s):
        st = r.lib.gbl_update_instances(r.handle, 1, n, arrays[s])
        assert st == _abi.GBL_OK, r.lib.gbl_last_error(r.handle).decode()
    kinds = {"list_ms": lambda s: r.update_instances(1, lists[s]), "host_entry_ms": host_entry,
             "device_host_ms": lambda s: r.update_instances(1, tensors[s]), "device_device_ms": lambda s: r.update_instances(1, tensors[s], device_tlas=True)}
    film = r.new_film()
    render = lambda: r.render(film=film, schedule="megakernel")   # noqa: E731
    for fn in kinds.values():   # warm-up: the tables, the kernels' code objects, the scratch
        fn(1)
        fn(0)
    render()
    t = {k: [] for k in kinds}
    s = 0
    for _ in range(a.edits):
        for k, fn in kinds.items():
            s ^= 1
            t[k].append(wall_ms(lambda: fn(s)))
    info = {}
    renders = {"render_host_ms": [], "render_device_ms": []}
    while len(renders["render_host_ms"]) < a.renders:
        for key, device_tlas in (("render_host_ms", False), ("render_device_ms", True)):
            r.update_instances(1, tensors[0], device_tlas=device_tlas)
            info[key] = {"tlas_nodes": int(r.info.tlas_nodes), "tlas_depth": int(r.info.tlas_depth), "stack_entries": r._instances_raw(0, 0)["stack_entries"]}
            render()
            renders[key] += [wall_ms(render) for _ in range(3)]
    row = {k: spread(v) for k, v in t.items()}
    row.update({k: spread(v) for k, v in renders.items()})
    row["tlas"] = info
    saved = row["host_entry_ms"]["median"] - row["device_device_ms"]["median"]
    slower = row["render_device_ms"]["median"] - row["render_host_ms"]["median"]
    row["breakeven_renders"] = saved / slower if slower > 0 and saved > 0 else None
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", type=int, nargs="+", default=[300, 10000, 100000])
    ap.add_argument("--edits", type=int, default=20)
    ap.add_argument("--renders", type=int, default=9)
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--out")
    a = ap.parse_args()
    result = {"device": torch.cuda.get_device_name(0), "edits": a.edits, "resolution": a.resolution, "spp": a.spp, "mesh": "few5", "counts": {}}
    with tempfile.TemporaryDirectory() as d:
        meshes.write_meshes(d, ["few5"])
        for n in a.counts:
            result["counts"][str(n)] = measure(n, a, d)
            print("instances %d: %s" % (n, json.dumps(result["counts"][str(n)])), file=sys.stderr, flush=True)
    text = json.dumps(result)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
