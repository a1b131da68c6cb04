#!/usr/bin/env python3
"""Cost of an environment edit (gbl_update_environment_device / gbl_update_environment) against the only route there was before
it: loading the scene again, which builds the pyramid on the host, and gbl_create of the result, which packs the light's
distribution and power on the host and builds every BVH again.

One quad under an image based light and a point light; the environment is 256 x 128, 1024 x 512, 2048 x 1024 and 4096 x 2048
(drawn from a seed and written as an EXR file into a scratch directory).  Per size:

    device   gbl_update_environment_device from a tensor on the device: HIP events around --window-ms of calls back to back, the
             median of --calls such windows after --warm warm-up calls (as tools/image_edit_bench.py times the image edit)
    pyramid, dist, tail
             the same with GBL_ENVIRONMENT_PARTS (csrc/api_environment.hip) naming one part: the level-0 copy and the pyramid
             launches; func and the rows' CDFs; the tail launch with the power's 4-byte read-back
    host     gbl_update_environment from a numpy array: wall clock from the call to the end of a device synchronise, median of --calls
    reload   the scene loaded again from its files (wall clock) and gbl_create of it with a device synchronise (wall clock),
             median of --reloads

and whether the pyramid, the distribution and the pick tables after the edits equal the fresh context's, bit for bit.

    python tools/environment_edit_bench.py [--out profiles/environment_edit_bench.txt]
"""
import argparse
import ctypes as C
import json
import math
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
SIZES = ((256, 128), (1024, 512), (2048, 1024), (4096, 2048))
PARTS = (("pyramid", 1), ("dist", 2), ("tail", 4))


def document():
    return {"render_setting": {"render_method": "path_tracing", "sample_per_pixel": 1, "max_ray_depth": 2, "thread_num": 1},
            "camera": {"type": "perspective", "position": [0.0, 2.0, -2.9], "orientation": [0.9396926, 0.3420201, 0.0, 0.0], "fov": 52.0, "near_plane": 0.1,
                       "far_plane": 100.0, "film": {"resolution": [64, 64]}, "filter": {"type": "gaussian", "width": [2, 2], "falloff": 2.0}},
            "geometries": [{"name": "quad", "type": "mesh", "file": "plane.obj"}],
            "lights": [{"name": "sky", "type": "ibl", "file": "env.exr", "filter": [1.0, 0.95, 0.9], "orientation": [1.0, 0.0, 0.0, 0.0], "sample_num": 1},
                       {"name": "lamp", "type": "point", "intensity": [14.0, 13.0, 12.0], "position": [-0.7, 2.4, -0.9]}],
            "textures": [{"format": "color", "name": "white", "type": "constant", "color": [0.5, 0.5, 0.5]}],
            "materials": [{"name": "m", "type": "lambert", "Kd": "white"}],
            "primitives": [{"type": "model", "name": "model", "geometry": "quad", "material": "m"},
                           {"type": "instance", "name": "i", "model": "model", "position": [0, 0, 0], "orientation": [1, 0, 0, 0], "scale": [1, 1, 1]}]}


def resource_lines():
    """The kernels' registers, spills, scratch and LDS as tools/kernel_resources.py reads them from the library."""
    import subprocess
    rows = json.loads(subprocess.check_output([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "--json"]).decode())
    return ["%s: %d VGPRs, %d SGPRs, %d + %d spilled, %d B scratch, %d B LDS" % (
        r["name"], r.get("vgpr_count", -1), r.get("sgpr_count", -1), r.get("vgpr_spill_count", 0), r.get("sgpr_spill_count", 0),
        r.get("private_segment_fixed_size", 0), r.get("group_segment_fixed_size", 0)) for r in rows if "environment" in r["name"] or "pyramid" in r["name"]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--window-ms", type=float, default=100.0)
    ap.add_argument("--warm", type=int, default=4)
    ap.add_argument("--reloads", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from goblin_amd import _abi
    from goblin_amd import scene as gs
    from goblin_amd.renderer import HipPathTracer
    assert torch.cuda.is_available(), "environment_edit_bench needs a HIP device"
    parts = list(PARTS)

    def window(fn, batch):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(batch):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / batch

    def by_events(fn):
        for _ in range(a.warm):
            fn()
        torch.cuda.synchronize()
        batch = max(a.batch, min(4096, int(math.ceil(a.window_ms / max(1e-3, window(fn, a.batch))))))
        return statistics.median(window(fn, batch) for _ in range(a.calls))

    def by_wall(fn, times):
        ms = []
        for _ in range(times):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ms)

    def tables(r):
        t = r._lights_raw()
        return np.concatenate([np.concatenate([l.ravel() for l in r.image(0)[1]]), r._environment_raw(0)["dist"], t["cdf"], t["pick_pdf"]]).view(np.uint32)

    rows = []
    work = tempfile.mkdtemp(prefix="environment_edit_bench_")
    try:
        shutil.copy(os.path.join(gs.SCENE_DIR, "models", "plane.obj"), os.path.join(work, "plane.obj"))
        text = json.dumps(document())
        for w, h in SIZES:
            rng = np.random.RandomState(w * 31 + h)
            img = np.ascontiguousarray(rng.randint(1, 33, (h, w, 3)).astype(np.float32) / np.float32(32.0))
            st = _abi.host_lib().gbl_host_write_exr(os.fsencode(os.path.join(work, "env.exr")), img.ctypes.data_as(C.c_void_p), w, h)
            assert st == _abi.GBL_OK, st
            loads, creates, kept = [], [], None
            for _ in range(a.reloads):
                t0 = time.perf_counter()
                scene = gs.load_scene_text(text, work)
                loads.append((time.perf_counter() - t0) * 1e3)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = HipPathTracer(scene, 0)
                torch.cuda.synchronize()
                creates.append((time.perf_counter() - t0) * 1e3)
                kept = (scene, r)
            scene, r = kept
            im = scene.desc.images[0]
            assert scene.desc.num_images == 1 and (im.width, im.height, im.channels) == (w, h, 4)
            fresh = tables(r)
            pool = np.ctypeslib.as_array(scene.desc.texels, shape=(scene.desc.num_texels,))
            level0 = np.array(pool[:w * h * 4]).reshape(h, w, 4)
            # another level 0 first, so that the edit back to the file's has something to put right
            r.update_environment(0, torch.from_numpy(np.ascontiguousarray(level0[::-1, ::-1])).to(r.device))
            assert not np.array_equal(tables(r), fresh)
            d_level0 = torch.from_numpy(level0).to(r.device)
            x = dict(name="%dx%d" % (w, h), levels=int(im.levels), dist="%dx%d" % (r._environment_raw(0)["dist_w"], r._environment_raw(0)["dist_h"]),
                     mib=pool.nbytes / 2.0**20)
            x["device_ms"] = by_events(lambda: r.update_environment(0, d_level0))
            for name, mask in parts:
                os.environ["GBL_ENVIRONMENT_PARTS"] = str(mask)
                try:
                    x[name + "_ms"] = by_events(lambda: r.update_environment(0, d_level0))
                finally:
                    del os.environ["GBL_ENVIRONMENT_PARTS"]
            x["host_ms"] = by_wall(lambda: r.update_environment(0, level0), a.calls)
            x["same"] = bool(np.array_equal(tables(r), fresh))
            x["load_ms"], x["create_ms"] = statistics.median(loads), statistics.median(creates)
            rows.append(x)
            del r, kept
    finally:
        shutil.rmtree(work, True)
    names = [n for n, _ in parts]
    lines = ["environment edits on %s: one image based light and a point light over one quad" % torch.cuda.get_device_name(0),
             "device and its parts: median of %d windows of %.0f ms of calls back to back (HIP events); host: wall clock to the end of a device synchronise, median of %d;" %
             (a.calls, a.window_ms, a.calls),
             "reload: wall clock of loading the scene again (EXR read, host pyramid) + gbl_create with a device synchronise, median of %d" % a.reloads, "",
             ("%-10s %6s %8s %9s %10s" + " %10s" * len(names) + " %10s %10s %10s %10s %6s") % (
                 ("size", "levels", "dist", "pool MiB", "device ms") + tuple(n + " ms" for n in names) + ("host ms", "load ms", "create ms", "reload/dev", "bits"))]
    for x in rows:
        lines.append(("%-10s %6d %8s %9.2f %10.4f" + " %10.4f" * len(names) + " %10.3f %10.2f %10.2f %10.0f %6s") % (
            (x["name"], x["levels"], x["dist"], x["mib"], x["device_ms"]) + tuple(x[n + "_ms"] for n in names) +
            (x["host_ms"], x["load_ms"], x["create_ms"], (x["load_ms"] + x["create_ms"]) / x["device_ms"], "same" if x["same"] else "DIFFER")))
    lines += ["", "pyramid: the level-0 copy and levels - 1 launches; dist: func and the rows' CDFs (two launches); tail: one launch and a 4-byte copy", ""] + resource_lines()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
        with open(os.path.splitext(a.out)[0] + ".json", "w") as f:
            json.dump(rows, f)
    if not all(x["same"] for x in rows):
        raise SystemExit("environment_edit_bench: the edited tables differ from the fresh context's")


if __name__ == "__main__":
    main()
