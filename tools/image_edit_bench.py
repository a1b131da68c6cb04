#!/usr/bin/env python3
"""Cost of an image edit (gbl_update_image_device / gbl_update_image) against the only route there was before it: loading the
scene again, which builds the pyramid on the host (csrc/host/mipmap.cpp), and gbl_create of the result.

One quad under one image texture; the image is a 256 x 256 float image, then 1024 x 1024, 2048 x 1024 and 4096 x 2048 colour
images (drawn from a seed and written as EXR files into a scratch directory).  Per image:

    device   gbl_update_image_device from a tensor on the device: HIP events around --window-ms of calls back to back, the median
             of --calls such windows after --warm warm-up calls (as tools/query_bench.py times gbl_trace_rays)
    copy     the level-0 copy alone (a device-to-device copy of the same bytes, timed the same way): what is left of `device` is
             the level kernels and their launches, levels - 1 of them
    host     gbl_update_image from a numpy array: wall clock from the call to the end of a device synchronise, median of --calls
    reload   the scene loaded again from its files (wall clock; reads the EXR and builds the pyramid) and gbl_create of it with a
             device synchronise (wall clock), median of --reloads

and whether the edited pool equals the loader's, bit for bit.

    python tools/image_edit_bench.py [--out profiles/image_edit_bench.txt]
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
IMAGES = (("256x256 float", 256, 256, "float"), ("1024x1024 colour", 1024, 1024, "color"), ("2048x1024 colour", 2048, 1024, "color"),
          ("4096x2048 colour", 4096, 2048, "color"))


def document(kind):
    tex = {"format": kind, "name": "img", "type": "image", "file": "image.exr", "filter": "trilinear", "address": "repeat"}
    if kind == "float":
        tex.update(channel="R", gamma=1.0)
    kd = {"format": "color", "name": "white", "type": "constant", "color": [0.5, 0.5, 0.5]}
    material = {"name": "m", "type": "lambert", "Kd": "white", "bumpmap": "img"} if kind == "float" else {"name": "m", "type": "lambert", "Kd": "img"}
    return {"render_setting": {"render_method": "path_tracing", "sample_per_pixel": 1, "max_ray_depth": 2, "thread_num": 1},
            "camera": {"type": "perspective", "position": [0.0, 2.0, -2.9], "orientation": [0.9396926, 0.3420201, 0.0, 0.0], "fov": 52.0, "near_plane": 0.1,
                       "far_plane": 100.0, "film": {"resolution": [64, 64]}, "filter": {"type": "gaussian", "width": [2, 2], "falloff": 2.0}},
            "geometries": [{"name": "quad", "type": "mesh", "file": "plane.obj"}],
            "lights": [{"name": "lamp", "type": "point", "intensity": [14.0, 13.0, 12.0], "position": [-0.7, 2.4, -0.9]}],
            "textures": [kd, tex], "materials": [material],
            "primitives": [{"type": "model", "name": "model", "geometry": "quad", "material": "m"},
                           {"type": "instance", "name": "i", "model": "model", "position": [0, 0, 0], "orientation": [1, 0, 0, 0], "scale": [1, 1, 1]}]}


def resource_lines():
    """The pyramid kernel's registers, spills, scratch and LDS as tools/kernel_resources.py reads them from the library."""
    import subprocess
    rows = json.loads(subprocess.check_output([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "--json"]).decode())
    return ["%s: %d VGPRs, %d SGPRs, %d + %d spilled, %d B scratch, %d B LDS" % (
        r["name"], r.get("vgpr_count", -1), r.get("sgpr_count", -1), r.get("vgpr_spill_count", 0), r.get("sgpr_spill_count", 0),
        r.get("private_segment_fixed_size", 0), r.get("group_segment_fixed_size", 0)) for r in rows if "pyramid" in r["name"]]


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
    assert torch.cuda.is_available(), "image_edit_bench needs a HIP device"

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

    rows = []
    work = tempfile.mkdtemp(prefix="image_edit_bench_")
    try:
        shutil.copy(os.path.join(gs.SCENE_DIR, "models", "plane.obj"), os.path.join(work, "plane.obj"))
        for name, w, h, kind in IMAGES:
            rng = np.random.RandomState(w * 31 + h)
            img = np.ascontiguousarray(rng.randint(0, 32, (h, w, 3)).astype(np.float32) / np.float32(32.0))
            st = _abi.host_lib().gbl_host_write_exr(os.fsencode(os.path.join(work, "image.exr")), img.ctypes.data_as(C.c_void_p), w, h)
            assert st == _abi.GBL_OK, st
            text = json.dumps(document(kind))
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
            assert scene.desc.num_images == 1 and (im.width, im.height) == (w, h)
            pool = np.ctypeslib.as_array(scene.desc.texels, shape=(scene.desc.num_texels,))
            level0 = np.array(pool[:w * h * im.channels]).reshape(h, w, im.channels)
            # another level 0 first, so that the edit back to the file's has something to put right
            other = np.ascontiguousarray(level0[::-1, ::-1])
            r.update_image(0, torch.from_numpy(other).to(r.device))
            d_level0 = torch.from_numpy(level0).to(r.device)
            scratch = torch.empty_like(d_level0)
            device_ms = by_events(lambda: r.update_image(0, d_level0))
            copy_ms = by_events(lambda: scratch.copy_(d_level0))
            host_ms = by_wall(lambda: r.update_image(0, level0), a.calls)
            _, levels = r.image(0)
            same = np.array_equal(np.concatenate([l.ravel() for l in levels]).view(np.uint32), pool.view(np.uint32))
            rows.append(dict(name=name, levels=int(im.levels), mib=pool.nbytes / 2.0**20, device_ms=device_ms, copy_ms=copy_ms, host_ms=host_ms,
                             load_ms=statistics.median(loads), create_ms=statistics.median(creates), same=bool(same)))
            del r, kept
    finally:
        shutil.rmtree(work, True)
    lines = ["image edits on %s: one image texture on one quad" % torch.cuda.get_device_name(0),
             "device, copy: median of %d windows of %.0f ms of calls back to back (HIP events); host: wall clock to the end of a device synchronise, median of %d;" %
             (a.calls, a.window_ms, a.calls),
             "reload: wall clock of loading the scene again (EXR read, host pyramid) + gbl_create with a device synchronise, median of %d" % a.reloads, "",
             "%-18s %6s %9s %11s %11s %11s %11s %11s %11s %8s %6s" % ("image", "levels", "pool MiB", "device ms", "copy ms", "per launch", "host ms", "load ms",
                                                                   "create ms", "reload/dev", "bits")]
    for x in rows:
        launches = max(1, x["levels"] - 1)
        lines.append("%-18s %6d %9.2f %11.4f %11.4f %11.4f %11.3f %11.2f %11.2f %8.0f %6s" % (
            x["name"], x["levels"], x["mib"], x["device_ms"], x["copy_ms"], (x["device_ms"] - x["copy_ms"]) / launches, x["host_ms"], x["load_ms"], x["create_ms"],
            (x["load_ms"] + x["create_ms"]) / x["device_ms"], "same" if x["same"] else "DIFFER"))
    lines += ["", "per launch: (device - copy) / (levels - 1), the level kernels' time and launch cost per level",
              "fused tail levels, LDS staging of source tiles: not tried", ""] + resource_lines()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
        with open(os.path.splitext(a.out)[0] + ".json", "w") as f:
            json.dump(rows, f)
    if not all(x["same"] for x in rows):
        raise SystemExit("image_edit_bench: an edited pool differs from the loader's")


if __name__ == "__main__":
    main()
