#!/usr/bin/env python3
"""Cost of a material or texture edit (gbl_update_materials*, gbl_update_textures*) against the only route there was before
them: loading the scene again and gbl_create of the result.

Two scenes: the bundled cornell (7 materials, no texture) and a generated one -- one quad per material over a lamp, N lambert
materials (--materials, 10000) whose Kd is a constant texture behind a scale node, so the texture table is about 3 N records.
Per scene and per table, for one record and for the whole table in one call:

    stream   the device form from a tensor on the device: HIP events around --window-ms of calls back to back, the median of
             --calls such windows after --warm warm-up calls (as tools/image_edit_bench.py times gbl_update_image_device): what
             an edit takes of the stream
    device   the device form's call, wall clock from the call to the end of a device synchronise, median of --calls
    host     the host form from records, on the same clock
    d call, h call   either form's call alone (wall clock until it returns; nothing is waited for), median of --calls windows of
             --batch: what an edit takes of the calling thread
    reload   the scene loaded again from its text (wall clock) and gbl_create of it with a device synchronise (wall clock),
             median of --reloads

and whether the tables after the last edit equal those of a fresh context, byte for byte.

    python tools/material_edit_bench.py [--out profiles/material_edit_bench.txt]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def generated(n):
    """N quads in a row under one lamp, one lambert material each: Kd = scale(constant colour, constant float)."""
    textures, materials, primitives = [], [], []
    for i in range(n):
        c = [0.2 + 0.6 * ((i * 37) % 101) / 100.0, 0.2 + 0.6 * ((i * 53) % 103) / 102.0, 0.2 + 0.6 * ((i * 71) % 107) / 106.0]
        textures += [{"format": "color", "name": "c%d" % i, "type": "constant", "color": c},
                     {"format": "float", "name": "f%d" % i, "type": "constant", "float": 0.5 + 0.5 * ((i * 13) % 17) / 16.0},
                     {"format": "color", "name": "s%d" % i, "type": "scale", "texture": "c%d" % i, "scale": "f%d" % i}]
        materials.append({"name": "m%d" % i, "type": "lambert", "Kd": "s%d" % i})
        primitives += [{"type": "model", "name": "model%d" % i, "geometry": "quad", "material": "m%d" % i},
                       {"type": "instance", "name": "i%d" % i, "model": "model%d" % i, "position": [2.5 * (i % 100) - 125.0, 0, 2.5 * (i // 100)],
                        "orientation": [1, 0, 0, 0], "scale": [1, 1, 1]}]
    return {"render_setting": {"render_method": "path_tracing", "sample_per_pixel": 1, "max_ray_depth": 2, "thread_num": 1},
            "camera": {"type": "perspective", "position": [0.0, 40.0, -30.0], "orientation": [0.9396926, 0.3420201, 0.0, 0.0], "fov": 52.0, "near_plane": 0.1,
                       "far_plane": 1000.0, "film": {"resolution": [64, 64]}, "filter": {"type": "gaussian", "width": [2, 2], "falloff": 2.0}},
            "geometries": [{"name": "quad", "type": "mesh", "file": "plane.obj"}],
            "lights": [{"name": "lamp", "type": "point", "intensity": [4000.0, 4000.0, 4000.0], "position": [0.0, 30.0, 100.0]}],
            "textures": textures, "materials": materials, "primitives": primitives}


def resource_lines():
    """The compose kernels' registers, spills, scratch and LDS as tools/kernel_resources.py reads them from the library."""
    import subprocess
    rows = json.loads(subprocess.check_output([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "--all", "--json"]).decode())
    return ["%s: %d VGPRs, %d SGPRs, %d + %d spilled, %d B scratch, %d B LDS" % (
        r["name"], r.get("vgpr_count", -1), r.get("sgpr_count", -1), r.get("vgpr_spill_count", 0), r.get("sgpr_spill_count", 0),
        r.get("private_segment_fixed_size", 0), r.get("group_segment_fixed_size", 0)) for r in rows if "mat_compose" in r["name"] or "tex_compose" in r["name"]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--materials", type=int, default=10000)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--window-ms", type=float, default=50.0)
    ap.add_argument("--warm", type=int, default=4)
    ap.add_argument("--reloads", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from goblin_amd import scene as gs
    from goblin_amd.renderer import HipPathTracer
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import material_edit_cases as mc
    assert torch.cuda.is_available(), "material_edit_bench needs a HIP device"

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

    def queue_only(fn):
        ms = []
        for _ in range(a.calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.batch):
                fn()
            ms.append((time.perf_counter() - t0) * 1e3 / a.batch)
        torch.cuda.synchronize()
        return statistics.median(ms)

    def fresh(name, text):
        loads, creates, kept = [], [], None
        for _ in range(a.reloads):
            t0 = time.perf_counter()
            scene = gs.load_scene(name, gs.config_overrides(resolution=(64, 64), spp=1, depth=2)) if text is None else gs.load_scene_text(text, os.path.join(gs.SCENE_DIR, "models"))
            loads.append((time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = HipPathTracer(scene, 0)
            torch.cuda.synchronize()
            creates.append((time.perf_counter() - t0) * 1e3)
            kept = (scene, r)
        return kept + (statistics.median(loads), statistics.median(creates))

    rows = []
    for name, text in (("cornell", None), ("generated %d" % a.materials, json.dumps(generated(a.materials)))):
        scene, r, load_ms, create_ms = fresh("cornell", text)
        other_r = HipPathTracer(scene, 0)   # never edited: the edits below write the description's own values
        M, T = mc.records(scene)
        for table, recs, update, host_fn, dev_fn, rows_of in (
                ("materials", M, r.update_materials, r.lib.gbl_update_materials, r.lib.gbl_update_materials_device, mc.material_rows),
                ("textures", T, r.update_textures, r.lib.gbl_update_textures, r.lib.gbl_update_textures_device, mc.texture_rows)):
            n = len(recs)
            if n == 0:
                continue
            for what, first, count in (("one record", n // 2, 1), ("whole table", 0, n)):
                part = recs[first:first + count]
                d_rows = torch.tensor(rows_of(part), dtype=torch.float32, device=r.device).reshape(count, -1)
                update(first, d_rows)   # (the first device edit makes the row table)
                ptr = d_rows.data_ptr()
                stream_ms = by_events(lambda: dev_fn(r.handle, first, count, ptr, None))
                device_ms = by_wall(lambda: dev_fn(r.handle, first, count, ptr, None), a.calls)
                dcall_ms = queue_only(lambda: dev_fn(r.handle, first, count, ptr, None))
                arr = (type(part[0]) * count)(*part)   # (made once: the call is timed, not ctypes)
                host_ms = by_wall(lambda: host_fn(r.handle, first, count, arr, None), a.calls)
                queue_ms = queue_only(lambda: host_fn(r.handle, first, count, arr, None))
                rows.append(dict(scene=name, table=table, what=what, records=count, stream_ms=stream_ms, device_ms=device_ms, dcall_ms=dcall_ms, host_ms=host_ms, queue_ms=queue_ms, load_ms=load_ms,
                                 create_ms=create_ms))
        got, want = r._materials_raw(), other_r._materials_raw()
        same = got["materials"].tobytes() == want["materials"].tobytes() and got["textures"].tobytes() == want["textures"].tobytes()
        for x in rows:
            if x["scene"] == name:
                x["same"] = bool(same)
        del r, other_r
    lines = ["material and texture edits on %s" % torch.cuda.get_device_name(0),
             "stream: the device form, median of %d windows of %.0f ms of calls back to back (HIP events); device, host: either form's call, wall clock to the end of a" %
             (a.calls, a.window_ms),
             "device synchronise, median of %d; d call, h call: the call alone, wall clock, median of %d windows of %d calls; reload: loading the scene again +" % (a.calls, a.calls, a.batch),
             "gbl_create with a device synchronise (wall clock), median of %d" % a.reloads, "",
             "%-16s %-10s %-12s %8s %10s %10s %10s %10s %10s %10s %10s %11s %6s %6s" % ("scene", "table", "edit", "records", "stream ms", "device ms", "host ms", "d call ms",
                                                                                    "h call ms", "load ms", "create ms", "reload/best", "wins", "bits")]
    for x in rows:
        best = min(x["device_ms"], x["host_ms"])
        lines.append("%-16s %-10s %-12s %8d %10.4f %10.4f %10.4f %10.4f %10.4f %10.2f %10.2f %11.0f %6s %6s" % (
            x["scene"], x["table"], x["what"], x["records"], x["stream_ms"], x["device_ms"], x["host_ms"], x["dcall_ms"], x["queue_ms"], x["load_ms"], x["create_ms"],
            (x["load_ms"] + x["create_ms"]) / best, "device" if x["device_ms"] < x["host_ms"] else "host", "same" if x["same"] else "DIFFER"))
    lines += ["", "wins: the smaller of device ms and host ms, which are one clock (the host form's rows lie in host memory already, the device form's in device memory).", ""] + resource_lines()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
        with open(os.path.splitext(a.out)[0] + ".json", "w") as f:
            json.dump(rows, f)
    if not all(x["same"] for x in rows):
        raise SystemExit("material_edit_bench: the edited tables differ from a fresh context's")


if __name__ == "__main__":
    main()
