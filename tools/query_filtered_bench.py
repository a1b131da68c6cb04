#!/usr/bin/env python3
"""Throughput of gbl_trace_rays_filtered against gbl_trace_rays on two mask scenes (host-built contexts):

    masked   the bundled masked.json: five mask instances (two cut-out quads, a tinted pane, a cut-out sphere, a ghost cube)
    cards    the bundled grid.json (ten bunnies on a floor) under --cards (256) mask quads at seeded places and angles over the
             grid, two thirds of them checkerboard cut-outs, the rest tinted panes of alpha 0.5

and two populations of 2^22 rays each (tools/query_bench.py's): `ao`, cosine-hemisphere rays of length 0.1 x scene radius from
the camera rays' hits, and `chords`, segments between uniform points of the scene bound.

For each: any-hit unfiltered (gbl_trace_rays), any-hit OPAQUE, closest-hit MASK, TRANSMITTANCE lean and exact -- by HIP events
around --window-ms (100 ms) of calls back to back, the median of --calls such windows after --warm warm-up calls; ms per call
and Grays/s.  Each scene is measured in a child process of its own, the two alternating, --rounds times; the table gives the
median over the runs and every run's own figure beside it.

    python tools/query_filtered_bench.py [--out table.txt] [--rounds 2] [--log2n 22]
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
SCENES = ("masked", "cards")
POPULATIONS = ("ao", "chords")
FORMS = (("any/none", dict(kind="any")), ("any/opaque", dict(kind="any", filter="opaque")), ("closest/mask", dict(kind="closest", filter="mask")),
         ("transmittance", dict(kind="transmittance")), ("transmittance/exact", dict(kind="transmittance", exact_ties=True)))


def cards_doc(n_cards, seed=4242):
    """grid.json with n_cards mask quads over the bunnies."""
    import numpy as np
    from goblin_amd import scene as gs
    with open(gs.scene_path("grid")) as f:
        doc = json.load(f)
    doc["textures"] += [{"format": "color", "name": "leaf_green", "type": "constant", "color": [0.15, 0.55, 0.12]},
                        {"format": "color", "name": "amber", "type": "constant", "color": [1.0, 0.75, 0.3]},
                        {"format": "float", "name": "zero", "type": "constant", "float": 0.0},
                        {"format": "float", "name": "one", "type": "constant", "float": 1.0},
                        {"format": "float", "name": "half", "type": "constant", "float": 0.5},
                        {"format": "float", "name": "cutout", "type": "checkerboard", "texture1": "one", "texture2": "zero", "scale": [5.0, 5.0]}]
    doc["materials"] += [{"name": "leaf_base", "type": "lambert", "Kd": "leaf_green"},
                         {"name": "leaf", "type": "mask", "material": "leaf_base", "alpha": "cutout"},
                         {"name": "pane", "type": "mask", "material": "leaf_base", "alpha": "half", "transparent_color": "amber"}]
    doc["primitives"] += [{"type": "model", "name": "m_leaf", "geometry": "plane", "material": "leaf"},
                          {"type": "model", "name": "m_pane", "geometry": "plane", "material": "pane"}]
    rng = np.random.default_rng(seed)
    for k in range(n_cards):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        pos = rng.uniform([-2.8, -1.0, -1.6], [2.8, 0.6, 1.6])
        size = float(rng.uniform(0.15, 0.35))
        doc["primitives"].append({"type": "instance", "name": "card_%d" % k, "model": "m_pane" if k % 3 == 2 else "m_leaf",
                                  "position": [float(v) for v in pos], "orientation": [float(v) for v in q], "scale": [size, size, size]})
    return doc


def child(a):
    import torch
    from goblin_amd import scene as gs
    from goblin_amd.renderer import HipPathTracer
    from query_bench import populations
    if a.scene == "cards":
        scene = gs.load_scene_text(json.dumps(cards_doc(a.cards)), gs.SCENE_DIR)
    else:
        scene = gs.load_scene("masked")
    r = HipPathTracer(scene, 0)
    n_side = 1 << (a.log2n // 2)
    pops, frac, radius = populations(torch, r, n_side)
    n = n_side * n_side
    res = {"scene": a.scene, "n": n, "device": torch.cuda.get_device_name(0), "instances": int(scene.desc.num_instances), "radius": radius, "ms": {}, "facts": {}}

    def window(fn, batch):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(batch):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / batch

    def timed(fn):
        for _ in range(a.warm):
            fn()
        torch.cuda.synchronize()
        batch = max(a.batch, min(4096, int(math.ceil(a.window_ms / max(1e-3, window(fn, a.batch))))))
        return statistics.median(window(fn, batch) for _ in range(a.calls))

    for name in POPULATIONS:
        rays = pops[name]
        outs = {"any": torch.empty((n,), dtype=torch.uint8, device=r.device), "closest": torch.empty((n, 8), dtype=torch.float32, device=r.device),
                "transmittance": torch.empty((n, 4), dtype=torch.float32, device=r.device)}
        for form, kw in FORMS:
            res["ms"]["%s/%s" % (name, form)] = timed(lambda: r.trace(rays, out=outs[kw["kind"]], **kw))
        # what the population meets: occluded fractions, mask hits, and the surfaces a clear segment crosses
        tr = r.trace(rays, kind="transmittance")
        res["facts"][name] = {"occluded_unfiltered": float(r.trace(rays, kind="any").float().mean()),
                              "occluded_opaque": float(tr["occluded"].float().mean()),
                              "hits_a_mask": float((r.trace(rays, filter="mask")["instance"] >= 0).float().mean()),
                              "crossed_mean_of_clear": float(tr["crossed"][~tr["occluded"]].float().mean()),
                              "crossed_max": int(tr["crossed"].max())}
    print("QUERY_FILTERED_BENCH " + json.dumps(res))


def grays(n, ms):
    return n / (ms * 1e-3) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--scene", default="masked", choices=SCENES)
    ap.add_argument("--cards", type=int, default=256)
    ap.add_argument("--log2n", type=int, default=22)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--window-ms", type=float, default=100.0)
    ap.add_argument("--warm", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    runs = {s: [] for s in SCENES}
    for _ in range(a.rounds):
        for scene in SCENES:   # alternating
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--scene", scene, "--cards", str(a.cards), "--log2n", str(a.log2n), "--calls", str(a.calls),
                   "--batch", str(a.batch), "--window-ms", str(a.window_ms), "--warm", str(a.warm)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=500)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("QUERY_FILTERED_BENCH ")]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit("query_filtered_bench: the run on %s failed (status %d)" % (scene, p.returncode))
            runs[scene].append(json.loads(line[0][len("QUERY_FILTERED_BENCH "):]))
    first = runs[SCENES[0]][0]
    n = first["n"]
    lines = ["gbl_trace_rays_filtered, host-built contexts, %d rays per population, %s" % (n, first["device"]),
             "median of %d windows of %.0f ms of calls back to back (HIP events) per run; %d runs per scene, the scenes alternating;" % (a.calls, a.window_ms, a.rounds),
             "ms per call (median of the runs) | Grays/s | each run's ms", ""]
    for scene in SCENES:
        rs = runs[scene]
        lines.append("%s (%d instances)" % (scene, rs[0]["instances"]))
        for name in POPULATIONS:
            f = rs[0]["facts"][name]
            lines.append("  %s: occluded unfiltered %.3f, occluded under OPAQUE %.3f, closest MASK hits %.3f, surfaces crossed by a clear segment: mean %.2f, most %d" %
                         (name, f["occluded_unfiltered"], f["occluded_opaque"], f["hits_a_mask"], f["crossed_mean_of_clear"], f["crossed_max"]))
            for form, _ in FORMS:
                key = "%s/%s" % (name, form)
                each = [r["ms"][key] for r in rs]
                ms = statistics.median(each)
                lines.append("    %-32s%10.3f |%7.2f | %s" % (key, ms, grays(n, ms), "  ".join("%.3f" % v for v in each)))
        lines.append("")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
        with open(os.path.splitext(a.out)[0] + ".json", "w") as f:
            json.dump(runs, f)


if __name__ == "__main__":
    main()
