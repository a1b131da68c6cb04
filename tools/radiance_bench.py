#!/usr/bin/env python3
"""Throughput of gbl_radiance_rays on the bundled bunny scene (host-built context) at max_ray_depth 8, two populations:

    camera   the rays of a 512 x 512 x 16 spp frame of the scene's own camera -- pixel-major, the 16 samples of a pixel jittered in
             its 4 x 4 sub-cells, so ray i is sample i % 16 of group i // 16 as a camera sample is of its pixel -- against gbl_render
             of that frame with per-sample radiance (li_out) under schedule="megakernel".  The same distribution of paths; the
             render path has the primary pass and the quad loops, this call has neither, so it is expected to lose: the ratio is
             a limit of the call, stated, not a failure.
    probes   4096 probes x 256 cosine-distributed directions about the surface normal, from surface points found with
             tracer.trace (tools/query_bench.py's camera rays), samples_per_group=256: a probe is a group.

By HIP events around --window-ms (200 ms) of calls back to back, the median of --calls such windows after --warm warm-up calls; each
run in a child process of its own, --rounds runs: ms per call and Mpaths/s, the median over the runs and every run's figure.

    python tools/radiance_bench.py [--out profiles/radiance_bench.txt] [--rounds 2]
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
SIDE, SPP, DEPTH = 512, 16, 8
PROBES, DIRECTIONS = 4096, 256


def camera_rays(torch, r):
    """(SIDE * SIDE * SPP, 8) rays of the pinhole camera, pixel-major, sample k of a pixel in sub-cell k of its 4 x 4 grid."""
    from query_bench import rotate
    dev = r.device
    cam = r.camera()
    q = [float(x) for x in cam.orientation]
    fwd, right, up = (rotate(torch, q, v).to(dev) for v in ((0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)))
    tan_half = math.tan(math.radians(float(cam.fov_degrees)) * 0.5)
    root = int(math.isqrt(SPP))
    gen = torch.Generator(device=dev)
    gen.manual_seed(4711)
    p = torch.arange(SIDE * SIDE, device=dev)
    k = torch.arange(SPP, device=dev)
    jit = torch.rand((SIDE * SIDE, SPP, 2), device=dev, generator=gen, dtype=torch.float64)
    x = ((p % SIDE)[:, None] + ((k % root)[None] + jit[..., 0]) / root).reshape(-1, 1) / SIDE
    y = ((p // SIDE)[:, None] + ((k // root)[None] + jit[..., 1]) / root).reshape(-1, 1) / SIDE
    d = fwd[None] + ((2.0 * x - 1.0) * tan_half) * right[None] + ((1.0 - 2.0 * y) * tan_half) * up[None]
    d = (d / d.norm(dim=1, keepdim=True)).float()
    d = d / d.norm(dim=1, keepdim=True)   # (unit in float32 to a few 1e-8)
    rays = torch.zeros((d.shape[0], 8), dtype=torch.float32, device=dev)
    rays[:, 0:3] = torch.tensor([float(v) for v in cam.position], device=dev)
    rays[:, 3], rays[:, 4:7], rays[:, 7] = 1e-3, d, float("inf")
    return rays


def probe_rays(torch, r):
    """(PROBES * DIRECTIONS, 8): probe g at a surface point a camera ray found, its DIRECTIONS rays cosine-distributed about the normal."""
    from query_bench import populations
    dev = r.device
    pops, _, radius = populations(torch, r, 256)
    primary = pops["primary"]
    hits = r.trace(primary, normals=True)
    idx = torch.nonzero(hits["instance"] >= 0).reshape(-1)
    idx = idx[(torch.arange(PROBES, device=dev) * max(1, idx.numel() // PROBES)) % idx.numel()]
    o = primary[idx, 0:3] + hits["t"][idx, None] * primary[idx, 4:7]
    nrm = hits["normal"][idx]
    nrm = torch.where((nrm * primary[idx, 4:7]).sum(dim=1, keepdim=True) > 0, -nrm, nrm)
    o, nrm = o.repeat_interleave(DIRECTIONS, dim=0), nrm.repeat_interleave(DIRECTIONS, dim=0)
    n = PROBES * DIRECTIONS
    gen = torch.Generator(device=dev)
    gen.manual_seed(4712)
    u = torch.rand((n, 2), device=dev, generator=gen)
    rad, phi = u[:, 0].sqrt(), 2.0 * math.pi * u[:, 1]
    a = torch.where(nrm[:, 0:1].abs() > 0.9, torch.tensor([0.0, 1.0, 0.0], device=dev), torch.tensor([1.0, 0.0, 0.0], device=dev)).expand(n, 3)
    t1 = torch.linalg.cross(nrm, a)
    t1 = t1 / t1.norm(dim=1, keepdim=True)
    t2 = torch.linalg.cross(nrm, t1)
    d = (rad * phi.cos())[:, None] * t1 + (rad * phi.sin())[:, None] * t2 + (1.0 - u[:, 0]).clamp_min(0).sqrt()[:, None] * nrm
    d = d / d.norm(dim=1, keepdim=True)
    rays = torch.zeros((n, 8), dtype=torch.float32, device=dev)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = o, 1e-3 * radius, d, float("inf")
    return rays.contiguous()


def child(a):
    import torch
    from goblin_amd import scene as gs
    from goblin_amd.renderer import HipPathTracer
    r = HipPathTracer(gs.load_scene("bunny", gs.config_overrides(resolution=(SIDE, SIDE), spp=SPP, depth=DEPTH)), 0)

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
        batch = max(1, min(4096, int(math.ceil(a.window_ms / max(1e-3, window(fn, 1))))))
        return statistics.median(window(fn, batch) for _ in range(a.calls))

    cam, probes = camera_rays(torch, r), probe_rays(torch, r)
    out_c = torch.empty((cam.shape[0], 4), dtype=torch.float32, device=r.device)
    out_p = torch.empty((probes.shape[0], 4), dtype=torch.float32, device=r.device)
    film = r.new_film()
    w = r.window
    res = {"device": torch.cuda.get_device_name(0), "n": {"camera": int(cam.shape[0]), "probes": int(probes.shape[0]),
                                                          "render": (w[1] - w[0]) * (w[3] - w[2]) * SPP}, "ms": {}}
    res["ms"]["camera"] = timed(lambda: r.radiance(cam, depth=DEPTH, seed=1, samples_per_group=SPP, out=out_c))
    res["ms"]["camera/exact"] = timed(lambda: r.radiance(cam, depth=DEPTH, seed=1, samples_per_group=SPP, exact_ties=True, out=out_c))
    res["ms"]["render"] = timed(lambda: r.render(film=film, seed=1, want_li=True, schedule="megakernel"))
    res["ms"]["probes"] = timed(lambda: r.radiance(probes, depth=DEPTH, seed=1, samples_per_group=DIRECTIONS, out=out_p))
    res["mean"] = {"camera": float(out_c[:, :3].nan_to_num().mean()), "probes": float(out_p[:, :3].nan_to_num().mean()),
                   "camera_hit_fraction": float((r.trace(cam[::SPP].contiguous())["instance"] >= 0).float().mean())}
    print("RADIANCE_BENCH " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    runs = []
    for _ in range(a.rounds):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--calls", str(a.calls), "--window-ms", str(a.window_ms), "--warm", str(a.warm)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=400)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RADIANCE_BENCH ")]
        if p.returncode != 0 or not line:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit("radiance_bench: a run failed (status %d)" % p.returncode)
        runs.append(json.loads(line[0][len("RADIANCE_BENCH "):]))
    first = runs[0]
    lines = ["gbl_radiance_rays, bunny, host-built context, max_ray_depth %d, %s" % (DEPTH, first["device"]),
             "median of %d windows of %.0f ms of calls back to back (HIP events) per run; %d runs" % (a.calls, a.window_ms, a.rounds),
             "camera: %d rays (%d x %d x %d spp, hit fraction %.3f); render: gbl_render with li_out, megakernel, %d camera samples (the sample window);"
             " probes: %d x %d" % (first["n"]["camera"], SIDE, SIDE, SPP, first["mean"]["camera_hit_fraction"], first["n"]["render"], PROBES, DIRECTIONS),
             "ms per call (median of the runs) | Mpaths/s | each run's ms", ""]
    for key, count in (("camera", "camera"), ("camera/exact", "camera"), ("render", "render"), ("probes", "probes")):
        each = [r["ms"][key] for r in runs]
        ms = statistics.median(each)
        lines.append("  %-16s%10.3f |%9.1f | %s" % (key, ms, first["n"][count] / (ms * 1e-3) / 1e6, "  ".join("%.3f" % v for v in each)))
    cam = statistics.median(r["ms"]["camera"] / r["n"]["camera"] for r in runs)
    ren = statistics.median(r["ms"]["render"] / r["n"]["render"] for r in runs)
    lines += ["", "time per path, camera rays through gbl_radiance_rays over gbl_render's: %.2f" % (cam / ren),
              "mean radiance: camera %.5f, probes %.5f" % (first["mean"]["camera"], first["mean"]["probes"]), ""]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
