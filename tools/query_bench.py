#!/usr/bin/env python3
"""Throughput of gbl_trace_rays on bunny.json (host-built context), three populations of 2^22 rays:

    primary   the camera's rays through a 2048 x 2048 grid of pixel centres, in pixel order (coherent)
    ao        cosine-hemisphere rays of length 0.1 x scene radius from those rays' hits (incoherent, short)
    chords    segments between uniform points of the scene bound (incoherent, long)

For each: closest and any, lean and exact, by HIP events around --window-ms (100 ms) of calls back to back, the median of --calls
such windows after --warm warm-up calls; reported as ms per call and Grays/s.  The baseline is the parent's only way to ask,
gbl_selftest_trace (EXT build, tie rule, plain LDS stacks, one ray per lane, a device synchronise), timed by wall clock around
the call on the same rays.  For context: gbl_render_aov's kernel_ms per camera ray on a 512 x 512 x 16 spp frame.

The two forms of the kernel are two builds of the library -- the shipped one and the one-ray-per-lane measurement form,
    python tools/build_variant.py queryplain kernels_query -DGBL_QUERY_PLAIN
-- each measured in a child process of its own (GOBLIN_HIP_LIB), alternating, --rounds times.

    python tools/query_bench.py [--out table.txt] [--rounds 2] [--log2n 22]
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PLAIN_LIB = os.path.join(REPO, "goblin_amd", "lib", "variants", "libgoblin_hip_queryplain.so")
POPULATIONS = ("primary", "ao", "chords")
VARIANTS = (("closest", False), ("closest", True), ("any", False), ("any", True))


def rotate(torch, q, v):
    """v turned by the unit quaternion q = (w, x, y, z)."""
    w, u = q[0], torch.tensor(q[1:], dtype=torch.float64)
    v = torch.tensor(v, dtype=torch.float64)
    return v + 2.0 * torch.linalg.cross(u, torch.linalg.cross(u, v) + w * v)


def populations(torch, r, n_side, seed=99):
    """The three (n, 8) ray tensors on the device, and each one's hit fraction under a lean closest-hit query."""
    dev = r.device
    cam = r.camera()
    q = [float(x) for x in cam.orientation]
    fwd, right, up = (rotate(torch, q, v).to(dev) for v in ((0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)))
    tan_half = math.tan(math.radians(float(cam.fov_degrees)) * 0.5)
    g = (torch.arange(n_side, device=dev, dtype=torch.float64) + 0.5) / n_side
    y, x = torch.meshgrid(g, g, indexing="ij")
    d = fwd[None] + ((2.0 * x.reshape(-1, 1) - 1.0) * tan_half) * right[None] + ((1.0 - 2.0 * y.reshape(-1, 1)) * tan_half) * up[None]
    d = d / d.norm(dim=1, keepdim=True)
    n = n_side * n_side
    primary = torch.zeros((n, 8), dtype=torch.float32, device=dev)
    primary[:, 0:3] = torch.tensor([float(v) for v in cam.position], device=dev)
    primary[:, 3], primary[:, 4:7], primary[:, 7] = 1e-3, d.float(), float("inf")
    # the scene bound: the instances' boxes without the stage floor (the widest of them)
    b = r._instances_raw()["bounds"]
    keep = sorted(range(len(b)), key=lambda i: float(((b["hi"][i] - b["lo"][i]) ** 2).sum()))[:max(1, len(b) - 1)]
    lo = torch.tensor(b["lo"][keep].min(axis=0), device=dev)
    hi = torch.tensor(b["hi"][keep].max(axis=0), device=dev)
    radius = 0.5 * float((hi - lo).norm())
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    # AO-like: cosine-hemisphere directions about the shading normal (turned towards the viewer) at the primary hits
    hits = r.trace(primary, normals=True)
    got = hits["instance"] >= 0
    idx = torch.nonzero(got).reshape(-1)
    idx = idx[torch.arange(n, device=dev) % max(1, idx.numel())]      # every ray starts from a hit; the hits repeat in order
    p = primary[idx, 0:3] + hits["t"][idx, None] * primary[idx, 4:7]
    nrm = hits["normal"][idx]
    nrm = torch.where((nrm * primary[idx, 4:7]).sum(dim=1, keepdim=True) > 0, -nrm, nrm)
    u = torch.rand((n, 2), device=dev, generator=gen)
    rad, phi = u[:, 0].sqrt(), 2.0 * math.pi * u[:, 1]
    a = torch.where(nrm[:, 0:1].abs() > 0.9, torch.tensor([0.0, 1.0, 0.0], device=dev), torch.tensor([1.0, 0.0, 0.0], device=dev)).expand(n, 3)
    t1 = torch.linalg.cross(nrm, a)
    t1 = t1 / t1.norm(dim=1, keepdim=True)
    t2 = torch.linalg.cross(nrm, t1)
    ad = (rad * phi.cos())[:, None] * t1 + (rad * phi.sin())[:, None] * t2 + (1.0 - u[:, 0]).clamp_min(0).sqrt()[:, None] * nrm
    ao = torch.zeros_like(primary)
    ao[:, 0:3], ao[:, 3], ao[:, 4:7], ao[:, 7] = p, 1e-3 * radius, ad, 0.1 * radius
    # chords
    pq = lo[None, None] + torch.rand((n, 2, 3), device=dev, generator=gen) * (hi - lo)[None, None]
    chords = torch.zeros_like(primary)
    chords[:, 0:3], chords[:, 3], chords[:, 4:7], chords[:, 7] = pq[:, 0], 1e-3, pq[:, 1] - pq[:, 0], 1.0
    out = {"primary": primary, "ao": ao.contiguous(), "chords": chords}
    frac = {k: float((r.trace(v)["instance"] >= 0).float().mean()) for k, v in out.items()}
    return out, frac, radius


def child(a):
    import torch
    from goblin_amd import _abi
    from goblin_amd import scene as gs
    from goblin_amd.renderer import HipPathTracer
    r = HipPathTracer(gs.load_scene("bunny", gs.config_overrides(resolution=(512, 512), spp=16, depth=5)), 0)
    n_side = 1 << (a.log2n // 2)
    pops, frac, radius = populations(torch, r, n_side)
    n = n_side * n_side
    res = {"n": n, "device": torch.cuda.get_device_name(0), "hit_fraction": frac, "radius": radius, "ms": {}, "hook_ms": {}}

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
        # a window holds as many calls back to back as fill --window-ms (a call is 0.07 - 1 ms: eight of them would time the
        # clock and the scheduler as much as the kernel), sized from a first window of --batch calls
        batch = max(a.batch, min(4096, int(math.ceil(a.window_ms / max(1e-3, window(fn, a.batch))))))
        return statistics.median(window(fn, batch) for _ in range(a.calls))

    for name, rays in pops.items():
        out_hit = torch.empty((n, 8), dtype=torch.float32, device=r.device)
        out_any = torch.empty((n,), dtype=torch.uint8, device=r.device)
        for kind, exact in VARIANTS:
            out = out_hit if kind == "closest" else out_any
            res["ms"]["%s/%s/%s" % (name, kind, "exact" if exact else "lean")] = timed(lambda: r.trace(rays, kind=kind, exact_ties=exact, out=out))
        if a.hook:   # the baseline: 9-float records, wall clock around the hook's own synchronise
            for kind in (0.0, 1.0):
                rec = torch.zeros((n, 9), dtype=torch.float32, device=r.device)
                rec[:, 0], rec[:, 1:4], rec[:, 4:7], rec[:, 7], rec[:, 8] = kind, rays[:, 0:3], rays[:, 4:7], rays[:, 3], rays[:, 7]
                out = torch.empty((n, 8), dtype=torch.float32, device=r.device)

                def call():
                    assert r.lib.gbl_selftest_trace(r.handle, rec.data_ptr(), out.data_ptr(), n) == _abi.GBL_OK
                for _ in range(a.warm):
                    call()
                ms = []
                for _ in range(a.calls):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    call()
                    ms.append((time.perf_counter() - t0) * 1e3)
                res["hook_ms"]["%s/%s" % (name, "closest" if kind == 0.0 else "any")] = statistics.median(ms)
    if a.hook:
        films = {k: r.new_film() for k in ("albedo", "normal", "depth")}
        st = [r.render_aov(films=films, timed=True)["stats"] for _ in range(4)][1:]
        res["aov_ms"], res["aov_rays"] = statistics.median(s["kernel_ms"] for s in st), int(st[0]["paths"])
    print("QUERY_BENCH " + json.dumps(res))


def grays(n, ms):
    return n / (ms * 1e-3) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--hook", action="store_true")
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
    forms = [("persistent", None)] + ([("plain", PLAIN_LIB)] if os.path.exists(PLAIN_LIB) else [])
    runs = {f: [] for f, _ in forms}
    for _ in range(a.rounds):
        for form, lib in forms:   # alternating
            env = dict(os.environ)
            env.pop("GOBLIN_HIP_LIB", None)
            if lib:
                env["GOBLIN_HIP_LIB"] = lib
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--log2n", str(a.log2n), "--calls", str(a.calls), "--batch", str(a.batch),
                   "--window-ms", str(a.window_ms), "--warm", str(a.warm)] + (["--hook"] if form == "persistent" else [])
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=500)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("QUERY_BENCH ")]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit("query_bench: the %s form's run failed (status %d)" % (form, p.returncode))
            runs[form].append(json.loads(line[0][len("QUERY_BENCH "):]))
    first = runs["persistent"][0]
    n = first["n"]
    med = lambda rs, key, field="ms": statistics.median(r[field][key] for r in rs)   # noqa: E731
    lines = ["gbl_trace_rays on bunny.json, host-built context, %d rays per population, %s" % (n, first["device"]),
             "median of %d windows of %.0f ms of calls back to back (HIP events) per run, median over %d alternating runs per form; ms per call | Grays/s" % (a.calls, a.window_ms, a.rounds),
             "hit fraction (lean closest): " + ", ".join("%s %.3f" % (k, first["hit_fraction"][k]) for k in POPULATIONS), "",
             "%-24s" % "population/kind/mode" + "".join("%22s" % f for f, _ in forms) + "%26s" % "gbl_selftest_trace (wall)"]
    for name in POPULATIONS:
        for kind, exact in VARIANTS:
            key = "%s/%s/%s" % (name, kind, "exact" if exact else "lean")
            row = "%-24s" % key
            for form, _ in forms:
                ms = med(runs[form], key)
                row += "%12.3f |%7.2f " % (ms, grays(n, ms))
            if exact:
                hk = med(runs["persistent"], "%s/%s" % (name, kind), "hook_ms")
                row += "%14.3f |%7.2f " % (hk, grays(n, hk))
            lines.append(row)
    aov = statistics.median(r["aov_ms"] for r in runs["persistent"])
    lines += ["", "for context: gbl_render_aov kernel_ms %.3f for %d camera rays (512 x 512 x 16 spp, three films): %.2f Grays/s" %
              (aov, first["aov_rays"], grays(first["aov_rays"], aov))]
    lean_ok = all(med(runs["persistent"], "%s/closest/lean" % p) <= med(runs["persistent"], "%s/closest" % p, "hook_ms") for p in POPULATIONS)
    lines.append("shipped lean closest-hit form not slower than gbl_selftest_trace on any population: %s" % ("yes" if lean_ok else "NO"))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
        with open(os.path.splitext(a.out)[0] + ".json", "w") as f:
            json.dump(runs, f)


if __name__ == "__main__":
    main()
