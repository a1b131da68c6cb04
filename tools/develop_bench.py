#!/usr/bin/env python3
"""Device time of gbl_film_develop (bloom + tone map) against the host chain gbl_host_bloom + gbl_host_tone_map on the same
image, and the tone map alone at a large size (its serial sum is the part that does not scale).  HIP events, one warm-up
call, the median of --calls calls; the host chain runs once.  Prints one JSON line.

    python tools/develop_bench.py [--sizes 512 1024] [--radius 0.05] [--tone-size 2048] [--no-host] [--calls 9]

Under `rocprofv3 --kernel-trace --stats -- python tools/develop_bench.py --no-host` the per-kernel rows give bloom_kernel and
tone_sum_kernel on their own, and the kernel trace's scratch column shows whether a kernel spills.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from goblin_amd import _abi, scene as gs  # noqa: E402
from goblin_amd.renderer import HipPathTracer  # noqa: E402


def image(n, seed=1):
    """A seeded HDR image: mostly below 4, a few hundred highlights."""
    rng = np.random.default_rng(seed)
    img = rng.random((n, n, 3), dtype=np.float32) ** 3 * 4.0
    ys, xs = rng.integers(n, size=n // 2), rng.integers(n, size=n // 2)
    img[ys, xs] = rng.uniform(20.0, 400.0, size=(n // 2, 3)).astype(np.float32)
    return np.ascontiguousarray(img)


def device_ms(tracer, accum, calls, **kw):
    tracer.develop(accum, **kw)    # warm-up: scratch, the filter table
    torch.cuda.synchronize()
    times = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = tracer.develop(accum, **kw)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), min(times), out["rgb"].cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--radius", type=float, default=0.05)
    ap.add_argument("--weight", type=float, default=0.3)
    ap.add_argument("--tone-size", type=int, default=2048)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    host = _abi.host_lib()
    result = {"radius": a.radius, "weight": a.weight, "calls": a.calls, "sizes": []}
    for n in a.sizes:
        tracer = HipPathTracer(gs.load_scene("cornell", gs.config_overrides(resolution=(n, n), spp=1, depth=2)), 0)
        rgb = image(n)
        accum = torch.ones((n, n, 4), dtype=torch.float32, device="cuda")
        accum[..., :3] = torch.from_numpy(rgb).cuda()
        med, best, got = device_ms(tracer, accum, a.calls, bloom_radius=a.radius, bloom_weight=a.weight, tone_mapping=True)
        row = {"size": n, "fw": int(np.ceil(np.float32(a.radius) * np.float32(n))) // 2, "device_ms_median": med, "device_ms_min": best}
        row["device_bloom_only_ms_median"] = device_ms(tracer, accum, a.calls, bloom_radius=a.radius, bloom_weight=a.weight, tone_mapping=False)[0]
        if not a.no_host:
            want = rgb.copy()
            t0 = time.perf_counter()
            host.gbl_host_bloom(want.ctypes.data_as(C.c_void_p), n, n, a.radius, a.weight)
            t1 = time.perf_counter()
            host.gbl_host_tone_map(want.ctypes.data_as(C.c_void_p), n, n)
            t2 = time.perf_counter()
            row.update(host_bloom_ms=(t1 - t0) * 1e3, host_tone_map_ms=(t2 - t1) * 1e3, host_ms=(t2 - t0) * 1e3,
                       max_rel_diff=float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-6))))
        result["sizes"].append(row)
        del tracer
    n = a.tone_size
    if n > 0:
        tracer = HipPathTracer(gs.load_scene("cornell", gs.config_overrides(resolution=(n, n), spp=1, depth=2)), 0)
        accum = torch.ones((n, n, 4), dtype=torch.float32, device="cuda")
        accum[..., :3] = torch.from_numpy(image(n)).cuda()
        tone = device_ms(tracer, accum, a.calls, bloom_radius=0.0, bloom_weight=0.0, tone_mapping=True)[0]
        plain = device_ms(tracer, accum, a.calls, bloom_radius=0.0, bloom_weight=0.0, tone_mapping=False)[0]
        result["tone_map"] = {"size": n, "tone_map_ms_median": tone - plain, "resolve_ms_median": plain}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
