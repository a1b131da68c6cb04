"""A/B of two libgoblin_hip builds on the workloads of ONE kernel unit: kernel ms (best of 3 renders) per workload, the two
libraries alternating, one fresh process per run.  What decided goblin_amd/build.py UNIT_FLAGS (profiles/slp_splat_ab.txt).

    python tools/unit_ab.py [--reps 3] <unit | case,case,...> <a.so | main> <b.so | main>

Library names are looked up under goblin_amd/lib/variants/ ('noslp_quad' -> libgoblin_hip_noslp_quad.so; 'main': the shipped one).
"""
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUNNY = dict(resolution=(512, 512), spp=256, depth=8)
CASES = {   # name: (scene, overrides, render keywords, environment)
    "bunny_mk": ("bunny", BUNNY, dict(schedule="megakernel"), {}),
    "bunny_exact": ("bunny", BUNNY, dict(schedule="megakernel", exact_ties=True), {}),
    "bunny_lane": ("bunny", BUNNY, dict(schedule="megakernel"), {"GBL_MK_QUAD": "0"}),
    "bunny_lane_exact": ("bunny", BUNNY, dict(schedule="megakernel", exact_ties=True), {"GBL_MK_QUAD": "0"}),
    "bunny_stream": ("bunny", BUNNY, dict(sampler="stream"), {}),
    "bunny_wf": ("bunny", BUNNY, dict(schedule="wavefront"), {}),
    "cornell_wf": ("cornell", dict(resolution=(512, 512), spp=64, depth=16), dict(schedule="wavefront"), {}),
    "cornell_mk": ("cornell", dict(resolution=(512, 512), spp=64, depth=16), dict(schedule="megakernel"), {}),
    "grid_mk": ("grid", dict(resolution=(512, 512), spp=64, depth=8), dict(schedule="megakernel"), {}),
    "bunny_ao": ("bunny", dict(resolution=(1024, 1024), spp=64, method="ao", ao_samples=25), {}, {}),
    "masked_mk": ("masked", dict(resolution=(512, 512), spp=64), dict(schedule="megakernel"), {}),
    "shapes_mk": ("shapes", dict(resolution=(512, 512), spp=64), dict(schedule="megakernel"), {}),
    "whitted": ("whitted", dict(resolution=(512, 512), spp=64), {}, {}),
    "subsurface": ("subsurface", dict(resolution=(256, 256), spp=16), dict(schedule="megakernel"), {}),
    "volume": ("volume", dict(resolution=(256, 256), spp=16), dict(schedule="megakernel"), {}),
    "aov": ("bunny", dict(resolution=(512, 512), spp=64, depth=8), "aov", {}),
    "aov_cornell": ("cornell", dict(resolution=(512, 512), spp=64, depth=8), "aov", {}),
}
UNITS = {"kernels_quad": ["bunny_mk", "bunny_exact", "bunny_ao", "grid_mk", "cornell_mk"],
         "kernels_path": ["bunny_lane", "bunny_lane_exact", "masked_mk", "shapes_mk"],
         "kernels_wavefront": ["cornell_wf", "bunny_wf"],
         "kernels_stream": ["bunny_stream"],
         "kernels_whitted": ["whitted"],
         "kernels_aux": ["subsurface", "volume"],
         "kernels_aov": ["aov", "aov_cornell"]}

CHILD = r'''
import sys, json, os
sys.path.insert(0, %r)
cases = json.loads(sys.argv[1])
import torch
from goblin_amd import scene as gs
from goblin_amd.renderer import HipPathTracer
row = {}
for name, (sc_name, ov, kw, env) in cases.items():
    os.environ.update(env)   # (read by the library when it picks a kernel: kept until the case is over)
    tr = HipPathTracer(gs.load_scene(sc_name, gs.config_overrides(**{k: tuple(v) if isinstance(v, list) else v for k, v in ov.items()})), 0)
    film = tr.new_film()
    best = 1e30
    for i in range(4):
        if kw == "aov":
            out = tr.render_aov(seed=1, timed=True)
        else:
            film.zero_()
            out = tr.render(film=film, seed=1, timed=True, **kw)
        torch.cuda.synchronize()
        if i:
            best = min(best, out["stats"]["kernel_ms"])
    row[name] = round(best, 3)
    for k in env:
        del os.environ[k]
print(json.dumps(row), flush=True)
''' % REPO


def lib_path(name):
    if name == "main":
        return os.path.join(REPO, "goblin_amd", "lib", "libgoblin_hip.so")
    if os.path.exists(name):
        return os.path.abspath(name)
    return os.path.join(REPO, "goblin_amd", "lib", "variants", "libgoblin_hip_%s.so" % name)


def main():
    args = sys.argv[1:]
    reps = 3
    if args[0] == "--reps":
        reps, args = int(args[1]), args[2:]
    what, a, b = args
    names = UNITS[what] if what in UNITS else what.split(",")
    cases = {n: CASES[n] for n in names}
    runs = {a: [], b: []}
    for _ in range(reps):
        for lib in (a, b):
            env = dict(os.environ, GOBLIN_HIP_LIB=lib_path(lib))
            p = subprocess.run([sys.executable, "-c", CHILD, json.dumps(cases)], env=env, capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                sys.stderr.write(p.stderr[-2000:])
                sys.exit("run of %s ended with status %d: nothing more is started" % (lib, p.returncode))
            runs[lib].append(json.loads(p.stdout.strip().splitlines()[-1]))
    for n in names:
        va, vb = [r[n] for r in runs[a]], [r[n] for r in runs[b]]
        print("%-18s %s: %s | %s: %s   median %.3f -> %.3f (%+.2f %%)" % (
            n, a, " ".join("%.3f" % v for v in va), b, " ".join("%.3f" % v for v in vb), statistics.median(va), statistics.median(vb),
            100.0 * (statistics.median(vb) / statistics.median(va) - 1.0)), flush=True)


if __name__ == "__main__":
    main()
