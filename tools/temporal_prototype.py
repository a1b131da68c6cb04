#!/usr/bin/env python3
"""CPU prototype of the temporal accumulation's quality: the frame loop of tests/test_gpu_temporal.py's
end-to-end test on films rendered by the oracle, accumulated and filtered by the numpy restatements of the two contracts.

    python tools/temporal_prototype.py [--frames 8] [--travel 0.1] [--iterations 3]

Cornell 64 x 64, depth 4, 4 spp per frame along a sideways camera move; the last frame against 256 spp from the last camera.
Prints the relMSE of the single last frame, of the accumulated film, and of both after the a-trous filter, with the variance
plane and without it (the moment-based variance)."""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from goblin_amd import scene as gs   # noqa: E402
import aov_reference as ar           # noqa: E402
import denoise_reference as dr       # noqa: E402
import oracle_binding as ob          # noqa: E402
import temporal_reference as tr      # noqa: E402


def camera_dict(cam):
    return {name: (tuple(getattr(cam, name)) if name in ("position", "orientation") else getattr(cam, name)) for name in tr.CAMERA_FIELDS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--travel", type=float, default=0.1)
    ap.add_argument("--iterations", type=int, default=3)
    args = ap.parse_args()
    frames = []
    for i in range(args.frames):
        scene = gs.load_scene("cornell", gs.config_overrides(resolution=(64, 64), spp=4, depth=4))
        scene.desc.camera.position[0] += args.travel * (i / max(1, args.frames - 1) - 1.0)
        ref = ar.Reference(scene, seed=i)
        li = ref.oracle.li_native(i)
        frames.append(dict(film=ref.oracle.splat(ref.samples, li), variance=dr.variance(li, ref.window, 4, 64, 64), camera=camera_dict(scene.desc.camera),
                           **ref.films()))
        print("frame %d rendered" % i, flush=True)
    scene = gs.load_scene("cornell", gs.config_overrides(resolution=(64, 64), spp=256, depth=4))
    oracle = ob.Oracle(scene)
    clean = ob.normalize_film(oracle.splat(oracle.native_samples(11), oracle.li_native(11, threads=ob.hardware_threads())))
    last = frames[-1]
    guides = dict(albedo=last["albedo"], normal=last["normal"], depth=last["depth"])
    noisy = dr.rel_mse(ob.normalize_film(last["film"]), clean)
    single = dr.rel_mse(dr.denoise(last["film"], last["variance"], iterations=args.iterations, **guides)[..., :3], clean)
    for with_variance in (True, False):
        history, prev = None, None
        for f in frames:
            acc = tr.accumulate(f["film"], f["depth"], f["camera"], variance=f["variance"] if with_variance else None, normal=f["normal"],
                                history=history, prev_camera=prev, **tr.DEFAULTS)
            history, prev = acc["history"], f["camera"]
        accumulated = dr.rel_mse(acc["film"][..., :3], clean)
        both = dr.rel_mse(dr.denoise(acc["film"], acc["variance"], iterations=args.iterations, **guides)[..., :3], clean)
        print("variance plane %s: history length mean %.2f; relMSE single frame %.4g, accumulated %.4g (ratio %.3f); single frame denoised %.4g, "
              "accumulated then denoised %.4g (ratio %.3f)" % (with_variance, acc["N"].mean(), noisy, accumulated, accumulated / noisy, single, both, both / single))


if __name__ == "__main__":
    main()
