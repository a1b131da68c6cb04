#!/usr/bin/env python3
"""Golden fixtures for the device side of Film::writeImage's tail (gbl_film_develop), from the REAL reference.

Runs only in the authoring container (needs oracle/_ref/ref_harness, `make -C oracle ref`).  Drives the harness's
`image` mode twice per case: once on a seeded synthetic HDR image (bloom, toneMapping and the tone-mapped .ppm of the
input) and once on the reference's own bloom output, which gives the whole chain bloom -> toneMapping -> .ppm.  Data only.

    python tests/golden/make_develop_golden.py

  develop_a  96 x 40, radius 0.5  -> filter width 24: a 47-wide window, wider than a tile and taller than the image
  develop_b  67 x 45, radius 0.15 -> filter width 5: odd sizes, clipped and unclipped pixels
  develop_c  67 x 45, same filter, luminance log-uniform over 10^-3 .. 10^8: the one input on which the ORDER of the tone
             map's sum shows in the output (asserted below)
"""
import ctypes
import ctypes.util
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
HARNESS = os.path.join(REPO, "oracle", "_ref", "ref_harness")

# name -> (width, height, seed, bloom radius, bloom weight, kind)
CASES = {"develop_a": (96, 40, 21, 0.5, 0.3, "gradient"),
         "develop_b": (67, 45, 22, 0.15, 0.6, "gradient"),
         "develop_c": (67, 45, 23, 0.15, 0.6, "log_uniform")}


def gradient(w, h, seed):
    """The image of make_image_golden.py without its half-float probes: a smooth gradient with a few very bright pixels."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.stack([0.2 + 0.8 * x / w, 0.1 + 0.5 * y / h, 0.3 + 0.3 * np.sin(0.4 * x + 0.3 * y), np.ones_like(x)], axis=-1).astype(np.float32)
    img[..., :3] *= rng.uniform(0.5, 1.5, size=(h, w, 3)).astype(np.float32)
    for _ in range(6):
        img[rng.integers(h), rng.integers(w), :3] = rng.uniform(20.0, 400.0, size=3).astype(np.float32)
    return img


def log_uniform(w, h, seed):
    """Luminance drawn log-uniformly from 10^-3 to 10^8, random chroma."""
    rng = np.random.default_rng(seed)
    lum = 10.0 ** rng.uniform(-3.0, 8.0, size=(h, w))
    chroma = rng.uniform(0.5, 1.5, size=(h, w, 3))
    img = np.ones((h, w, 4), np.float32)
    img[..., :3] = (chroma * lum[..., None]).astype(np.float32)
    return img


def filter_width(radius, w, h):
    """Goblin::bloom's filterWidth, in float like the reference (GoblinImageIO.cpp:175)."""
    return int(np.ceil(np.float32(radius) * np.float32(max(w, h)))) // 2


def harness(img, w, h, radius, weight, tmp, tag):
    src = os.path.join(tmp, tag + ".in.f32")
    np.ascontiguousarray(img, np.float32).tofile(src)
    prefix = os.path.join(tmp, tag)
    meta = json.loads(subprocess.check_output([HARNESS, "image", src, str(w), str(h), prefix, repr(radius), repr(weight)]).decode())
    assert (meta["width"], meta["height"]) == (w, h)
    out = {k: np.fromfile(prefix + "." + k + ".f32", np.float32).reshape(h, w, 4) for k in ("bloom", "tone")}
    out["ppm_bytes"] = np.fromfile(prefix + ".ppm", np.uint8)
    return out


def tone_map(rgb, total):
    """Goblin::toneMapping given the sum of logf(1e4 + luminance): glibc's expf, float arithmetic in the reference's order."""
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.expf.restype, libm.expf.argtypes = ctypes.c_float, [ctypes.c_float]
    h, w, _ = rgb.shape
    ywa = np.float32(libm.expf(ctypes.c_float(np.float32(total) / np.float32(w * h))))
    inv = np.float32(1.0) / (ywa * ywa)
    y = luminance(rgb)
    s = (np.float32(1.0) + y * inv) / (np.float32(1.0) + y)
    return rgb * s[..., None]


def luminance(rgb):
    return np.float32(0.212671) * rgb[..., 0] + np.float32(0.715160) * rgb[..., 1] + np.float32(0.072169) * rgb[..., 2]


def log_luminance(rgb):
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.logf.restype, libm.logf.argtypes = ctypes.c_float, [ctypes.c_float]
    v = (np.float32(1e4) + luminance(rgb)).reshape(-1)
    return np.array([libm.logf(ctypes.c_float(x)) for x in v], np.float32)


def sum_order_shows(img, tone_ref):
    """Fraction of pixels whose tone-mapped value changes, bit-wise, when the sum of the logs is numpy's pairwise
    np.sum instead of the reference's serial one.  The serial restatement must reproduce the reference exactly first."""
    rgb = np.ascontiguousarray(img[..., :3])
    logs = log_luminance(rgb)
    serial = np.cumsum(logs, dtype=np.float32)[-1]     # cumsum adds in index order
    np.testing.assert_array_equal(tone_map(rgb, serial), tone_ref[..., :3])
    tree = tone_map(rgb, np.sum(logs, dtype=np.float32))
    return float(np.mean(np.any(tree.view(np.uint32) != tone_ref[..., :3].view(np.uint32), axis=-1)))


def main():
    if not os.path.exists(HARNESS):
        sys.exit("oracle/_ref/ref_harness is missing: run `make -C oracle ref` (needs the reference's sources)")
    for name, (w, h, seed, radius, weight, kind) in CASES.items():
        img = (gradient if kind == "gradient" else log_uniform)(w, h, seed)
        with tempfile.TemporaryDirectory() as tmp:
            first = harness(img, w, h, radius, weight, tmp, "first")
            second = harness(first["bloom"], w, h, radius, weight, tmp, "second")   # toneMapping / .ppm of the bloomed image
        arrays = {"input": img, "bloom_radius": np.float32(radius), "bloom_weight": np.float32(weight),
                  "fw": np.int32(filter_width(radius, w, h)),
                  "bloom": first["bloom"], "tone": first["tone"], "ppm_bytes": first["ppm_bytes"],
                  "bloom_tone": second["tone"], "bloom_tone_ppm": second["ppm_bytes"]}
        changed = sum_order_shows(img, first["tone"])
        if kind == "log_uniform":
            assert changed > 0.05, "%s: a reordered sum changes only %.1f %% of the pixels" % (name, 100.0 * changed)
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **arrays)
        print("%s %d x %d fw %d: a pairwise sum changes %.1f %% of the tone-mapped pixels" % (name, w, h, int(arrays["fw"]), 100.0 * changed))


if __name__ == "__main__":
    main()
