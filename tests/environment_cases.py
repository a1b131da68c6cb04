"""TEST INFRASTRUCTURE: pairs of scenes that differ only in the files behind their image based lights
(tests/test_gpu_environment.py, tests/test_environment_cpu.py).

Scene A and scene B of a case are one generated document -- a few lit quads (tests/texture_chart.py _base), an `ibl` light over
env.exr and, by variant, a point light -- loaded from two directories whose env.exr have the same size and other texels.  The
expected tables are always a fresh context made from B, read through the hooks the edited context is read through: that is
gbl_create's path (scene_prep.cpp on the host), never the code under test.

Sizes, and why each is there:
  1x1                       the distribution and the average radiance are level 0 itself
  2x1 1x8 5x3 64x4 4x64 16x16   the texture charts' sizes (5x3 becomes 8x4 in the loader): single rows and columns, strips
  256x128                   the largest distribution taken from level 0; more rows than a wave, rows of four column tiles
  512x256                   the distribution is read from level 1, which the pyramid launches have just written
  1024x4                    a distribution of 256 x 1
  4x1024                    a distribution of 1 x 256

Variants: "lamp_first" (point light, then the ibl), "ibl_first", "only" (the ibl is the only light), "two" (ibl over env.exr,
point light, ibl over env2.exr of 8 x 4), "whitted" (lamp_first under the Whitted integrator).

Texels: "render" -- multiples of 1/32 in [1/32, 1], strictly positive, since a row or an image that sums to zero makes the
host's own CDF 0 / 0; "wide" -- image_edit_cases.draw's, either sign and any magnitude of half's normal range, for cancellation
in the serial sums (table-only: a negative radiance is nothing to render; WIDE_SALT is chosen so that fresh B's distribution is
all finite, which the test asserts); "blackrow" -- "render" with row 5 of B exactly black, whose row block is NaN on the host
(table-only: the NaN positions and every other bit are compared)."""
import functools
import json
import os
import zlib

import numpy as np

from goblin_amd import scene as gs
import image_edit_cases as ic
import texture_chart as tc

SIZES = {"1x1": (1, 1), "2x1": (2, 1), "1x8": (1, 8), "5x3": (5, 3), "64x4": (64, 4), "4x64": (4, 64), "16x16": (16, 16),
         "256x128": (256, 128), "512x256": (512, 256), "1024x4": (1024, 4), "4x1024": (4, 1024)}
LOADED = dict(SIZES, **{"5x3": (8, 4)})          # the sides the loader leaves
SECOND = (8, 4)                                  # env2.exr of the "two" variant
VARIANTS = ["lamp_first", "ibl_first", "only", "two", "whitted"]
FRAME = dict(resolution=(24, 16), spp=4, depth=3)
WIDE_SIZE, WIDE_SALT = "256x128", "B"
BLACK_SIZE, BLACK_ROW = "16x16", 5
CELLS = [[0.7, 0.6, 0.5], [0.3, 0.6, 0.8], [0.8, 0.8, 0.8], [0.6, 0.3, 0.4]]


def draw(w, h, flavour, salt):
    """(h, w, 3) float32 texels that are exact in half floats."""
    if flavour == "wide":
        return ic.draw(w, h, "wide", salt)
    rng = np.random.RandomState(zlib.crc32(("environment %dx%d %s" % (w, h, salt)).encode()) & 0x7FFFFFFF)
    img = np.ascontiguousarray(rng.randint(1, 33, (h, w, 3)).astype(np.float32) / np.float32(32.0))
    if flavour == "blackrow" and salt == "B":
        img[BLACK_ROW] = 0.0
    else:
        assert flavour in ("render", "blackrow"), flavour
    return img


def ibl(name, file, orientation=(0.9659258, 0.0, 0.258819, 0.0)):
    return {"name": name, "type": "ibl", "file": file, "filter": [1.0, 0.95, 0.9], "orientation": list(orientation), "sample_num": 4}


def doc(variant):
    d = tc._base("perspective")
    lamp = d["lights"][0]
    for k, colour in enumerate(CELLS):
        d["textures"].append({"format": "color", "name": "k%d" % k, "type": "constant", "color": colour})
        d["materials"].append({"name": "c%d" % k, "type": "lambert", "Kd": "k%d" % k})
        tc._place(d, k + 4, "c%d" % k)               # the grid's middle row
    d["lights"] = {"lamp_first": [lamp, ibl("sky", "env.exr")], "whitted": [lamp, ibl("sky", "env.exr")], "ibl_first": [ibl("sky", "env.exr"), lamp],
                   "only": [ibl("sky", "env.exr")],
                   "two": [ibl("sky", "env.exr"), lamp, ibl("ground", "env2.exr", (0.7071068, 0.7071068, 0.0, 0.0))]}[variant]
    gs._merge(d, gs.config_overrides(method="whitted" if variant == "whitted" else None, **FRAME))
    return d


def directory(size, flavour, salt):
    """plane.obj, env.exr of `size` and env2.exr."""
    def fill(d):
        tc.write_files(d, images=())
        w, h = SIZES[size]
        ic.write_exr(os.path.join(d, "env.exr"), draw(w, h, flavour, salt))
        ic.write_exr(os.path.join(d, "env2.exr"), draw(SECOND[0], SECOND[1], "render", salt + " second"))
    return ic._directory(("environment", size, flavour, salt), fill)


@functools.lru_cache(maxsize=None)
def pair(size, variant="lamp_first", flavour="render"):
    """(scene A, scene B), loaded once and never written to."""
    text = json.dumps(doc(variant))
    salt_b = WIDE_SALT if flavour == "wide" else "B"
    return gs.load_scene_text(text, directory(size, flavour, "A")), gs.load_scene_text(text, directory(size, flavour, salt_b))


@functools.lru_cache(maxsize=None)
def bundled_pair():
    """The bundled `ibl` scene, and the same document over a drawn images/env.exr of the bundled file's size."""
    with open(gs.scene_path("ibl")) as f:
        d = ic._frame(json.load(f), **ic.BUNDLED_FRAME)

    def fill(to):
        import shutil
        from goblin_amd import _abi
        for sub in ("models", "images"):
            os.makedirs(os.path.join(to, sub))
        for g in d["geometries"]:
            if "file" in g:
                shutil.copy(os.path.join(gs.SCENE_DIR, g["file"]), os.path.join(to, g["file"]))
        for t in d.get("textures", []):
            if "file" in t:
                shutil.copy(os.path.join(gs.SCENE_DIR, t["file"]), os.path.join(to, t["file"]))
        h, w = _abi.read_image(os.path.join(gs.SCENE_DIR, "images", "env.exr")).shape[:2]
        ic.write_exr(os.path.join(to, "images", "env.exr"), draw(w, h, "render", "B"))
    text = json.dumps(d)
    return gs.load_scene_text(text, gs.SCENE_DIR), gs.load_scene_text(text, ic._directory(("environment", "bundled"), fill))


def ibl_lights(scene):
    from goblin_amd import _abi
    d = scene.desc
    return [i for i in range(d.num_lights) if d.lights[i].type == _abi.GBL_LIGHT_IBL]


def environment_level0(scene, light):
    """Level 0 of the light's image as the loader left it: (height, width, 4)."""
    return ic.level0(scene, scene.desc.lights[light].image)
