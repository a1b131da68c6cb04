"""TEST INFRASTRUCTURE: pairs of scenes that differ only in the files behind their images (tests/test_gpu_image_edit.py).

Scene A and scene B of a case are one document loaded from two directories whose image files have the same names and sizes and
other texels.  The expected pyramids are the project's own loader's: B.desc.texels is what gbl_create uploads for B, so a context
made from A whose every image was edited to B's level 0 must hold B's pool, byte for byte.

The files pass through the EXR writer's half floats, so the texels are drawn as halves.  Two flavours:
  wide  a sign, an exponent anywhere in half's normal range (2^-14 .. 2^15), a 10-bit mantissa, one texel in eight exactly 0 --
        for the pyramid bytes (a weight times a texel of either sign and any magnitude; sums that cancel);
  mild  multiples of 1 / 32 in [0, 31 / 32], exact zeros among them -- for the renders, whose materials want an albedo below 1
        and whose gamma slots (powf) want no negative texel, or the radiance would hold NaNs of unspecified bits.

Cases: "sizes" -- every chart size (tests/texture_chart.py IMAGES) once as a colour and once as a float image, then a 256 x 128
colour image whose levels span many workgroups, in one pool: a 1-channel pyramid of an odd float count in front of a 4-channel
one puts that one at a float offset that is no multiple of four, between neighbours a stray write would hit; "chart_16x16",
"chart_5x3" and "slots" -- the texture charts; "imagetex" and "bumpy" -- the bundled scenes, whose models are copied beside a
drawn images/tiles.exr of the bundled one's size."""
import atexit
import ctypes as C
import functools
import json
import os
import shutil
import tempfile
import zlib

import numpy as np

from goblin_amd import _abi
from goblin_amd import scene as gs
import texture_chart as tc

BIG = "256x128"
SIZES = dict(tc.IMAGES, **{BIG: (256, 128)})
SIZE_IMAGES = [(name, kind) for name in tc.IMAGES for kind in ("color", "float")] + [(BIG, "color")]   # in pool order
CHART_FRAME = dict(resolution=(24, 16), spp=4, depth=3)
BUNDLED_FRAME = dict(resolution=(32, 32), spp=2, depth=3)
CASES = ["sizes", "chart_16x16", "chart_5x3", "slots", "imagetex", "bumpy"]


def draw(w, h, flavour, salt):
    """(h, w, 3) float32 texels that are exact in half floats, seeded by the size, the flavour and `salt`."""
    rng = np.random.RandomState(zlib.crc32(("%dx%d %s %s" % (w, h, flavour, salt)).encode()) & 0x7FFFFFFF)
    shape = (h, w, 3)
    if flavour == "mild":
        return np.ascontiguousarray(rng.randint(0, 32, shape).astype(np.float32) / np.float32(32.0))
    assert flavour == "wide", flavour
    sign = np.where(rng.randint(0, 2, shape) == 1, np.float32(-1.0), np.float32(1.0))
    value = sign * np.ldexp((1.0 + rng.randint(0, 1024, shape) / 1024.0), rng.randint(-14, 16, shape)).astype(np.float32)
    value[rng.randint(0, 8, shape) == 0] = 0.0
    assert (value.astype(np.float16).astype(np.float32) == value).all() and np.isfinite(value).all()
    return np.ascontiguousarray(value, np.float32)


def write_exr(path, img):
    st = _abi.host_lib().gbl_host_write_exr(os.fsencode(path), img.ctypes.data_as(C.c_void_p), img.shape[1], img.shape[0])
    assert st == _abi.GBL_OK, (path, st)


def sizes_doc():
    """One cell per image of SIZE_IMAGES: a colour image under Kd, a float image (channel R, no gamma) under a bump map."""
    doc = tc._base("perspective")
    doc["textures"] += [{"format": "color", "name": "white", "type": "constant", "color": [0.5, 0.5, 0.5]}]
    for k, (name, kind) in enumerate(SIZE_IMAGES):
        t = {"format": kind, "name": "t%d" % k, "type": "image", "file": name + ".exr", "filter": "trilinear", "address": "repeat", "scale": [2.0, 2.0]}
        if kind == "float":
            t.update(channel="R", gamma=1.0)
            doc["materials"].append({"name": "c%d" % k, "type": "lambert", "Kd": "white", "bumpmap": "t%d" % k})
        else:
            doc["materials"].append({"name": "c%d" % k, "type": "lambert", "Kd": "t%d" % k})
        doc["textures"].append(t)
        tc._place(doc, k, "c%d" % k)
    return doc


def _frame(doc, resolution, spp, depth):
    gs._merge(doc, gs.config_overrides(resolution=resolution, spp=spp, depth=depth))
    return doc


_dirs = {}


def _directory(key, fill):
    if key not in _dirs:
        _dirs[key] = tempfile.mkdtemp(prefix="image_edit_")
        atexit.register(shutil.rmtree, _dirs[key], True)
        fill(_dirs[key])
    return _dirs[key]


def chart_dir(flavour, salt):
    """plane.obj and every image of SIZES drawn in `flavour`."""
    def fill(d):
        tc.write_files(d, images=())
        for name, (w, h) in SIZES.items():
            write_exr(os.path.join(d, name + ".exr"), draw(w, h, flavour, salt))
    return _directory(("chart", flavour, salt), fill)


def bundled_dir(doc, salt):
    """The bundled scenes' directory again: the models the document names, and a drawn images/tiles.exr of the bundled one's size."""
    def fill(d):
        os.makedirs(os.path.join(d, "models"))
        os.makedirs(os.path.join(d, "images"))
        for g in doc["geometries"]:
            if "file" in g:
                shutil.copy(os.path.join(gs.SCENE_DIR, g["file"]), os.path.join(d, g["file"]))
        h, w = _abi.read_image(os.path.join(gs.SCENE_DIR, "images", "tiles.exr")).shape[:2]
        write_exr(os.path.join(d, "images", "tiles.exr"), draw(w, h, "mild", salt))
    files = sorted(g["file"] for g in doc["geometries"] if "file" in g)
    return _directory(("bundled", tuple(files), salt), fill)


@functools.lru_cache(maxsize=None)
def pair(case):
    """(scene A, scene B) of a case, loaded once and never written to."""
    if case == "sizes":
        text = json.dumps(_frame(sizes_doc(), **CHART_FRAME))
        return gs.load_scene_text(text, chart_dir("wide", "A")), gs.load_scene_text(text, chart_dir("wide", "B"))
    if case in ("slots", "chart_16x16", "chart_5x3"):
        text = json.dumps(_frame(tc.doc(case[len("chart_"):] if case != "slots" else "slots"), **CHART_FRAME))
        return gs.load_scene_text(text, chart_dir("mild", "A")), gs.load_scene_text(text, chart_dir("mild", "B"))
    assert case in ("imagetex", "bumpy"), case
    with open(gs.scene_path(case)) as f:
        doc = _frame(json.load(f), **BUNDLED_FRAME)
    return gs.load_scene_text(json.dumps(doc), gs.SCENE_DIR), gs.load_scene_text(json.dumps(doc), bundled_dir(doc, "B"))


def pool(scene):
    """The scene's texel pool as the loader built it: a read-only float32 view."""
    n = int(scene.desc.num_texels)
    a = np.ctypeslib.as_array(scene.desc.texels, shape=(n,)) if n else np.zeros(0, np.float32)
    a.flags.writeable = False
    return a


def level_shapes(im):
    return [(max(1, im.height >> l), max(1, im.width >> l), im.channels) for l in range(im.levels)]


def pyramid(scene, image):
    """The image's slice of the pool: its whole pyramid, level 0 first."""
    im = scene.desc.images[image]
    n = sum(h * w * c for h, w, c in level_shapes(im))
    return pool(scene)[im.texel_offset:im.texel_offset + n]


def level0(scene, image):
    """The image's level 0 as (height, width, channels)."""
    im = scene.desc.images[image]
    h, w, c = level_shapes(im)[0]
    return pyramid(scene, image)[:h * w * c].reshape(h, w, c)
