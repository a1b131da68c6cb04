"""TEST INFRASTRUCTURE: generated texture charts -- scenes whose every cell is one way of looking an image up.

Images: texels are integer arithmetic on (x, y, channel), multiples of 1 / 32 in [0.0625, 0.9375] (exact in the EXR's half floats),
written with gbl_host_write_exr into the caller's scene directory.  Their sizes give the pyramids the bundled tiles.exr does not:
one level (1x1), two (2x1), a column and strips whose short side reaches 1 levels before the long one (1x8, 64x4, 4x64), a size
the loader resamples (5x3 -> 8x4) and a square one (16x16).

chart_doc(image, camera): a 4 x 3 grid of plane.obj quads on the floor, each a Lambert whose Kd is that image; columns are the
filters nearest / bilinear / trilinear / EWA, rows (far to near) the address modes repeat / clamp / border.  The camera looks down
the rows at a low angle, and each row's uv scale is about the size of its cells in pixels, so that the footprint of a pixel passes
the width of the whole image inside every cell under the two projective cameras: in front of that line the lookups read the levels
of the pyramid, behind it its 1x1 top.  s and t run from well below -1 to well above 2 across a quad.  The orthographic camera has
one footprint per cell, so it takes another part of the pyramid: a uv scale of (4, 3.4) over cells of 11 x 7 pixels makes every
footprint about 0.4 of the image, two or three levels below the top -- where, on the strips, a level is one texel wide and EWA's
ellipse can miss every texel centre (its weight_sum == 0 fallback).
slot_doc(camera): the same grid with one texture graph or material slot per cell (SLOT_CELLS) on the 16x16 and 5x3 images.
Cells are numbered row-major (row = k // 4, column = k % 4); cell_instances(scene) gives their instance ids.
"""
import atexit
import ctypes as C
import functools
import json
import os
import shutil
import tempfile

import numpy as np

from goblin_amd import _abi
from goblin_amd import scene as gs

IMAGES = {"1x1": (1, 1), "2x1": (2, 1), "1x8": (1, 8), "5x3": (5, 3), "64x4": (64, 4), "4x64": (4, 64), "16x16": (16, 16)}
FILTERS = ["nearest", "bilinear", "trilinear", "EWA"]
MODES = ["repeat", "clamp", "border"]
CAMERAS = ["perspective", "orthographic", "thinlens"]
SHAPE = dict(resolution=(48, 36), spp=4, depth=3)
COLS, ROWS = 4, 3
PITCH = 1.04                      # cell centres; the quads are 1 x 1 (plane.obj is 2 x 2, instanced at scale 0.5)
# A cell's width and depth in pixels under the perspective camera, nearest row first (row 0 of the grid is the farthest).  Its uv
# scale is (width, depth) where the level comes from the footprint's shorter axis (EWA; nearest shares it) and (width / 2, depth)
# where it comes from the longest derivative (trilinear; bilinear, which rounds the level, 0.7 of that): either way that quantity
# is about 1 -- the whole image -- half way up the cell.
ROW_PIXELS = [(14.0, 10.0), (12.0, 6.0), (10.0, 4.0)]
ORTHO_SCALE = (4.0, 3.4)          # every cell under the orthographic camera (11 x 7 pixels): footprints of 0.36 and 0.49


def texels(w, h):
    y, x, c = np.mgrid[0:h, 0:w, 0:3]
    k = 2 + (7 * x + 13 * y + 5 * c + 3 * x * y + 11 * c * x) % 29
    return np.ascontiguousarray(k.astype(np.float32) / np.float32(32.0))


def write_files(scene_dir, images=IMAGES):
    """plane.obj and the chart images into scene_dir."""
    scene_dir = str(scene_dir)
    shutil.copy(os.path.join(gs.SCENE_DIR, "models", "plane.obj"), os.path.join(scene_dir, "plane.obj"))
    for name in images:
        w, h = IMAGES[name]
        img = texels(w, h)
        assert img.min() >= 0.05 and img.max() <= 0.95
        st = _abi.host_lib().gbl_host_write_exr(os.fsencode(os.path.join(scene_dir, name + ".exr")), img.ctypes.data_as(C.c_void_p), w, h)
        assert st == _abi.GBL_OK, (name, st)


def _camera(kind):
    cam = {"type": "perspective", "position": [0.0, 2.0, -2.9], "orientation": [0.9396926, 0.3420201, 0.0, 0.0], "fov": 52.0,   # 40 degrees down
           "near_plane": 0.1, "far_plane": 100.0, "film": {"resolution": list(SHAPE["resolution"])},
           "filter": {"type": "gaussian", "width": [2, 2], "falloff": 2.0}}
    if kind == "orthographic":
        cam.update({"type": "orthographic", "film_width": 4.4})
    elif kind == "thinlens":
        cam.update({"lens_radius": 0.04, "focal_distance": 3.4})
    else:
        assert kind == "perspective", kind
    return cam


def _base(camera):
    return {"render_setting": {"render_method": "path_tracing", "sample_per_pixel": SHAPE["spp"], "max_ray_depth": SHAPE["depth"], "thread_num": 1},
            "camera": _camera(camera),
            "geometries": [{"name": "quad", "type": "mesh", "file": "plane.obj"}],
            "lights": [{"name": "lamp", "type": "point", "intensity": [14.0, 13.0, 12.0], "position": [-0.7, 2.4, -0.9]}],
            "textures": [], "materials": [], "primitives": []}


def _place(doc, k, material):
    row, col = divmod(k, COLS)
    doc["primitives"].append({"type": "model", "name": "m%d" % k, "geometry": "quad", "material": material})
    doc["primitives"].append({"type": "instance", "name": "i%d" % k, "model": "m%d" % k,
                              "position": [PITCH * (col - 0.5 * (COLS - 1)), 0.0, PITCH * (0.5 * (ROWS - 1) - row)],
                              "orientation": [1, 0, 0, 0], "scale": [0.5, 0.5, 0.5]})


def _uv(row, filt, camera):
    """scale and offset of a cell of the row: s and t symmetric about 0.5, so the image's own square lies mid-cell."""
    ks, kt = ROW_PIXELS[ROWS - 1 - row]
    if camera == "orthographic":
        ks, kt = ORTHO_SCALE
    elif filt == "trilinear":
        ks = 0.5 * ks
    elif filt == "bilinear":       # (rounds the level: the top from a footprint of 0.71)
        ks, kt = 0.35 * ks, 0.7 * kt
    return {"scale": [ks, kt], "offset": [0.5 - 0.5 * ks, 0.5 - 0.5 * kt]}


def chart_doc(image, camera="perspective"):
    doc = _base(camera)
    for row, mode in enumerate(MODES):
        for col, filt in enumerate(FILTERS):
            k = row * COLS + col
            doc["textures"].append(dict({"format": "color", "name": "t%d" % k, "type": "image", "file": image + ".exr", "filter": filt, "address": mode},
                                        **_uv(row, filt, camera)))
            doc["materials"].append({"name": "c%d" % k, "type": "lambert", "Kd": "t%d" % k})
            _place(doc, k, "c%d" % k)
    return doc


SLOT_CELLS = ["scale", "checker", "spherical", "gamma", "blinn_Kg", "mirror_Kr", "transparent_Kr", "subsurface_Kr", "mask", "bump", "normal", "bump_normal"]


def slot_doc(camera="perspective"):
    doc = _base(camera)
    T, M = doc["textures"], doc["materials"]
    img = lambda name, file, filt, mode, row, **kw: dict({"format": "color", "name": name, "type": "image", "file": file + ".exr", "filter": filt,
                                                         "address": mode}, **dict(_uv(row, filt, camera), **kw))
    T += [{"format": "color", "name": "white", "type": "constant", "color": [0.9, 0.9, 0.9]},
          {"format": "float", "name": "rough", "type": "constant", "float": 12.0},
          {"format": "float", "name": "half", "type": "constant", "float": 0.5},
          {"format": "float", "name": "amp", "type": "constant", "float": 0.05},
          {"format": "color", "name": "absorb", "type": "constant", "color": [3.0, 0.8, 2.0]},
          {"format": "color", "name": "scatter", "type": "constant", "color": [100.0, 140.0, 120.0]},
          # row 0: texture graphs under a Lambert Kd
          img("a16", "16x16", "trilinear", "repeat", 0),
          dict(img("f53", "5x3", "EWA", "clamp", 0), format="float", channel="G", gamma=1.0),
          {"format": "color", "name": "scaled", "type": "scale", "texture": "a16", "scale": "f53"},
          img("b53", "5x3", "EWA", "repeat", 0),
          {"format": "color", "name": "checker", "type": "checkerboard", "texture1": "a16", "texture2": "b53", "scale": [3.0, 5.0], "offset": [0.25, 0.0],
           "filter": True},
          {"format": "color", "name": "globe", "type": "image", "file": "16x16.exr", "filter": "EWA", "address": "repeat", "mapping": "spherical",
           "position": [PITCH * 0.5, 0.6, -PITCH], "orientation": [0.9238795, 0.3826834, 0, 0], "scale": [0.3, 0.3, 0.3]},
          img("gamma", "5x3", "trilinear", "border", 0, gamma=2.2),
          # row 1: the first colour slot of the other materials
          img("kg", "16x16", "EWA", "clamp", 1),
          img("kr_mirror", "5x3", "trilinear", "repeat", 1),
          img("kr_glass", "16x16", "bilinear", "border", 1),
          img("kr_sss", "5x3", "EWA", "repeat", 1),
          # row 2: behind a mask, and under bump and normal maps
          img("kd_far", "16x16", "EWA", "repeat", 2),
          img("kd_far53", "5x3", "trilinear", "clamp", 2),
          dict(img("bump_img", "16x16", "bilinear", "repeat", 2), format="float", channel="R", gamma=1.0),
          {"format": "float", "name": "bump", "type": "scale", "texture": "bump_img", "scale": "amp"},
          img("nmap", "5x3", "trilinear", "repeat", 2)]
    M += [{"name": "scale", "type": "lambert", "Kd": "scaled"},
          {"name": "checker", "type": "lambert", "Kd": "checker"},
          {"name": "spherical", "type": "lambert", "Kd": "globe"},
          {"name": "gamma", "type": "lambert", "Kd": "gamma"},
          {"name": "blinn_Kg", "type": "blinn", "Kg": "kg", "exponent": "rough", "index": 1.5},
          {"name": "mirror_Kr", "type": "mirror", "Kr": "kr_mirror"},
          {"name": "transparent_Kr", "type": "transparent", "Kr": "kr_glass", "Kt": "white", "index": 1.5},
          {"name": "subsurface_Kr", "type": "subsurface", "absorb": "absorb", "scatter_prime": "scatter", "Kr": "kr_sss", "index": 1.5, "g": 0.4},
          {"name": "wrapped", "type": "lambert", "Kd": "kd_far"},
          {"name": "mask", "type": "mask", "material": "wrapped", "alpha": "half"},
          {"name": "bump", "type": "lambert", "Kd": "kd_far53", "bumpmap": "bump"},
          {"name": "normal", "type": "lambert", "Kd": "kd_far", "normalmap": "nmap"},
          {"name": "bump_normal", "type": "lambert", "Kd": "kd_far53", "bumpmap": "bump", "normalmap": "nmap"}]
    for k, name in enumerate(SLOT_CELLS):
        _place(doc, k, name)
    return doc


CHARTS = list(IMAGES) + ["slots"]


def cell_instances(scene):
    """The instance ids of cells 0..11 (a thin-lens camera puts its lens in front of them in the instance table)."""
    n = scene.desc.num_instances
    assert n in (COLS * ROWS, COLS * ROWS + 1), n
    return list(range(n - COLS * ROWS, n))


def doc(chart, camera="perspective"):
    return slot_doc(camera) if chart == "slots" else chart_doc(chart, camera)


_dir = None


def scene_dir():
    """A scratch scene directory holding plane.obj and every chart image, made once per process."""
    global _dir
    if _dir is None:
        _dir = tempfile.mkdtemp(prefix="texture_chart_")
        atexit.register(shutil.rmtree, _dir, True)
        write_files(_dir)
    return _dir


@functools.lru_cache(maxsize=None)
def scene(chart, camera="perspective", method=None):
    d = doc(chart, camera)
    if method:
        d["render_setting"]["render_method"] = method
    return gs.load_scene_text(json.dumps(d), scene_dir())


@functools.lru_cache(maxsize=None)
def reference(chart, camera="perspective"):
    """aov_reference.Reference of the chart (seed aov_reference.SEED), shared read-only."""
    import aov_reference as ar
    return ar.Reference(scene(chart, camera))


def cell_masks(ref):
    """Per cell, the samples of the reference that hit it."""
    return [ref.instance == i for i in cell_instances(ref.scene)]


# ---------------------------------------------------------------------------
# the cases whose first-hit records are pinned to the compiled reference (tests/test_first_hit_cpu.py, tests/golden/make_golden.py)
# ---------------------------------------------------------------------------
FIRSTHIT_SCENES = ["textured", "imagetex", "bumpy"]
FIRSTHIT_CASES = FIRSTHIT_SCENES + ["chart_" + c for c in CHARTS] + ["chart_%s_orthographic" % c for c in ("1x8", "64x4", "4x64")]   # (the strips' EWA fallback)
FIRSTHIT_SEED = 7
FIRSTHIT_STRIDE = 5          # the fixtures keep every fifth sample (coprime to the 4 samples of a pixel)


def firsthit_case(name):
    """(document, scene directory, image textures the compiled reference must not filter bilinearly, instances left out of its
    comparison).  MIPMap::lookupBilinear rounds the level and MIPMap::lookup clamps it to [0, levels], one past the pyramid, so a
    footprint wider than about 0.7 of the image reads out of bounds in the reference (GoblinTexture.cpp:104-110, 276-277): the
    colour slots that filter bilinearly are looked up `nearest` there and their hits compared in geometry only."""
    if name.startswith("chart_"):
        chart, _, camera = name[len("chart_"):].partition("_")
        d = doc(chart, camera or "perspective")
        if chart == "slots":
            return d, scene_dir(), ["kr_glass"], [SLOT_CELLS.index("transparent_Kr")]
        cells = [k for k in range(COLS * ROWS) if FILTERS[k % COLS] == "bilinear"]
        return d, scene_dir(), ["t%d" % k for k in cells], cells
    with open(gs.scene_path(name)) as f:
        d = json.load(f)
    gs._merge(d, gs.config_overrides(**SHAPE))
    return d, gs.SCENE_DIR, {"imagetex": ["globe_tiles"]}.get(name, []), {"imagetex": [2]}.get(name, [])


def harness_doc(d, directory, not_bilinear=()):
    """The document as the compiled reference loads it: absolute file paths, one thread, the named textures filtered `nearest`."""
    d = json.loads(json.dumps(d))
    d["render_setting"]["thread_num"] = 1
    for section in ("geometries", "textures", "lights"):
        for g in d.get(section, []):
            if "file" in g:
                g["file"] = os.path.join(directory, g["file"])
    for t in d["textures"]:
        if t["name"] in not_bilinear:
            assert t["filter"] == "bilinear", t
            t["filter"] = "nearest"
    return d


def top_texel(scene, image=0):
    """The 1x1 top of an image's pyramid: the last texel of its levels in the host-built pool, as rgb."""
    d = scene.desc
    im = d.images[image]
    total = sum(max(1, im.width >> l) * max(1, im.height >> l) for l in range(im.levels)) * im.channels
    assert max(1, im.width >> (im.levels - 1)) == 1 and max(1, im.height >> (im.levels - 1)) == 1
    if image == d.num_images - 1:
        assert im.texel_offset + total == d.num_texels
    last = np.array([d.texels[im.texel_offset + total - im.channels + c] for c in range(im.channels)], np.float32)
    return last[:3] if im.channels >= 3 else np.repeat(last[:1], 3)
