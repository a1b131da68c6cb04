"""TEST INFRASTRUCTURE: generated medium charts -- small scenes whose every case is one way of meeting the participating medium.

Frame: 24 x 16 pixels, one sample per pixel, box filter of width [0.5, 0.5].  With that filter a pixel receives its own sample and
nothing else (a second addend only where an image position lies exactly on a pixel edge, and two float addends commute), so a Film
pixel IS one sample's w * (tr * L + Lv), bit for bit, in whatever order a device's atomics land: the Film stands in for per-sample
records, which the compiled reference's probes cannot give with a medium present (they log Li, the tile receives tr * L + Lv).

Base scene: a Lambert floor and back wall (plane.obj), a small sphere in the upper part of the region (it ends some camera rays
inside the region and shadows part of it), one point light up to the left.  The region is a box of about [-1, 1]^3 scaled by 0.9 in
front of the wall, narrower than the frame: the outer columns miss it.  Two bases -- `hom` (homogeneous, grey attenuation 0.5) and
`het` (heterogeneous, the 6x5x4 grid) -- and every other case changes one thing (CASES below: name -> (base, what changes)).
Grids are written at test time into a scratch scene directory (Mitsuba float32 .vol, as goblin_amd/scenes/volumes/make_volumes.py),
their values formulas and default_rng with fixed seeds; every grid's file bounds are the non-cubic BOUNDS.

SUMMED: four cases repeated at 4 samples per pixel under the Gaussian filter of width [2, 2] -- the ordinary summed Film and the
stream sampler's chunked walk.
"""
import atexit
import copy
import functools
import json
import os
import shutil
import struct
import tempfile

import numpy as np

from goblin_amd import scene as gs

RESOLUTION = (24, 16)
BOUNDS = ((-1.0, -0.8, -0.9), (1.0, 0.8, 0.9))
CENTRE = [0.0, 1.1, 0.4]
SCALE = [0.9, 0.9, 0.9]
# The thin region: the box itself is thin (a thin SCALE instead would take the transform's determinant below the 1e-5 at which
# the reference's matrix inverse gives up half written -- another subject).  Along an orthographic camera's parallel rays the slab
# is 0.9 * 2 * THIN_Z / cos(11 degrees) = 9.9e-6 thick: 20.8 ulps of the ray parameter there (t in [4, 8), ulp 4.77e-7), and
# float(1e-5) lies between 20 and 21 ulps -- the rounding of tmin and tmax puts crossing rays on either side of the
# (tmax - tmin) < 1e-5f early-out.
THIN_Z = 5.4e-6
THIN_BOUNDS = ((-1.0, -0.8, -THIN_Z), (1.0, 0.8, THIN_Z))
DIAGONAL = 2.0 * 0.9 * float(np.sqrt(1.0 + 0.64 + 0.81))       # of the region in world space, 2.82
DENSITY = 0.5                                                   # the homogeneous base's attenuation and the 1x1x1 grid's one voxel


# ---------------------------------------------------------------------------
# grids
# ---------------------------------------------------------------------------
def grid(name):
    """(nz, ny, nx, channels) float32."""
    if name == "1x1x1":
        return np.full((1, 1, 1, 1), DENSITY, np.float32)
    if name == "2x1x1":
        return np.array([0.9, 0.25], np.float32).reshape(1, 1, 2, 1)
    if name == "1x1x8":
        z, c = np.mgrid[0:8, 0:3]
        return (0.15 + ((3 * z + 5 * c) % 7) / 8.0).astype(np.float32).reshape(8, 1, 1, 3)
    if name == "5x3x2":
        return np.random.default_rng(532).uniform(0.05, 1.2, (2, 3, 5, 3)).astype(np.float32)
    if name == "16x16x16":     # a slab of exact zeros through the middle and one octant of exact zeros
        z, y, x = np.mgrid[0:16, 0:16, 0:16]
        d = 0.3 + 0.9 * np.random.default_rng(16).random((16, 16, 16)) + 0.4 * np.sin(0.7 * x + 0.3 * z)
        d[:, 7:9, :] = 0.0
        d[8:, 8:, 8:] = 0.0
        return d.astype(np.float32)[..., None]
    assert name == "6x5x4", name
    z, y, x = np.mgrid[0:4, 0:5, 0:6]
    d = 0.2 + 1.3 * np.exp(-0.25 * ((x - 2.5) ** 2 + (y - 2.0) ** 2 + 2.0 * (z - 1.5) ** 2)) * (0.8 + 0.4 * np.random.default_rng(654).random((4, 5, 6)))
    return d.astype(np.float32)[..., None]


GRIDS = ["6x5x4", "1x1x1", "2x1x1", "1x1x8", "5x3x2", "16x16x16"]


def write_vol(path, data, lo, hi):
    nz, ny, nx, nch = data.shape
    with open(path, "wb") as f:
        f.write(b"VOL\x03")
        f.write(struct.pack("<5i", 1, nx, ny, nz, nch))
        f.write(struct.pack("<6f", *lo, *hi))
        f.write(np.ascontiguousarray(data, np.float32).tobytes())


def write_files(scene_dir):
    """plane.obj, env.exr and every grid into scene_dir."""
    scene_dir = str(scene_dir)
    shutil.copy(os.path.join(gs.SCENE_DIR, "models", "plane.obj"), os.path.join(scene_dir, "plane.obj"))
    shutil.copy(os.path.join(gs.SCENE_DIR, "images", "env.exr"), os.path.join(scene_dir, "env.exr"))
    for name in GRIDS:
        write_vol(os.path.join(scene_dir, name + ".vol"), grid(name), *BOUNDS)
    write_vol(os.path.join(scene_dir, "thin.vol"), grid("6x5x4"), *THIN_BOUNDS)


_dir = None


def scene_dir():
    """A scratch scene directory holding the charts' files, made once per process."""
    global _dir
    if _dir is None:
        _dir = tempfile.mkdtemp(prefix="medium_chart_")
        atexit.register(shutil.rmtree, _dir, True)
        write_files(_dir)
    return _dir


# ---------------------------------------------------------------------------
# the base scene
# ---------------------------------------------------------------------------
DOWN = [0.0, 1.0, 0.0, 0.0]                     # plane.obj's +y normal turned to -y
DISK_DOWN = [0.70710678, 0.70710678, 0.0, 0.0]  # a disk's +z normal turned to -y
POINT_OUT = {"name": "lamp", "type": "point", "intensity": [30.0, 28.0, 25.0], "position": [-1.4, 3.0, -1.2]}


def _area(geometry, position, scale, orientation=DOWN, radiance=(40.0, 36.0, 30.0)):
    return {"name": "emitter", "type": "area", "geometry": geometry, "radiance": list(radiance), "position": position,
            "orientation": orientation, "scale": [scale] * 3}


LIGHTS = {
    "point_in": [{"name": "lamp", "type": "point", "intensity": [3.0, 2.8, 2.5], "position": [-0.3, 1.3, 0.5]}],
    "spot": [{"name": "lamp", "type": "spot", "intensity": [60.0, 56.0, 50.0], "position": [-1.4, 3.0, -1.2], "target": [-0.5, 1.1, 0.4],
              "theta_max": 16.0, "falloff_start": 10.0}],     # the cone's edge runs through the region
    "directional": [{"name": "sun", "type": "directional", "radiance": [1.5, 1.4, 1.2], "direction": [0.3713907, -0.8355491, 0.4053267]}],
    "quad_out": [_area("quad", [-0.4, 2.9, 0.2], 0.4)],
    "quad_in": [_area("quad", [-0.3, 1.55, 0.5], 0.15)],
    "sphere_in": [_area("ball", [-0.35, 1.45, 0.5], 0.1, [1.0, 0.0, 0.0, 0.0])],
    "sphere_out": [_area("ball", [-1.3, 2.6, -0.6], 0.2, [1.0, 0.0, 0.0, 0.0])],
    "disk_in": [_area("plate", [-0.3, 1.55, 0.5], 0.2, DISK_DOWN)],
    "disk_out": [_area("plate", [-0.4, 2.9, 0.2], 0.5, DISK_DOWN)],
    "ibl": [{"name": "sky", "type": "ibl", "file": "env.exr", "filter": [0.9, 0.8, 0.7], "orientation": [0.9238795, 0.0, 0.3826834, 0.0],
             "sample_num": 2}],
    # light 0 has no power: Scene's power distribution never picks it
    "two": [{"name": "dark", "type": "point", "intensity": [0.0, 0.0, 0.0], "position": [0.8, 2.5, -0.5]}, POINT_OUT],
    "none": [],
}


def _camera(kind, position=(0.0, 1.3, -4.4)):
    cam = {"type": "perspective", "position": list(position), "orientation": [0.9953962, 0.0958458, 0.0, 0.0], "fov": 28.0,   # 11 degrees down
           "near_plane": 0.1, "far_plane": 100.0, "film": {"resolution": list(RESOLUTION)}, "filter": {"type": "box", "width": [0.5, 0.5]}}
    if kind == "orthographic":
        cam.update({"type": "orthographic", "film_width": 3.4})
    elif kind == "thinlens":
        cam.update({"lens_radius": 0.06, "focal_distance": 4.6})
    else:
        assert kind == "perspective", kind
    return cam


def _volume(base):
    v = {"albedo": [0.85, 0.8, 0.7], "emission": [0.0, 0.0, 0.0], "g": 0.3, "sample_num": 2, "position": list(CENTRE),
         "orientation": [1.0, 0.0, 0.0, 0.0], "scale": list(SCALE)}
    if base == "hom":
        v.update({"type": "homogeneous", "attenuation": [DENSITY] * 3, "box_min": list(BOUNDS[0]), "box_max": list(BOUNDS[1])})
    else:
        assert base == "het", base
        v.update({"type": "heterogeneous", "density_grid": "6x5x4.vol", "step_size": 0.45})
    return v


def _base(base):
    return {"render_setting": {"render_method": "path_tracing", "sample_per_pixel": 1, "max_ray_depth": 3, "thread_num": 1},
            "camera": _camera("perspective"),
            "volume": _volume(base),
            "geometries": [{"name": "quad", "type": "mesh", "file": "plane.obj"}, {"name": "ball", "type": "sphere", "radius": 1.0},
                           {"name": "plate", "type": "disk", "radius": 1.0}],
            "textures": [{"format": "color", "name": "white", "type": "constant", "color": [0.75, 0.75, 0.75]},
                         {"format": "color", "name": "ochre", "type": "constant", "color": [0.7, 0.5, 0.2]}],
            "materials": [{"name": "white", "type": "lambert", "Kd": "white"}, {"name": "ochre", "type": "lambert", "Kd": "ochre"}],
            "primitives": [{"type": "model", "name": "m_quad", "geometry": "quad", "material": "white"},
                           {"type": "model", "name": "m_ball", "geometry": "ball", "material": "ochre"},
                           {"type": "instance", "name": "floor", "model": "m_quad", "position": [0, 0, 0], "orientation": [1, 0, 0, 0], "scale": [4, 4, 4]},
                           {"type": "instance", "name": "wall", "model": "m_quad", "position": [0, 2.0, 2.0],
                            "orientation": [0.70710678, -0.70710678, 0, 0], "scale": [4, 4, 4]},
                           {"type": "instance", "name": "occluder", "model": "m_ball", "position": [0.3, 1.5, 0.2], "orientation": [1, 0, 0, 0],
                            "scale": [0.22, 0.22, 0.22]}],
            "lights": [copy.deepcopy(POINT_OUT)]}


# ---------------------------------------------------------------------------
# what a case changes
# ---------------------------------------------------------------------------
def _set_volume(**kw):
    return lambda d: d["volume"].update(kw)


def _set_render(**kw):
    return lambda d: d["render_setting"].update(kw)


def _lights(name):
    def f(d):
        d["lights"] = copy.deepcopy(LIGHTS[name])
    return f


def _camera_kind(kind):
    def f(d):
        d["camera"] = _camera(kind)
    return f


def _inside(d):          # the camera inside the region
    d["camera"] = _camera("perspective", (0.0, 1.2, -0.25))


def _clipped(d):         # an opaque sphere at the region's centre: the rays that meet it end inside the region
    d["primitives"].append({"type": "instance", "name": "core", "model": "m_ball", "position": list(CENTRE), "orientation": [1, 0, 0, 0],
                            "scale": [0.55, 0.55, 0.55]})


def _behind(d):          # wholly behind the wall: every camera ray ends before the region
    d["volume"]["position"] = [0.0, 1.1, 3.5]


def _thin(d):
    d["camera"] = _camera("orthographic")
    if d["volume"]["type"] == "homogeneous":
        d["volume"].update({"box_min": list(THIN_BOUNDS[0]), "box_max": list(THIN_BOUNDS[1])})
    else:
        d["volume"]["density_grid"] = "thin.vol"


def _rotated(d):         # a quaternion plus non-uniform scale
    d["volume"]["orientation"] = [0.8804762, 0.2798481, 0.3647052, 0.1159169]
    d["volume"]["scale"] = [0.7, 1.0, 0.55]


def _grid(name):
    return _set_volume(density_grid=name + ".vol")


CASES = {
    # the bases: placement `through`, path tracer, perspective camera, point light outside the region
    "hom": ("hom", None),
    "het": ("het", None),
    # grids
    "het_grid_1x1x1": ("het", _grid("1x1x1")),
    "het_grid_2x1x1": ("het", _grid("2x1x1")),
    "het_grid_1x1x8": ("het", _grid("1x1x8")),
    "het_grid_5x3x2": ("het", _grid("5x3x2")),
    "het_grid_16x16x16": ("het", _grid("16x16x16")),
    # placement
    "hom_inside": ("hom", _inside), "het_inside": ("het", _inside),
    "hom_clipped": ("hom", _clipped), "het_clipped": ("het", _clipped),
    "hom_behind": ("hom", _behind), "het_behind": ("het", _behind),
    "hom_thin": ("hom", _thin), "het_thin": ("het", _thin),
    "hom_rotated": ("hom", _rotated), "het_rotated": ("het", _rotated),
    # march length: longer than the region's diagonal, about one cell of the base grid, diagonal / 200
    "het_step_long": ("het", _set_volume(step_size=3.5)),
    "het_step_cell": ("het", _set_volume(step_size=0.3)),
    "het_step_fine": ("het", _set_volume(step_size=DIAGONAL / 200.0)),
    # lights
    "het_light_point_in": ("het", _lights("point_in")),
    "het_light_spot": ("het", _lights("spot")),
    "het_light_directional": ("het", _lights("directional")),
    "het_light_quad_out": ("het", _lights("quad_out")), "het_light_quad_in": ("het", _lights("quad_in")),
    "het_light_sphere_in": ("het", _lights("sphere_in")), "het_light_disk_out": ("het", _lights("disk_out")),
    "het_light_ibl": ("het", _lights("ibl")),
    "het_light_two": ("het", _lights("two")),
    "het_light_none": ("het", _lights("none")),
    "het_light_none_whitted": ("het", lambda d: (_lights("none")(d), _set_render(render_method="whitted", max_ray_depth=2)(d))),
    "het_light_none_ao": ("het", lambda d: (_lights("none")(d), _set_render(render_method="ao", ao_sample_num=4)(d))),
    "hom_light_quad_in": ("hom", _lights("quad_in")), "hom_light_quad_out": ("hom", _lights("quad_out")),
    "hom_light_sphere_out": ("hom", _lights("sphere_out")), "hom_light_disk_in": ("hom", _lights("disk_in")),
    "hom_light_spot": ("hom", _lights("spot")),
    "hom_light_two": ("hom", _lights("two")),
    "hom_light_none": ("hom", _lights("none")),
    # medium parameters
    "hom_g_0": ("hom", _set_volume(g=0.0)), "hom_g_0.6": ("hom", _set_volume(g=0.6)), "hom_g_-0.6": ("hom", _set_volume(g=-0.6)),
    "hom_g_0.95": ("hom", _set_volume(g=0.95)),
    "het_g_0.6": ("het", _set_volume(g=0.6)), "het_g_-0.6": ("het", _set_volume(g=-0.6)), "het_g_0.95": ("het", _set_volume(g=0.95)),
    "hom_samples_1": ("hom", _set_volume(sample_num=1)), "hom_samples_3": ("hom", _set_volume(sample_num=3)),
    "hom_coloured": ("hom", _set_volume(attenuation=[0.9, 0.45, 0.15])),
    "hom_clear": ("hom", _set_volume(attenuation=[0.0, 0.0, 0.0])),      # 0 / 0 in the distance sampling: NaN samples, dropped by the splat
    # integrators (the path tracer at depth 3 is the base)
    "hom_whitted": ("hom", _set_render(render_method="whitted", max_ray_depth=2)), "het_whitted": ("het", _set_render(render_method="whitted", max_ray_depth=2)),
    "hom_ao": ("hom", _set_render(render_method="ao", ao_sample_num=4)), "het_ao": ("het", _set_render(render_method="ao", ao_sample_num=4)),
    # cameras (perspective is the base)
    "hom_orthographic": ("hom", _camera_kind("orthographic")), "het_orthographic": ("het", _camera_kind("orthographic")),
    "hom_thinlens": ("hom", _camera_kind("thinlens")), "het_thinlens": ("het", _camera_kind("thinlens")),
}
# No case was dropped: the compiled reference runs every one of them.

# the summed cases: name -> the spp-1 case they repeat at 4 samples per pixel under the Gaussian filter
SUMMED = {"sum_het": "het", "sum_het_clipped": "het_clipped", "sum_hom": "hom", "sum_het_whitted": "het_whitted"}
ALL_CASES = list(CASES) + list(SUMMED)
EMITTER_CASES = [c for c in CASES if "_light_" in c and c.rsplit("_", 2)[-2] in ("quad", "sphere", "disk")]
PATH_CASES = [c for c in ALL_CASES if not c.endswith(("_whitted", "_ao"))]


def doc(case):
    summed = case in SUMMED
    base, change = CASES[SUMMED.get(case, case)]
    d = _base(base)
    if change:
        change(d)
    if summed:
        d["render_setting"]["sample_per_pixel"] = 4
        d["camera"]["filter"] = {"type": "gaussian", "width": [2, 2], "falloff": 2.0}
    return d


def clear_doc(case):
    """The case without its medium: the scene whose replay gives L."""
    d = doc(case)
    del d["volume"]
    return d


@functools.lru_cache(maxsize=None)
def scene(case, clear=False):
    return gs.load_scene_text(json.dumps(clear_doc(case) if clear else doc(case)), scene_dir())


def harness_doc(case, directory):
    """The document as the compiled reference loads it: absolute file paths, one thread."""
    d = doc(case)
    d["render_setting"]["thread_num"] = 1
    for section in ("geometries", "lights"):
        for g in d[section]:
            if "file" in g:
                g["file"] = os.path.join(directory, g["file"])
    if "density_grid" in d["volume"]:
        d["volume"]["density_grid"] = os.path.join(directory, d["volume"]["density_grid"])
    return d


GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def golden(case):
    """tests/golden/medium_<case>.npz (tests/golden/make_medium_golden.py): the compiled reference's film, samples (n, 4) and li,
    shared read-only."""
    with np.load(os.path.join(GOLDEN_DIR, "medium_" + case + ".npz")) as z:
        out = {k: z[k] for k in ("film", "samples", "li")}
    for a in out.values():
        a.setflags(write=False)
    return out


def same_bits(a, b):
    """Float arrays equal bit for bit, NaN positions equal (a NaN's payload is not compared)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def pixel_report(case, film, ref, limit=8):
    """The pixels at which two Films differ, for an assertion message: case, coordinates, both values."""
    bad = np.argwhere((film.view(np.uint32) != ref.view(np.uint32)).any(axis=-1))
    return "\n".join("%s pixel (x %d, y %d): %r != %r" % (case, x, y, film[y, x].tolist(), ref[y, x].tolist()) for y, x in bad[:limit]) \
        + ("\n... %d pixels in all" % len(bad) if len(bad) > limit else "")
