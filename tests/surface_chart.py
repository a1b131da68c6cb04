"""TEST INFRASTRUCTURE: generated surface charts -- small scenes whose every case is one way of meeting the materials
(mat_bsdf / mat_pdf / mat_sample, the Blinn lobe, the two Fresnel terms), the lights (light_sample, light_pdf, the area shapes,
hit_Le, environment_le) and the sphere and disk tests.

Frame: 24 x 16 pixels, one sample per pixel, box filter of width [0.5, 0.5] (tests/medium_chart.py's frame): a pixel receives its own
sample and nothing else, so a Film pixel IS one sample's w * Li bit for bit, in whatever order a device's atomics land.

Four bases, and every other case changes one thing (CASES below: name -> (base, what changes)):
  `lean`  the path tracer at max_ray_depth 2, where Li = Le + one vertex's light sample + its BSDF sample.  Meshes only (plane.obj,
          cube.obj), constant colours, a pinhole camera, one point light: a Lambert floor and back wall and a row of four cubes in
          Lambert, Blinn, transparent and mirror, each covering twenty pixels or more.  Nothing in it sets DevScene::extended
          (scene_prep.cpp), so the native sampler runs the lean kernels and the primary pass (api_render.hip's lean_native).
  `ext`   the same with a sphere and a disk above the row: extended == 1, the EXT kernels.
  `deep`  `lean` at max_ray_depth 6 -- paths enter and leave the glass cube, and meet total internal reflection on the way out --
          with a fifth cube above the row under a mask material (alpha 0.5 over Lambert).
  `wh`    Whitted at depth 3 over `ext`: whitted.h has its own light loop and its own specular recursion.

Lean twins: for every `lean`-based case `<case>+ext` is the same document plus one sphere model far below the floor, where no ray of
the case reaches it.  The twin resolves to the EXT kernels and must give the case's li bit for bit (asserted on the oracle; a twin
needs no fixture of its own).

An image based light needs sky to show: the cases that use one also take the back wall away (`_sky`).

SUMMED: four cases repeated at 4 samples per pixel under the Gaussian filter of width [2, 2] (`sum_*`).
"""
import atexit
import copy
import functools
import json
import os
import shutil
import tempfile

import numpy as np

from goblin_amd import scene as gs
from sss_chart import _quat, _quat_from_to, same_bits, film_report, sample_report   # noqa: F401  (shared with the sibling charts)

RESOLUTION = (24, 16)
CAMERA_AT = (0.0, 1.3, -4.4)
ROW = {"lambert": -1.35, "blinn": -0.45, "glass": 0.45, "mirror": 1.35}      # the cubes' x; z 0.3, 0.6 wide and 0.7 high, turned 30 degrees
CUBE_TURN = _quat([0, 1, 0], 30.0)
CUBE_Y, CUBE_SCALE = 0.37, [0.6, 0.7, 0.6]
LAMP_AT = [-1.4, 3.0, -1.2]
DOWN = [0.0, 1.0, 0.0, 0.0]                       # plane.obj's +y normal turned to -y
TO_CAMERA = [0.70710678, -0.70710678, 0.0, 0.0]   # plane.obj's +y normal turned to -z
FROM_CAMERA = [0.70710678, 0.70710678, 0.0, 0.0]  # ... to +z
DISK_DOWN = [0.70710678, 0.70710678, 0.0, 0.0]    # a disk's +z normal turned to -y
DISK_UP = [0.70710678, -0.70710678, 0.0, 0.0]     # ... to +y
BALL_AT = [-0.9, 1.35, 0.5]
FAR_BELOW = [0.0, -60.0, 0.0]                     # the twin's sphere


def write_files(scene_dir):
    scene_dir = str(scene_dir)
    for f in ("plane.obj", "cube.obj"):
        shutil.copy(os.path.join(gs.SCENE_DIR, "models", f), os.path.join(scene_dir, f))
    shutil.copy(os.path.join(gs.SCENE_DIR, "images", "env.exr"), os.path.join(scene_dir, "env.exr"))


_dir = None


def scene_dir():
    """A scratch scene directory holding the charts' files, made once per process."""
    global _dir
    if _dir is None:
        _dir = tempfile.mkdtemp(prefix="surface_chart_")
        atexit.register(shutil.rmtree, _dir, True)
        write_files(_dir)
    return _dir


# ---------------------------------------------------------------------------
# the base scenes
# ---------------------------------------------------------------------------
POINT = {"name": "lamp", "type": "point", "intensity": [30.0, 28.0, 25.0], "position": LAMP_AT}


def _area(geometry, position, scale, orientation=DOWN, radiance=(40.0, 36.0, 30.0), name="emitter", **kw):
    return dict({"name": name, "type": "area", "geometry": geometry, "radiance": list(radiance), "position": list(position),
                 "orientation": list(orientation), "scale": [scale] * 3}, **kw)


def _spot(theta_max, falloff_start, position=LAMP_AT, target=(0.0, 0.3, 0.3)):
    return [{"name": "lamp", "type": "spot", "intensity": [60.0, 56.0, 50.0], "position": list(position), "target": list(target),
             "theta_max": theta_max, "falloff_start": falloff_start}]


def _ibl(orientation=(0.9238795, 0.0, 0.3826834, 0.0), sample_num=1):
    return [{"name": "sky", "type": "ibl", "file": "env.exr", "filter": [0.9, 0.8, 0.7], "orientation": list(orientation), "sample_num": sample_num}]


LIGHTS = {
    # the cone's edge (18 degrees) and the falloff's start (8) both run across the row of cubes, 3.4 away
    "spot": _spot(18.0, 8.0),
    "spot_no_falloff": _spot(18.0, 18.0),           # falloff_start == theta_max: the two comparisons leave no falloff zone but cos == both
    "spot_falloff_0": _spot(18.0, 0.0),             # cos_falloff 1: `cos > 1` never holds, all of the cone is falloff
    "spot_90": _spot(90.0, 10.0),                   # cos_max = cos(90 degrees) in float: 6e-17 in double, -4.4e-8 after the float radians
    "spot_in_glass": _spot(50.0, 35.0, position=[ROW["glass"], CUBE_Y, 0.3], target=[ROW["glass"], CUBE_Y, -2.0]),
    "directional": [{"name": "sun", "type": "directional", "radiance": [1.5, 1.4, 1.2], "direction": [0.3713907, -0.8355491, 0.4053267]}],
    "quad": [_area("quad", [-0.5, 2.6, -0.4], 0.4)],
    "quad_behind": [_area("quad", [-0.5, 2.6, -0.4], 0.4, [1.0, 0.0, 0.0, 0.0])],      # its normal points up: every L is black
    "quad_edge_on": [_area("quad", [5.0, 0.0, 0.0], 0.4, [1.0, 0.0, 0.0, 0.0])],       # in the floor's plane, beside the floor
    "cube": [_area("cube", [-0.5, 2.6, -0.4], 0.5, [1.0, 0.0, 0.0, 0.0])],             # twelve triangles: the cdf pick
    "sphere": [_area("ball", [-1.2, 2.4, -0.8], 0.2, [1.0, 0.0, 0.0, 0.0])],
    "sphere_around": [_area("ball", [ROW["lambert"], CUBE_Y, 0.3], 0.62, [1.0, 0.0, 0.0, 0.0], radiance=(2.0, 1.8, 1.5))],   # contains the Lambert cube
    "disk": [_area("plate", [-0.5, 2.6, -0.4], 0.5, DISK_DOWN)],
    "disk_edge_on": [_area("plate", [5.0, 0.0, 0.0], 0.5, DISK_UP)],
    # in view, between the row and the wall
    "emitter_front": [_area("quad", [0.0, 1.3, 1.2], 0.35, TO_CAMERA, radiance=(4.0, 3.6, 3.0))],
    "emitter_back": [_area("quad", [0.0, 1.3, 1.2], 0.35, FROM_CAMERA, radiance=(4.0, 3.6, 3.0))],
    # two large quads overhead: a BSDF sample from the floor lands on either, whichever was picked
    "two_emitters": [_area("quad", [-1.2, 2.6, 0.0], 1.0, radiance=(4.0, 3.6, 3.0), name="left"),
                     _area("quad", [1.2, 2.6, 0.0], 1.0, radiance=(3.0, 3.6, 4.0), name="right")],
    "ibl": _ibl(),
    "ibl_3": _ibl(sample_num=3),
    "ibl_pole": _ibl(orientation=(1.0, 0.0, 0.0, 0.0)),      # the map's pole is its frame's z: the direction the camera looks in
    "two": [{"name": "dark", "type": "point", "intensity": [0.0, 0.0, 0.0], "position": [0.8, 2.5, -0.5]}, POINT],
    "three": [{"name": "a", "type": "point", "intensity": [6.0, 6.0, 6.0], "position": [1.5, 2.5, -1.5]}, POINT,
              {"name": "c", "type": "point", "intensity": [12.0, 14.0, 16.0], "position": [0.2, 3.2, 0.2]}],
    "none": [],
    # exactly in the floor's plane, in front of the row: dot(n, wi) is exactly 0 at the floor samples whose y is exactly 0 (most)
    "in_plane": [dict(POINT, position=[0.3, 0.0, -1.2], intensity=[3.0, 2.8, 2.5])],
    # 1e-4 above the floor, in view: in_plane's contrast, lit under cosines of 1e-4 (no drawn sample comes within its 4e-3 epsilon)
    "near_floor": [dict(POINT, position=[0.3, 1e-4, -1.2], intensity=[3.0, 2.8, 2.5])],
}


def _camera(kind):
    cam = {"type": "perspective", "position": list(CAMERA_AT), "orientation": [0.9986295, 0.0523360, 0.0, 0.0], "fov": 28.0,   # 6 degrees down
           "near_plane": 0.1, "far_plane": 100.0, "film": {"resolution": list(RESOLUTION)}, "filter": {"type": "box", "width": [0.5, 0.5]}}
    if kind == "orthographic":
        cam.update({"type": "orthographic", "film_width": 3.6})
    elif kind == "thinlens":
        cam.update({"lens_radius": 0.06, "focal_distance": 4.7})
    else:
        assert kind == "perspective", kind
    return cam


def _constant(name, color):
    return {"format": "color", "name": name, "type": "constant", "color": list(color)}


def _float(name, value):
    return {"format": "float", "name": name, "type": "constant", "float": value}


def _instance(name, model, position, orientation=(1, 0, 0, 0), scale=(1, 1, 1)):
    return {"type": "instance", "name": name, "model": model, "position": list(position), "orientation": list(orientation), "scale": list(scale)}


def _model(name, geometry, material):
    return {"type": "model", "name": name, "geometry": geometry, "material": material}


def _add_model(d, name, geometry, material):
    """Models go before the instances that use them."""
    first = next(i for i, p in enumerate(d["primitives"]) if p["type"] == "instance")
    d["primitives"].insert(first, _model(name, geometry, material))


def _base(base):
    d = {"render_setting": {"render_method": "path_tracing", "sample_per_pixel": 1, "max_ray_depth": 2, "thread_num": 1},
         "camera": _camera("perspective"),
         "geometries": [{"name": "quad", "type": "mesh", "file": "plane.obj"}, {"name": "cube", "type": "mesh", "file": "cube.obj"}],
         "textures": [_constant("white", [0.75, 0.75, 0.75]), _constant("ochre", [0.7, 0.5, 0.2]), _constant("gold", [0.9, 0.7, 0.3]),
                      _constant("full", [0.95, 0.95, 0.95]), _constant("tint", [0.7, 0.9, 0.8]), _constant("black", [0.0, 0.0, 0.0]),
                      _constant("one", [1.0, 1.0, 1.0]), _float("exponent", 20.0), _float("alpha", 0.5)],
         "materials": [{"name": "white", "type": "lambert", "Kd": "white"}, {"name": "lambert", "type": "lambert", "Kd": "ochre"},
                       {"name": "blinn", "type": "blinn", "Kg": "gold", "exponent": "exponent", "index": 1.5},
                       {"name": "glass", "type": "transparent", "Kr": "full", "Kt": "tint", "index": 1.5},
                       {"name": "mirror", "type": "mirror", "Kr": "full"}],
         "primitives": [_model("m_quad", "quad", "white")] + [_model("m_" + k, "cube", k) for k in ROW] +
                       [_instance("floor", "m_quad", [0, 0, 0], scale=[4, 4, 4]),
                        _instance("wall", "m_quad", [0, 2.0, 2.0], TO_CAMERA, [4, 4, 4])] +
                       [_instance(k, "m_" + k, [x, CUBE_Y, 0.3], CUBE_TURN, CUBE_SCALE) for k, x in ROW.items()],
         "lights": [copy.deepcopy(POINT)]}
    if base in ("ext", "wh"):
        d["geometries"] += [{"name": "ball", "type": "sphere", "radius": 1.0}, {"name": "plate", "type": "disk", "radius": 1.0}]
        _add_model(d, "m_ball", "ball", "blinn")
        _add_model(d, "m_plate", "plate", "lambert")
        d["primitives"] += [_instance("ball", "m_ball", [-0.9, 1.35, 0.5], scale=[0.45, 0.45, 0.45]),
                            _instance("plate", "m_plate", [0.9, 1.3, 0.5], _quat_from_to([0, 0, 1], [-0.3, 0.4, -1.0]), [0.36, 0.36, 0.36])]
        if base == "wh":
            d["render_setting"].update({"render_method": "whitted", "max_ray_depth": 3})
    elif base == "deep":
        d["render_setting"]["max_ray_depth"] = 6
        d["materials"].append({"name": "masked", "type": "mask", "material": "lambert", "alpha": "alpha"})
        _add_model(d, "m_masked", "cube", "masked")
        d["primitives"].append(_instance("masked", "m_masked", [0.0, 1.3, 0.5], CUBE_TURN, [0.6, 0.6, 0.6]))
    else:
        assert base == "lean", base
    return d


# ---------------------------------------------------------------------------
# what a case changes
# ---------------------------------------------------------------------------
def _find(d, section, name):
    return next(x for x in d[section] if x["name"] == name)


def _mat(name, **kw):
    return lambda d: _find(d, "materials", name).update(kw)


def _tex(name, **kw):
    return lambda d: _find(d, "textures", name).update(kw)


def _set_render(**kw):
    return lambda d: d["render_setting"].update(kw)


def _sky(d):
    d["primitives"] = [p for p in d["primitives"] if p["name"] != "wall"]


def _lights(name, **kw):
    def f(d):
        d["lights"] = copy.deepcopy(LIGHTS[name])
        for light in d["lights"]:
            light.update(kw)
        if name.startswith("ibl"):
            _sky(d)
        needs = {x["geometry"] for x in d["lights"] if "geometry" in x} - {g["name"] for g in d["geometries"]}
        d["geometries"] += [g for g in ({"name": "ball", "type": "sphere", "radius": 1.0}, {"name": "plate", "type": "disk", "radius": 1.0})
                            if g["name"] in needs]
    return f


def _camera_kind(kind):
    def f(d):
        d["camera"] = _camera(kind)
    return f


def _both(*changes):
    def f(d):
        for c in changes:
            c(d)
    return f


def _grazing_pane(d):     # a glass quad through the frame's middle whose plane nearly holds the camera: cosines of a few hundredths
    _add_model(d, "m_pane", "quad", "glass")
    d["primitives"].append(_instance("pane", "m_pane", [0.16, 1.3, 0.0], _quat_from_to([0, 1, 0], [-1.0, 0.0, -0.02]), [0.7, 0.7, 1.8]))


def _light_on_vertex(d):  # a small axis-aligned step just above the floor, and the lamp exactly on one of its corners
    d["primitives"].append(_instance("step", "m_quad", [0.0, 0.0625, -1.5], scale=[0.5, 0.5, 0.5]))
    d["lights"] = [dict(POINT, position=[0.5, 0.0625, -1.0], intensity=[3.0, 2.8, 2.5])]


def _light_inside_epsilon(d):
    """The same frame from 400 units away (a field of view of a third of a degree): a fragment's epsilon, 1e-3 t, is 0.4, wider than
    two pixels, and the lamp stands 0.05 in front of the wall -- for the wall's fragments within 0.4 of it the shadow ray's
    maxt = dist - epsilon is negative."""
    d["camera"].update({"position": [0.0, 42.62, -397.53], "fov": 0.3438, "far_plane": 1000.0})
    d["lights"] = [dict(POINT, position=[-0.6, 1.6, 1.95], intensity=[3.0, 2.8, 2.5])]


def _facing_mirrors(d):   # two upright mirrors either side of the frame's middle, facing each other across the Blinn and glass cubes
    _add_model(d, "m_wide", "quad", "mirror")
    d["primitives"] += [_instance("mirror_l", "m_wide", [-0.95, 0.9, 0.3], _quat_from_to([0, 1, 0], [1.0, 0.0, -0.12]), [0.8, 0.8, 0.8]),
                        _instance("mirror_r", "m_wide", [0.95, 0.9, 0.3], _quat_from_to([0, 1, 0], [-1.0, 0.0, -0.12]), [0.8, 0.8, 0.8])]


def _shape(name, **kw):
    return lambda d: _find(d, "primitives", name).update(kw)


def _camera_in_sphere(d):  # a Lambert sphere of radius 12 around everything, the camera included
    _add_model(d, "m_shell", "ball", "white")
    d["primitives"].append(_instance("shell", "m_shell", [0.0, 1.0, 0.0], scale=[12.0, 12.0, 12.0]))
    _sky(d)


def _masked(inner, alpha):
    def f(d):
        _find(d, "materials", "masked")["material"] = inner
        _find(d, "textures", "alpha")["float"] = alpha
        _lights("ibl")(d)
    return f


def _stacked_masks(d):    # two masked quads one behind the other, between the lamp and the wall: a shadow ray from the wall walks both
    _add_model(d, "m_veil", "quad", "masked")
    d["primitives"] += [_instance("veil%d" % k, "m_veil", [-0.6, 1.6, 0.9 + 0.3 * k], TO_CAMERA, [0.7, 0.7, 0.5]) for k in range(2)]


def _mask_before_sky(d):  # the masked cube alone in front of the sky: a punched-through camera path escapes at bounce 0
    _lights("ibl")(d)
    _find(d, "primitives", "masked").update({"position": [0.0, 1.35, 0.5], "scale": [1.6, 0.9, 0.3]})


def _mask_behind_mirror(d):   # ... and a mirror in the frame's upper left that shows it: the same escape, at bounce 1 -- no environment
    _mask_before_sky(d)
    _add_model(d, "m_wide", "quad", "mirror")
    _find(d, "primitives", "masked").update({"position": [1.0, 1.35, 0.5], "scale": [1.2, 0.9, 0.3]})
    d["primitives"].append(_instance("looking", "m_wide", [-1.0, 1.4, 0.8], _quat_from_to([0, 1, 0], [0.72, -0.03, -0.69]), [0.6, 0.6, 0.45]))


def _wh_mask(d):
    d["materials"].append({"name": "masked", "type": "mask", "material": "lambert", "alpha": "alpha"})
    _add_model(d, "m_masked", "cube", "masked")
    d["primitives"].append(_instance("masked", "m_masked", [0.0, 1.3, 0.5], CUBE_TURN, [0.6, 0.6, 0.6]))


POLE = _quat_from_to([0, 0, 1], np.asarray(CAMERA_AT) - np.asarray(BALL_AT))     # the ball's +z pole turned to the camera
CASES = {
    "lean": ("lean", None), "ext": ("ext", None), "deep": ("deep", None), "wh": ("wh", None),
    # transparent
    "glass_kt_black": ("lean", _mat("glass", Kt="black")),
    "glass_both_black": ("lean", _mat("glass", Kr="black", Kt="black")),
    "glass_grazing": ("lean", _grazing_pane),
    "deep_kr_black": ("deep", _mat("glass", Kr="black")), "deep_index_1": ("deep", _mat("glass", index=1.0)),
    "deep_index_1.0001": ("deep", _mat("glass", index=1.0001)),
    "deep_index_2.4": ("deep", _mat("glass", index=2.4)), "deep_index_0.8": ("deep", _mat("glass", index=0.8)),
    # Blinn
    "blinn_exponent_0": ("lean", _tex("exponent", float=0.0)), "blinn_exponent_1": ("lean", _tex("exponent", float=1.0)),
    "blinn_exponent_1e3": ("lean", _tex("exponent", float=1e3)), "blinn_exponent_1e5": ("lean", _tex("exponent", float=1e5)),
    "blinn_k_0": ("lean", _mat("blinn", k=0.0)), "blinn_k_0.5": ("lean", _mat("blinn", k=0.5)), "blinn_k_6": ("lean", _mat("blinn", k=6.0, index=0.8)),
    "blinn_k_negative": ("lean", _mat("blinn", k=-2.0)),
    "blinn_index_1": ("lean", _mat("blinn", index=1.0)),
    # mirror
    "deep_mirror_k_0.5": ("deep", _mat("mirror", k=0.5, index=1.5)), "deep_mirror_k_0": ("deep", _mat("mirror", k=0.0, index=1.5)),
    "deep_facing_mirrors": ("deep", _facing_mirrors),
    # Lambert
    "lambert_kd_0": ("lean", _mat("lambert", Kd="black")), "lambert_kd_1": ("lean", _mat("lambert", Kd="one")),
    # exactly-zero cosine
    "in_plane_lambert": ("lean", _lights("in_plane")),
    "in_plane_blinn": ("lean", _both(_lights("in_plane"), lambda d: _find(d, "primitives", "m_quad").update(material="blinn"))),
    # light distance
    "light_near_floor": ("lean", _lights("near_floor")), "light_on_vertex": ("lean", _light_on_vertex),
    "light_inside_epsilon": ("lean", _light_inside_epsilon),
    # spot
    "spot": ("lean", _lights("spot")), "spot_no_falloff": ("lean", _lights("spot_no_falloff")), "spot_falloff_0": ("lean", _lights("spot_falloff_0")),
    "spot_90": ("lean", _lights("spot_90")), "spot_in_glass": ("lean", _lights("spot_in_glass")),
    # area lights
    "quad": ("lean", _lights("quad")), "quad_behind": ("lean", _lights("quad_behind")), "quad_edge_on": ("lean", _lights("quad_edge_on")),
    "cube_emitter": ("lean", _lights("cube")),
    "sphere_emitter": ("lean", _lights("sphere")), "sphere_around": ("lean", _lights("sphere_around")),
    "disk_emitter": ("lean", _lights("disk")), "disk_edge_on": ("lean", _lights("disk_edge_on")),
    "emitter_front": ("lean", _lights("emitter_front")), "emitter_back": ("lean", _lights("emitter_back")),
    "two_emitters": ("lean", _lights("two_emitters")),
    # other lights
    "directional": ("lean", _lights("directional")),
    "ibl": ("lean", _lights("ibl")), "ibl_pole": ("lean", _lights("ibl_pole")),
    "lights_two": ("lean", _lights("two")), "lights_three": ("lean", _lights("three")), "lights_none": ("lean", _lights("none")),
    # shapes
    "sphere_pole": ("ext", _shape("ball", orientation=POLE)),
    "sphere_stretched": ("ext", _shape("ball", scale=[0.6, 0.3, 0.45], orientation=_quat([0.3, 1.0, 0.2], 40.0))),
    "sphere_large": ("ext", _shape("ball", scale=[0.7, 0.7, 0.7])),       # a longer silhouette
    "camera_in_sphere": ("ext", _camera_in_sphere),
    "disk_head_on": ("ext", _shape("plate", position=[0.0, 0.8, 0.5], orientation=_quat_from_to([0, 0, 1], np.asarray(CAMERA_AT) - np.asarray([0.0, 0.8, 0.5])))),
    "disk_edge_on_camera": ("ext", _shape("plate", position=[0.9, 1.3, 0.5], orientation=DISK_UP)),     # at the camera's height
    # masks
    "mask_lambert_0": ("deep", _masked("lambert", 0.0)), "mask_lambert_0.5": ("deep", _masked("lambert", 0.5)), "mask_lambert_1": ("deep", _masked("lambert", 1.0)),
    "mask_glass_0": ("deep", _masked("glass", 0.0)), "mask_glass_0.5": ("deep", _masked("glass", 0.5)), "mask_glass_1": ("deep", _masked("glass", 1.0)),
    "mask_stacked": ("deep", _stacked_masks), "mask_before_sky": ("deep", _mask_before_sky), "mask_behind_mirror": ("deep", _mask_behind_mirror),
    # cameras and integrators
    "orthographic": ("lean", _camera_kind("orthographic")), "thinlens": ("lean", _camera_kind("thinlens")),
    "wh_glass_2.4": ("wh", _mat("glass", index=2.4)), "wh_glass_0.8": ("wh", _mat("glass", index=0.8)),
    "wh_conductor": ("wh", _mat("blinn", k=0.5)), "wh_spot": ("wh", _lights("spot")),
    "wh_quad_1": ("wh", _lights("quad", sample_num=1)), "wh_quad_4": ("wh", _lights("quad", sample_num=4)),
    "wh_sphere_4": ("wh", _lights("sphere", sample_num=4)), "wh_ibl_3": ("wh", _lights("ibl_3")),
    "wh_mask": ("wh", _both(_wh_mask, _lights("quad", sample_num=4))), "wh_none": ("wh", _lights("none")),
    "ao": ("ext", _set_render(render_method="ao", ao_sample_num=4)),
}
SUMMED = {"sum_lean": "lean", "sum_ext": "ext", "sum_deep": "deep", "sum_wh": "wh"}
ALL_CASES = list(CASES) + list(SUMMED)
LEAN = [c for c, (base, _) in CASES.items() if base == "lean"]
TWINS = [c + "+ext" for c in LEAN]
BASES = ["lean", "ext", "deep", "wh"]


def is_lean(case):
    """Whether nothing in the case sets DevScene::extended (scene_prep.cpp: an analytic shape, also as an emitter; a directional or
    image based light; a mask, a subsurface material or a texture that is not constant; a camera that is no pinhole), so that the
    native sampler resolves to the lean kernels (api_render.hip's lean_native)."""
    d = doc(case)
    return (all(g["type"] == "mesh" for g in d["geometries"]) and all(x["type"] in ("point", "spot", "area") for x in d["lights"])
            and all(m["type"] != "mask" for m in d["materials"]) and d["camera"]["type"] == "perspective" and "lens_radius" not in d["camera"]
            and d["render_setting"]["render_method"] == "path_tracing")


def is_path(case):
    return doc(case)["render_setting"]["render_method"] == "path_tracing"


def doc(case):
    twin = case.endswith("+ext")
    case = case[:-4] if twin else case
    base, change = CASES[SUMMED.get(case, case)]
    d = _base(base)
    if change:
        change(d)
    if twin:
        assert base == "lean", case
        if not any(g["name"] == "ball" for g in d["geometries"]):
            d["geometries"].append({"name": "ball", "type": "sphere", "radius": 1.0})
        _add_model(d, "m_twin", "ball", "white")
        d["primitives"].append(_instance("twin", "m_twin", FAR_BELOW, scale=[0.1, 0.1, 0.1]))
    if case in SUMMED:
        d["render_setting"]["sample_per_pixel"] = 4
        d["camera"]["filter"] = {"type": "gaussian", "width": [2, 2], "falloff": 2.0}
    return d


@functools.lru_cache(maxsize=None)
def scene(case):
    return gs.load_scene_text(json.dumps(doc(case)), scene_dir())


def instance_id(case, name):
    """The instance index of the named primitive (instances are numbered in document order)."""
    return [p["name"] for p in doc(case)["primitives"] if p["type"] == "instance"].index(name)


def harness_doc(case, directory):
    """The document as the compiled reference loads it: absolute file paths, one thread."""
    d = doc(case)
    d["render_setting"]["thread_num"] = 1
    for section in ("geometries", "lights", "textures"):
        for g in d[section]:
            if "file" in g:
                g["file"] = os.path.join(directory, g["file"])
    return d


# ---------------------------------------------------------------------------
# Draws no generator gives: columns of real sample records overwritten.  Oracle.pt_offsets gives, per bounce, the columns of
# {light component, light geometry (2), BSDF component, BSDF direction (2), light pick}.
# ---------------------------------------------------------------------------
_F = np.float32
BELOW_ONE = np.nextafter(_F(1), _F(0))
# name -> (which columns of every bounce, value); "chance" and "masked" are per sample, taken from the probe
CRAFTED = {
    "bsdf_comp_below_chance": ("bsdf_comp", "chance-"), "bsdf_comp_at_chance": ("bsdf_comp", "chance"), "bsdf_comp_above_chance": ("bsdf_comp", "chance+"),
    "bsdf_comp_below_masked": ("bsdf_comp", "masked-"), "bsdf_comp_at_masked": ("bsdf_comp", "masked"), "bsdf_comp_above_masked": ("bsdf_comp", "masked+"),
    "pick_0": ("pick", _F(0)), "pick_below_1": ("pick", BELOW_ONE),
    "bsdf_dir_0": ("bsdf_dir", _F(0)), "bsdf_dir_below_1": ("bsdf_dir", BELOW_ONE),
    "light_geo_0": ("light_geo", _F(0)),
}
CRAFTED_CASES = {"lean": [n for n in CRAFTED if "masked" not in n and "bsdf_dir" not in n], "mask_lambert_0.5": [n for n in CRAFTED if "masked" in n],
                 "lights_two": ["pick_0", "pick_below_1"], "deep": ["bsdf_comp_below_chance", "bsdf_comp_at_chance", "bsdf_comp_above_chance", "bsdf_dir_0", "bsdf_dir_below_1", "bsdf_comp_at_masked"],
                 "two_emitters": ["light_geo_0", "bsdf_dir_0", "bsdf_dir_below_1"], "sphere_emitter": ["light_geo_0"], "disk_emitter": ["light_geo_0"],
                 "cube_emitter": ["light_geo_0"]}
COLUMNS = {"light_comp": (0, 1), "light_geo": (1, 2), "bsdf_comp": (2, 1), "bsdf_dir": (3, 2), "pick": (4, 1)}


def crafted(oracle, samples, name):
    """`samples` (n, dims) with one kind of column overwritten (CRAFTED): a constant at every bounce, a per-sample value at the
    first bounce only, the vertex it belongs to -- a later vertex has a threshold of its own, which may lie an ulp from this one.
    The per-sample values come from the probe's record of the unmodified samples: the first transparent vertex's reflectChance,
    the first masked vertex's maskedProb; they sit on the threshold of the samples whose first vertex is that material."""
    which, value = CRAFTED[name]
    out = np.array(samples, np.float32)
    rows = oracle.pt_offsets()
    if isinstance(value, str):
        rows = rows[:1]
        probe, _ = oracle.surface(samples)
        v = probe[:, oracle.SURF_REFLECT_CHANCE if value.startswith("chance") else oracle.SURF_MASKED_PROB].astype(np.float32)
        if value.endswith("-"):
            v = np.nextafter(v, _F(-1))
        elif value.endswith("+"):
            v = np.nextafter(v, _F(2))
        value = v[:, None]
    kind, width = COLUMNS[which]
    for row in rows:
        out[:, row[kind]:row[kind] + width] = value
    return out


GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def golden(case):
    """tests/golden/surface_<case>.npz (tests/golden/make_surface_golden.py): the compiled reference's film, samples (n, 4) and li,
    shared read-only."""
    with np.load(os.path.join(GOLDEN_DIR, "surface_" + case + ".npz")) as z:
        out = {k: z[k] for k in ("film", "samples", "li")}
    for a in out.values():
        a.setflags(write=False)
    return out
