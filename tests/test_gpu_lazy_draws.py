"""A vertex's sample dimensions drawn only where they are read (kernels/render_kernels.h LAZY_DRAWS; kernels/shade.h
light_sample_reads_u, mat_sample_reads_comp, mat_sample_reads_2d).

PathTracer::Li draws seven dimensions at every shaded vertex: the light pick, the light's component and 2D pair, the BSDF's
component and 2D pair.  The native sampler is counter-based, so the six lean kernels -- the quad megakernel with and without the
primary pass (GBL_PRIMARY=0), the one-ray-per-lane megakernel (GBL_MK_QUAD=0), each with and without exact_ties -- leave out the
draws nobody reads: the pick with a single light, the light's three unless the picked light is an area light, and of the
BSDF's three either the component (a transparent material) or the pair (every other one), never both -- the two kinds of lane
share one instruction stream (sampler.h native_1d_or_2d), whose values must be those of native_1d and native_2d bit for bit.
The instrumented megakernel render (stats=True) and the wavefront schedule go on drawing all seven
ahead of the vertex: the per-sample radiance of the six must be bit for bit theirs (torch.equal), and every sample must be
written exactly once (li[:, 3] == 1 over a buffer that starts at zero).

Scene: the closed box of test_gpu_last_ray.py (inside a second one, three times its size and tilted, that sends back the few rays
that slip through a corner), here with walls of all four lean materials so that the lanes of one wave part on the material:
  Lambert      the floor                      Blinn    the -x wall
  transparent  the ceiling                    mirror   the +x and -z walls
and the +z wall, the one the camera looks at, cut into four panes, one of each material, that meet where the camera's axis
meets the wall: the FIRST vertex of a frame's paths already falls on all four.
Light sets, each checked from the scene description for the kinds it is here for:
  point        one point light: the pick is skipped, and so are the light's draws
  point+spot   the pick is read (both lights are picked often), the light's draws are skipped
  area         one area light: the pick is skipped, the light's draws are made
  point+area   of comparable power: lanes of one wave disagree on the light's draws
Frames (the render window is the film's own pixels): 4 x 4 px x 1 spp, 16 paths; 16 x 16 px x 4 spp; 8 x 8 px x 9 spp -- not a
power of two, so the keyed permutation's cycle-walk loop runs, now inside a divergent branch; 8 x 8 px x 64 spp -- wave-owned
units of one tile row x 64 samples turning over.  Depths 1 (nothing is shaded), 2, 3 and 8.
"""
import json
import os

import numpy as np
import pytest

import meshes
import oracle_binding as ob
from goblin_amd import _abi
from goblin_amd import scene as gs

pytestmark = pytest.mark.gpu
SEED = 20261019
FRAMES = {"4x4x1": ((4, 4), 1), "16x16x4": ((16, 16), 4), "8x8x9": ((8, 8), 9), "8x8x64": ((8, 8), 64)}
DEPTHS = (1, 2, 3, 8)
HALF = 3.0                                           # the box is [-HALF, HALF]^3; the camera sits 1.4 from its centre
LEAN = {"quad+primary": {}, "quad": {"GBL_PRIMARY": "0"}, "one-ray": {"GBL_MK_QUAD": "0"}}   # x exact_ties: the six kernels

POINT = {"name": "bulb", "type": "point", "intensity": [2.5, 2.5, 2.5], "position": [-0.8, 2.0, -0.9]}
SPOT = {"name": "spot", "type": "spot", "intensity": [40.0, 38.0, 30.0], "position": [1.0, 2.0, -1.0], "target": [-1.9, -2.3, HALF],
        "theta_max": 25.0, "falloff_start": 15.0}   # aimed at the point of the +z wall where the four panes meet
PANEL = {"name": "panel", "type": "area", "geometry": "floor", "radiance": [10.0, 10.0, 10.0], "position": [0.3, 2.5, 0.2],
         "orientation": [0, 1, 0, 0], "scale": [0.5, 0.5, 0.5]}           # a 1 x 1 quad facing down: power pi * 10 ~ the bulb's 4 pi * 2.5
LIGHTS = {"point": [POINT], "point+spot": [POINT, SPOT], "area": [PANEL], "point+area": [POINT, PANEL]}
KINDS = {"point": [_abi.GBL_LIGHT_POINT], "point+spot": [_abi.GBL_LIGHT_POINT, _abi.GBL_LIGHT_SPOT], "area": [_abi.GBL_LIGHT_AREA],
         "point+area": [_abi.GBL_LIGHT_POINT, _abi.GBL_LIGHT_AREA]}
MATERIALS = {"white": _abi.GBL_MAT_LAMBERT, "brass": _abi.GBL_MAT_BLINN, "glass": _abi.GBL_MAT_TRANSPARENT, "mirror": _abi.GBL_MAT_MIRROR}


def _rects(rects):
    """Axis-aligned rectangles of the cube [-1, 1]^3's faces, each (inward normal, lo, hi) with lo / hi its extent along the two
    in-plane axes (u, v) = (cyclic shift of the normal, n x u); the geometric normal (v1 - v0) x (v2 - v0) is the inward one."""
    V, F = [], []
    for n, lo, hi in rects:
        n = np.array(n, np.float64)
        u = np.array([n[1], n[2], n[0]])
        v = np.cross(n, u)
        c = -n
        F += [[len(V), len(V) + 1, len(V) + 2], [len(V), len(V) + 2, len(V) + 3]]
        V += [c + lo[0] * u + lo[1] * v, c + hi[0] * u + lo[1] * v, c + hi[0] * u + hi[1] * v, c + lo[0] * u + hi[1] * v]
    return np.array(V, np.float32), np.array(F, np.int64)


FULL = ((-1.0, -1.0), (1.0, 1.0))
# the +z wall (inward normal -z: u = -y, v = -x) cut at the point the camera's axis meets it, (-1.93, -2.35, 3) / HALF
CUT_U, CUT_V = 2.35 / HALF, 1.93 / HALF
PANES = [((-1.0, -1.0), (CUT_U, CUT_V)), ((CUT_U, -1.0), (1.0, CUT_V)), ((CUT_U, CUT_V), (1.0, 1.0)), ((-1.0, CUT_V), (CUT_U, 1.0))]
WALLS = {   # one mesh per material
    "white": [([0, 1, 0],) + FULL, ([0, 0, -1],) + PANES[0]],
    "brass": [([1, 0, 0],) + FULL, ([0, 0, -1],) + PANES[1]],
    "glass": [([0, -1, 0],) + FULL, ([0, 0, -1],) + PANES[2]],
    "mirror": [([-1, 0, 0],) + FULL, ([0, 0, 1],) + FULL, ([0, 0, -1],) + PANES[3]],
}


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("lazy_draws")
    meshes.write_meshes(d, [])                       # floor.obj: the area light's quad
    for material, rects in WALLS.items():
        meshes.write_obj(os.path.join(str(d), "walls_%s.obj" % material), *_rects(rects))
    return str(d)


def _doc(name, resolution, spp):
    doc = meshes._base_doc([0, 0, 0], 0.35, 0.0, 1.0, None, resolution, spp, 8, None)
    doc["geometries"] = [{"name": "floor", "type": "mesh", "file": "floor.obj"}]
    doc["textures"] += [{"format": "color", "name": "silver", "type": "constant", "color": [0.9, 0.85, 0.8]},
                        {"format": "color", "name": "gold", "type": "constant", "color": [0.9, 0.7, 0.3]},
                        {"format": "float", "name": "shiny", "type": "constant", "float": 20.0}]
    doc["materials"] += [{"name": "mirror", "type": "mirror", "Kr": "silver"},
                         {"name": "brass", "type": "blinn", "Kg": "gold", "exponent": "shiny", "index": 1.5}]
    doc["primitives"] = []
    for material in WALLS:
        mesh = "walls_" + material
        doc["geometries"].append({"name": mesh, "type": "mesh", "file": mesh + ".obj"})
        doc["primitives"].append({"type": "model", "name": "m_" + mesh, "geometry": mesh, "material": material})
        doc["primitives"].append({"type": "instance", "name": "i_" + mesh, "model": "m_" + mesh, "position": [0.0, 0.0, 0.0],
                                  "orientation": [1, 0, 0, 0], "scale": [HALF] * 3})
        doc["primitives"].append({"type": "instance", "name": "o_" + mesh, "model": "m_" + mesh, "position": [0.0, 0.0, 0.0],
                                  "orientation": meshes.TILT, "scale": [3.0 * HALF] * 3})   # the outer shell
    doc["lights"] = LIGHTS[name]
    return doc


def _film_window(r, resolution):
    """The film's own pixels within the renderer's sample window (which adds the filter's margin all round)."""
    x0, x1, y0, y1 = r.window
    mx, my = (x1 - x0 - resolution[0]) // 2, (y1 - y0 - resolution[1]) // 2
    assert mx >= 0 and my >= 0
    return (x0 + mx, x0 + mx + resolution[0], y0 + my, y0 + my + resolution[1])


def _setting(r, depth):
    s = type(r.scene.desc.setting).from_buffer_copy(r.scene.desc.setting)
    s.max_ray_depth = depth
    return s


def _render(r, depth, window, exact=False, schedule="megakernel", stats=False, env=None):
    for k, v in (env or {}).items():
        os.environ[k] = v
    try:
        return r.render(setting=_setting(r, depth), seed=SEED, want_li=True, window=window, schedule=schedule, exact_ties=exact, stats=stats)
    finally:
        for k in (env or {}):
            os.environ.pop(k, None)


def _check_scene(name, r):
    """What the scene is in the list for, read from the scene description."""
    d = r.scene.desc
    assert sorted(d.lights[i].type for i in range(d.num_lights)) == sorted(KINDS[name])
    used = {d.materials[d.instances[i].material].type for i in range(d.num_instances) if d.instances[i].area_light < 0}
    assert used == set(MATERIALS.values()), used     # Lambert, Blinn, transparent and mirror walls, and nothing else
    assert r.info.instances == 2 * len(WALLS) + sum(1 for l in LIGHTS[name] if l["type"] == "area")
    if d.num_lights > 1:                             # both lights are picked, often: the pick's value matters
        power = ob.Oracle(r.scene).light_power()[:, 3]
        pick = power / power.sum()
        assert pick.shape == (2,) and 0.25 < float(pick.min()) and float(pick.max()) < 0.75, pick


@pytest.mark.parametrize("frame", list(FRAMES))
@pytest.mark.parametrize("name", list(LIGHTS))
def test_lean_kernels_equal_the_renderings_that_draw_every_dimension(torch, scene_dir, name, frame):
    from goblin_amd.renderer import HipPathTracer
    resolution, spp = FRAMES[frame]
    r = HipPathTracer(gs.load_scene_text(json.dumps(_doc(name, resolution, spp)), scene_dir), 0)
    _check_scene(name, r)
    window = _film_window(r, resolution)
    paths = resolution[0] * resolution[1] * spp
    for depth in DEPTHS:
        counted = _render(r, depth, window, stats=True)
        st = counted["stats"]
        assert st["paths"] == paths
        print("%s %s depth %d: extension rays %d, shadow rays %d, dimensions %d of %d paths" % (
            name, frame, depth, st["extension_rays"], st["shadow_rays"], st["dims"], paths))
        references = {"instrumented": counted["li"]}
        for exact in (False, True):
            references["wavefront, exact_ties %d" % exact] = _render(r, depth, window, exact, schedule="wavefront")["li"]
        for which, ref in references.items():
            assert bool((ref[:, 3] == 1).all()) and torch.isfinite(ref).all(), (name, frame, depth, which)
        for exact in (False, True):
            for kernel, env in LEAN.items():
                li = _render(r, depth, window, exact, env=env)["li"]
                tag = (name, frame, depth, kernel, exact)
                assert li.shape[0] == paths
                assert bool((li[:, 3] == 1).all()), tag           # every sample written, once
                assert torch.isfinite(li).all(), tag
                for which, ref in references.items():
                    assert torch.equal(li, ref), tag + (which,)
        # (depth 1 only sees emitters, and the camera sees none)
        assert depth == 1 or float(references["instrumented"][:, :3].sum()) > 0.0, "the frame is black: nothing is lit"
