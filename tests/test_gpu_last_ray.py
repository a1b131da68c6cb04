"""The capped vertex's extension ray (kernels/render_kernels.h, "the last vertex under a delta light").

PathTracer::Li shades the vertices at bounce 0 .. max_ray_depth - 2 and traces an extension ray from each; the hit of the LAST of
them is only looked at by the MIS test `instances[hit].area_light == picked light`, which nothing passes when the light picked at
that vertex is a point, spot or directional light.  The six lean kernels of the native sampler -- the quad megakernel with and
without the primary pass (GBL_PRIMARY=0), the one-ray-per-lane megakernel (GBL_MK_QUAD=0), each with and without exact_ties -- end
such a lane at the vertex instead, with the term the close step would have added one iteration later.  The wavefront schedule and
the instrumented megakernel render (stats=True) go on tracing the ray: the per-sample radiance of the six must be bit for bit
theirs, and every sample must be written exactly once (li[:, 3] == 1 over a buffer that starts at zero).

Scenes (tests/meshes.py plus an inward-facing box of two meshes, written to a temporary directory), each checked for the property
it is here for.  The box has three Lambert and three mirror walls around the camera and the lights: every ray hits and no BSDF
sample is black, so every path reaches the cap, which the instrumented render shows as extension_rays == paths * max_ray_depth.
(A ray that leaves a wall within its own epsilon, 1e-3 t, of a corner starts behind the neighbouring wall and is outside: two in a
thousand do.  So the box stands inside a second one, three times its size and tilted off every axis, whose walls send them back.)
  box              a point and a spot light: every capped lane takes the new exit
  box-point        the point light alone
  box-spot         the spot light alone; its cone misses part of the walls, so L is black at some capped vertices and Ld is zero
  box-directional  a directional light (it makes the scene an EXT one -- its power depends on the scene bound -- so the lean
                   kernels do not run and the rule is compiled out; and inside a closed box every shadow ray towards it is
                   occluded, so the frame is black: it is here so that both stay true)
  open             few5 over the floor: most paths leave the scene before the cap
  box-area         an area light alone: the rule never fires
  box-mixed        a point and an area light of comparable power: lanes of one wave pick different lights, and the one that
                   picked the area light still needs its ray (both pick probabilities are checked from the lights' powers,
                   which is what light_pick_pdf is made of: power[i] / sum)
Frames (the render window is the film's own pixels): 4 x 4 px x 1 spp -- 16 paths, every query a quad phase from its first step --
and 16 x 16 px x 4 spp, 1024 paths: the dense phase, the migration, units turning over in wave_take.
Depths 1 (nothing is shaded), 2 (the first vertex is the capped one: with the primary pass a path is fetched, shaded and ended in
one iteration), 3 and 8.
"""
import json
import math
import os

import numpy as np
import pytest

import meshes
import oracle_binding as ob
from goblin_amd import scene as gs

pytestmark = pytest.mark.gpu
SEED = 20261003
FRAMES = {"16-paths": ((4, 4), 1), "1024-paths": ((16, 16), 4)}
SCENES = ("box", "box-point", "box-spot", "box-directional", "open", "box-area", "box-mixed")
DEPTHS = (1, 2, 3, 8)
HALF = 3.0                                           # the box is [-HALF, HALF]^3; the camera sits 1.4 from its centre
LEAN = {"quad+primary": {}, "quad": {"GBL_PRIMARY": "0"}, "one-ray": {"GBL_MK_QUAD": "0"}}   # x exact_ties: the six kernels

POINT = {"name": "bulb", "type": "point", "intensity": [2.5, 2.5, 2.5], "position": [-0.8, 2.0, -0.9]}
SPOT = {"name": "spot", "type": "spot", "intensity": [40.0, 38.0, 30.0], "position": [1.0, 2.0, -1.0], "target": [-1.9, -2.3, HALF],
        "theta_max": 25.0, "falloff_start": 15.0}   # aimed at the Lambert wall the camera looks at
SUN = {"name": "sun", "type": "directional", "radiance": [3.0, 3.0, 2.5], "direction": [0.3, -1.0, 0.2]}
PANEL = {"name": "panel", "type": "area", "geometry": "floor", "radiance": [10.0, 10.0, 10.0], "position": [0.3, 2.5, 0.2],
         "orientation": [0, 1, 0, 0], "scale": [0.5, 0.5, 0.5]}           # a 1 x 1 quad facing down: power pi * 10 ~ the bulb's 4 pi * 2.5
LIGHTS = {"box": [POINT, SPOT], "box-point": [POINT], "box-spot": [SPOT], "box-directional": [SUN], "box-area": [PANEL],
          "box-mixed": [POINT, PANEL]}


def _walls(normals):
    """Unit quads at distance 1 from the origin whose geometric normal (v1 - v0) x (v2 - v0) is the given INWARD one."""
    V, F = [], []
    for n in normals:
        n = np.array(n, np.float64)
        u = np.array([n[1], n[2], n[0]])             # a cyclic shift of an axis vector: u x v == n
        v = np.cross(n, u)
        c = -n
        F += [[len(V), len(V) + 1, len(V) + 2], [len(V), len(V) + 2, len(V) + 3]]
        V += [c - u - v, c + u - v, c + u + v, c - u + v]
    return np.array(V, np.float32), np.array(F, np.int64)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("last_ray")
    meshes.write_meshes(d, ["few5"])
    meshes.write_obj(os.path.join(str(d), "walls_a.obj"), *_walls([[0, 1, 0], [-1, 0, 0], [0, 0, 1]]))    # floor, +x and -z walls
    meshes.write_obj(os.path.join(str(d), "walls_b.obj"), *_walls([[0, -1, 0], [1, 0, 0], [0, 0, -1]]))   # ceiling, -x and +z walls
    return str(d)


def _doc(name, resolution, spp):
    if name == "open":
        return meshes.scene_doc("few5", resolution=resolution, spp=spp, depth=8)
    doc = meshes._base_doc([0, 0, 0], 0.35, 0.0, 1.0, None, resolution, spp, 8, None)
    doc["geometries"] = [{"name": "floor", "type": "mesh", "file": "floor.obj"}, {"name": "walls_a", "type": "mesh", "file": "walls_a.obj"},
                         {"name": "walls_b", "type": "mesh", "file": "walls_b.obj"}]
    doc["textures"].append({"format": "color", "name": "silver", "type": "constant", "color": [0.9, 0.85, 0.8]})
    doc["materials"].append({"name": "mirror", "type": "mirror", "Kr": "silver"})
    doc["primitives"] = []
    for mesh, material in (("walls_a", "mirror"), ("walls_b", "white")):   # the camera looks at the +z wall: Lambert
        doc["primitives"].append({"type": "model", "name": "m_" + mesh, "geometry": mesh, "material": material})
        doc["primitives"].append({"type": "instance", "name": "i_" + mesh, "model": "m_" + mesh, "position": [0.0, 0.0, 0.0],
                                  "orientation": [1, 0, 0, 0], "scale": [HALF] * 3})
        doc["primitives"].append({"type": "instance", "name": "o_" + mesh, "model": "m_" + mesh, "position": [0.0, 0.0, 0.0],
                                  "orientation": meshes.TILT, "scale": [3.0 * HALF] * 3})   # the outer shell (see the module's text)
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
    """The property the scene is in the list for, read from the scene itself."""
    d = r.scene.desc
    kinds = sorted(d.lights[i].type for i in range(d.num_lights))
    if name == "box-spot":
        # the cone holds the point it is aimed at and leaves at least one corner of the box out
        pos, tgt = np.array(SPOT["position"]), np.array(SPOT["target"])
        axis = (tgt - pos) / np.linalg.norm(tgt - pos)
        cos_max = math.cos(math.radians(SPOT["theta_max"]))
        corners = [np.array([x, y, z]) for x in (-HALF, HALF) for y in (-HALF, HALF) for z in (-HALF, HALF)]
        assert min(float(np.dot((c - pos) / np.linalg.norm(c - pos), axis)) for c in corners) < cos_max < 1.0
    if name == "box-mixed":
        from goblin_amd import _abi
        assert kinds == sorted([_abi.GBL_LIGHT_POINT, _abi.GBL_LIGHT_AREA])
        power = ob.Oracle(r.scene).light_power()[:, 3]
        pick = power / power.sum()
        assert pick.shape == (2,) and 0.25 < float(pick.min()) and float(pick.max()) < 0.75, pick   # both are picked, often
    if name == "box-area":
        assert d.num_lights == 1
    if name.startswith("box"):
        assert r.info.instances == 4 + sum(1 for l in LIGHTS[name] if l["type"] == "area")


@pytest.mark.parametrize("frame", list(FRAMES))
@pytest.mark.parametrize("name", SCENES)
def test_lean_kernels_equal_the_renderings_that_trace_the_last_ray(torch, scene_dir, name, frame):
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
        print("%s %s depth %d: extension rays %d, shadow rays %d of %d paths" % (name, frame, depth, st["extension_rays"], st["shadow_rays"], paths))
        if name in ("box", "box-point", "box-spot"):
            assert st["extension_rays"] == paths * depth, (name, frame, depth)   # every path reaches the cap
        if name == "open" and depth == 8:
            assert st["extension_rays"] < paths * depth // 2, (name, frame, depth)   # most do not: under half the rays of capped paths
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
        # (depth 1 only sees emitters; a directional light never reaches the inside of a closed box: that frame is black and stays so)
        lit = float(references["instrumented"][:, :3].sum()) > 0.0
        assert lit or depth == 1 or name == "box-directional", "the frame is black: nothing is lit"
