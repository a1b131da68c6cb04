"""One fragment per bounce in the quad path kernels that start at the primary pass's record (kernels/render_kernels.h, the PRIM
vertex step): the lanes that continue a path and the lanes that start one are complementary, so the step decides first who ends
(without a fragment), refills the idle lanes, and then makes ONE fragment for every lane that holds a hit -- the continuing lanes,
the new ones, and the lanes whose hit instance is an area light: only those need the fragment's normal to close their bounce
(hit_Le), so they close it behind the regeneration ("deferred") and, when the path ends there, are refilled an iteration later.

Nothing a sample's radiance is made of changes, so the per-sample radiance of the three lean flavours x exact_ties must be bit for
bit (torch.equal) that of the renderings the reorder does not touch: the instrumented megakernel (stats=True), the wavefront
schedule with and without exact_ties, and -- for the two changed kernels -- the quad kernel without the pass (GBL_PRIMARY=0).
Every sample is written exactly once (li[:, 3] == 1 over a buffer that starts at zero) and is finite.  _render, the flavours and
the film window are tests/test_gpu_lazy_draws.py's.

The closed boxes of the last-ray, lazy-draws, primary, leaf-step and ties tests run the changed kernels under every light kind; the
scenes here are the cases the reorder itself can get wrong, each checked from its scene or its result to be what it is here for.
The camera sits at the origin and looks down +z (half angle atan 0.25); all quads are given in world coordinates:
  mirror     a mirror wall across the view; behind the camera two one-sided emitters side by side, one facing the wall ("lit", its
             reflection fills one half of the film) and one facing away ("dark", the other half).  At depth 2 and 3 the ray of
             the last shaded vertex on the wall hits an emitter: a deferred lane that ends at the cap, and its MIS term is the
             path's whole value -- the lit half is non-black, the dark half black (hit_Le from the back).
  floor      the same with a Lambert floor in view, depth 8: lanes of one wave split between hits with and without an area light,
             and the deferred ones continue.
  emitters   the two emitters in front of the camera, depth 1: the film is Le on the lit half and 0 on the dark one (the new
             lanes' 0 + Le).
  open       one Lambert quad floating in front of nothing, more than half of the camera rays leaving, 13 x 11 px (tiles clipped
             on both axes), 1 and 64 spp: rounds of regeneration that skip misses, units the pass found nothing in, a wave that
             never fills.
  tied       two coincident quads of different materials over one half of the view (their camera rays come back from the pass as
             GBL_PRIM_TIED and are traced by the path kernel: bounce -1) beside a single quad (record-started lanes: bounce 0).
             The pair is one mesh instanced twice under one transform, so both quads return bit-identical distances; that the
             camera rays over it meet both is read from the instrumented counters (RenderArgs::prim_inst is not visible from
             Python): they test at least one triangle more per such ray than in the same scene with the pair's second quad
             left out.  Which quad of a tie a lean kernel keeps depends on its own visiting order (the last triangle tested), so
             the lean kernels are compared with the quad kernel without the pass only, the exact_ties ones with every reference.
  point      a Lambert wall under a point light at depths 1 and 2: paths that are fetched, shaded and ended in one iteration;
             4 x 4 px x 1 spp (16 paths in a 64-lane wave) and 8 x 8 px x 64 spp (wave-owned units turning over).
"""
import json
import os

import numpy as np
import pytest

import meshes
import test_gpu_lazy_draws as lz
from goblin_amd import _abi
from goblin_amd import scene as gs

pytestmark = pytest.mark.gpu

LE = [10.0, 10.0, 10.0]
BULB = {"name": "bulb", "type": "point", "intensity": [30.0, 30.0, 30.0], "position": [0.5, 1.0, 0.0]}


def _quad(p0, u, v):
    """The quad p0, p0 + u, p0 + u + v, p0 + v as two triangles; its geometric normal is u x v."""
    p0, u, v = (np.asarray(a, np.float64) for a in (p0, u, v))
    V = np.array([p0, p0 + u, p0 + u + v, p0 + v], np.float32)
    return V, np.array([[0, 1, 2], [0, 2, 3]], np.int64)


QUADS = {
    "wall": _quad([-3, -3, 4], [0, 6, 0], [6, 0, 0]),            # z = 4 across the whole view, normal -z (towards the camera)
    "lit_behind": _quad([-6, -6, -3], [5.95, 0, 0], [0, 12, 0]),   # z = -3, x < 0, normal +z: faces the wall
    "dark_behind": _quad([0.05, -6, -3], [0, 12, 0], [5.95, 0, 0]),  # z = -3, x > 0, normal -z: the wall sees its back
    "ground": _quad([-3, -0.6, 1], [0, 0, 3], [6, 0, 0]),          # y = -0.6, normal +y: the lower part of the view
    "lit_front": _quad([-3, -3, 4], [0, 6, 0], [2.95, 0, 0]),      # z = 4, x < 0, normal -z: faces the camera
    "dark_front": _quad([0.05, -3, 4], [2.95, 0, 0], [0, 6, 0]),   # z = 4, x > 0, normal +z: the camera sees its back
    "island": _quad([-0.5, -0.45, 4], [0, 0.9, 0], [1.0, 0, 0]),   # 1.0 x 0.9 of the view's 2 x 2 at z = 4: 22 % of it
    "pair": _quad([-3, -3, 4], [0, 6, 0], [3, 0, 0]),              # z = 4, x < 0: instanced twice, two materials
    "single": _quad([0, -3, 5], [0, 6, 0], [3, 0, 0]),             # z = 5, x > 0
}


def _emitter(name):
    return {"name": name, "type": "area", "geometry": name, "radiance": LE, "position": [0.0, 0.0, 0.0], "orientation": [1, 0, 0, 0],
            "scale": [1.0, 1.0, 1.0]}


SCENES = {   # name: ([(quad, material)], lights)
    "mirror": ([("wall", "mirror")], [_emitter("lit_behind"), _emitter("dark_behind")]),
    "floor": ([("wall", "mirror"), ("ground", "white")], [_emitter("lit_behind"), _emitter("dark_behind")]),
    "emitters": ([], [_emitter("lit_front"), _emitter("dark_front")]),
    "open": ([("island", "white")], [BULB]),
    "tied": ([("pair", "white"), ("pair", "mirror"), ("single", "white")], [BULB]),
    "tied_once": ([("pair", "white"), ("single", "white")], [BULB]),   # (the counters' baseline for "tied")
    "point": ([("wall", "white")], [BULB]),
}


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("one_fragment")
    for name, (V, F) in QUADS.items():
        meshes.write_obj(os.path.join(str(d), name + ".obj"), V, F)
    return str(d)


def _doc(name, resolution, spp):
    surfaces, lights = SCENES[name]
    doc = meshes._base_doc([0, 0, 0], 1.0, 0.0, 1.0, None, resolution, spp, 8, None)
    doc["camera"]["position"] = [0.0, 0.0, 0.0]
    doc["camera"]["orientation"] = meshes._look([0.0, 0.0, 1.0])
    doc["textures"].append({"format": "color", "name": "silver", "type": "constant", "color": [0.9, 0.85, 0.8]})
    doc["materials"].append({"name": "mirror", "type": "mirror", "Kr": "silver"})
    used = sorted({q for q, _ in surfaces} | {l["geometry"] for l in lights if l["type"] == "area"})
    doc["geometries"] = [{"name": q, "type": "mesh", "file": q + ".obj"} for q in used]
    doc["primitives"] = []
    for i, (q, material) in enumerate(surfaces):
        doc["primitives"].append({"type": "model", "name": "m%d" % i, "geometry": q, "material": material})
        doc["primitives"].append({"type": "instance", "name": "i%d" % i, "model": "m%d" % i, "position": [0.0, 0.0, 0.0],
                                  "orientation": [1, 0, 0, 0], "scale": [1.0, 1.0, 1.0]})
    doc["lights"] = lights
    return doc


def _tracer(scene_dir, name, resolution, spp):
    from goblin_amd.renderer import HipPathTracer
    r = HipPathTracer(gs.load_scene_text(json.dumps(_doc(name, resolution, spp)), scene_dir), 0)
    d = r.scene.desc
    surfaces, lights = SCENES[name]
    kinds = {"area": _abi.GBL_LIGHT_AREA, "point": _abi.GBL_LIGHT_POINT}
    assert sorted(d.lights[i].type for i in range(d.num_lights)) == sorted(kinds[l["type"]] for l in lights)
    emitting = sum(1 for i in range(d.num_instances) if d.instances[i].area_light >= 0)
    assert emitting == sum(1 for l in lights if l["type"] == "area") and d.num_instances == len(surfaces) + emitting
    return r, lz._film_window(r, resolution)


def _references(torch, r, depth, window, tag, exact_only=None):
    """{name: li} of the renderings the reorder does not touch; each written once and finite."""
    refs = {"instrumented": lz._render(r, depth, window, stats=True)["li"]}
    for exact in (False, True):
        refs["wavefront, exact_ties %d" % exact] = lz._render(r, depth, window, exact, schedule="wavefront")["li"]
    for which, ref in refs.items():
        assert bool((ref[:, 3] == 1).all()) and torch.isfinite(ref).all(), tag + (which,)
    return refs


def _check(torch, li, paths, refs, tag):
    assert li.shape[0] == paths, tag
    assert bool((li[:, 3] == 1).all()), tag           # every sample written, once
    assert torch.isfinite(li).all(), tag
    for which, ref in refs.items():
        assert torch.equal(li, ref), tag + (which,)


def _all_flavours(torch, r, depth, window, paths, tag):
    """The three lean flavours x exact_ties against every reference; returns the headline kernel's radiance."""
    refs = _references(torch, r, depth, window, tag)
    headline = None
    for exact in (False, True):
        refs["quad kernel without the pass, exact_ties %d" % exact] = lz._render(r, depth, window, exact, env=lz.LEAN["quad"])["li"]
    for exact in (False, True):
        for kernel, env in lz.LEAN.items():
            li = lz._render(r, depth, window, exact, env=env)["li"]
            _check(torch, li, paths, refs, tag + (kernel, exact))
            if kernel == "quad+primary" and not exact:
                headline = li
    return headline


def _pixels(li, resolution, spp):
    """Per-pixel sum of the samples' radiance, [rows, columns]."""
    return li[:, :3].reshape(resolution[1], resolution[0], spp, 3).sum(dim=(2, 3)).cpu().numpy()


def _halves(img):
    """The film's two halves without the two middle columns (the gap between the emitters falls there)."""
    w = img.shape[1]
    return img[:, :w // 2 - 1], img[:, w // 2 + 1:]


def _one_half_lit_one_black(img, tag):
    a, b = _halves(img)
    lit, dark = (a, b) if a.sum() > b.sum() else (b, a)
    assert (lit > 0.0).all(), tag          # every pixel whose ray ends on the emitter's front
    assert (dark == 0.0).all(), tag        # hit_Le from the back
    return lit


@pytest.mark.parametrize("depth", [2, 3])
def test_deferred_lanes_that_end_at_the_cap_carry_the_mis_term(torch, scene_dir, depth):
    resolution, spp = (16, 16), 16
    r, window = _tracer(scene_dir, "mirror", resolution, spp)
    li = _all_flavours(torch, r, depth, window, resolution[0] * resolution[1] * spp, ("mirror", depth))
    img = _pixels(li, resolution, spp)
    print("mirror, depth %d: film sum %.6g" % (depth, img.sum()))
    _one_half_lit_one_black(img, ("mirror", depth))


def test_deferred_lanes_that_continue_beside_lanes_without_an_area_light(torch, scene_dir):
    resolution, spp = (16, 16), 16
    r, window = _tracer(scene_dir, "floor", resolution, spp)
    d = r.scene.desc
    surface = {d.materials[d.instances[i].material].type for i in range(d.num_instances) if d.instances[i].area_light < 0}
    assert surface == {_abi.GBL_MAT_LAMBERT, _abi.GBL_MAT_MIRROR}, surface
    paths = resolution[0] * resolution[1] * spp
    rays = {depth: lz._render(r, depth, window, stats=True)["stats"]["extension_rays"] for depth in (3, 8)}
    print("floor: extension rays at depth 3 / 8: %d / %d of %d paths" % (rays[3], rays[8], paths))
    assert rays[8] > rays[3] > paths          # paths go on past the vertex whose ray found the emitter
    li = _all_flavours(torch, r, 8, window, paths, ("floor", 8))
    img = _pixels(li, resolution, spp)
    assert (img > 0.0).any()


def test_an_emitter_seen_directly_is_le_in_front_and_black_behind(torch, scene_dir):
    resolution, spp = (16, 16), 4
    r, window = _tracer(scene_dir, "emitters", resolution, spp)
    li = _all_flavours(torch, r, 1, window, resolution[0] * resolution[1] * spp, ("emitters", 1))
    lit = _one_half_lit_one_black(_pixels(li, resolution, spp), ("emitters", 1))
    assert (lit == np.float32(3 * spp * LE[0])).all()       # 0 + Le, every sample


@pytest.mark.parametrize("spp", [1, 64])
def test_misses_and_units_the_pass_found_nothing_in(torch, scene_dir, spp):
    resolution = (13, 11)
    r, window = _tracer(scene_dir, "open", resolution, spp)
    for depth in (2, 8):
        li = _all_flavours(torch, r, depth, window, resolution[0] * resolution[1] * spp, ("open", spp, depth))
        left = float((li[:, :3].sum(dim=1) == 0.0).float().mean())
        print("open, %d spp, depth %d: %.1f %% of the samples are black" % (spp, depth, 100.0 * left))
        assert 0.5 < left < 1.0, left          # more than half of the camera rays leave, the others are lit


def test_tied_camera_rays_beside_record_started_ones(torch, scene_dir):
    resolution, spp = (16, 16), 16
    r, window = _tracer(scene_dir, "tied", resolution, spp)
    paths = resolution[0] * resolution[1] * spp
    once, window_once = _tracer(scene_dir, "tied_once", resolution, spp)
    assert window_once == window
    tests = {name: lz._render(t, 1, window, stats=True)["stats"]["tris"] for name, t in (("tied", r), ("tied_once", once))}
    over_pair = paths * (resolution[0] // 2 - 1) // resolution[0]       # the camera rays of the columns that lie on the pair entirely
    print("tied: triangle tests of the camera rays %d, without the second quad %d; at least %d rays cross the pair" % (
        tests["tied"], tests["tied_once"], over_pair))
    assert tests["tied"] - tests["tied_once"] >= over_pair
    for depth in (2, 4):
        tag = ("tied", depth)
        refs = _references(torch, r, depth, window, tag)
        without = {exact: lz._render(r, depth, window, exact, env=lz.LEAN["quad"])["li"] for exact in (False, True)}
        exact_refs = {"instrumented": refs["instrumented"], "wavefront, exact_ties 1": refs["wavefront, exact_ties 1"],
                      "quad kernel without the pass": without[True]}
        for kernel, env in lz.LEAN.items():
            _check(torch, lz._render(r, depth, window, True, env=env)["li"], paths, exact_refs, tag + (kernel, True))
        lean = lz._render(r, depth, window, False)["li"]
        _check(torch, lean, paths, {"quad kernel without the pass": without[False]}, tag + ("quad+primary", False))


@pytest.mark.parametrize("frame", ["4x4x1", "8x8x64"])
def test_paths_fetched_shaded_and_ended_in_one_iteration(torch, scene_dir, frame):
    resolution, spp = lz.FRAMES[frame]
    r, window = _tracer(scene_dir, "point", resolution, spp)
    paths = resolution[0] * resolution[1] * spp
    for depth in (1, 2):
        st = lz._render(r, depth, window, stats=True)["stats"]
        assert st["paths"] == paths and st["shadow_rays"] <= paths      # one shaded vertex per path at most
        li = _all_flavours(torch, r, depth, window, paths, ("point", frame, depth))
        lit = float(li[:, :3].sum())
        assert (lit == 0.0) if depth == 1 else (lit > 0.0), (frame, depth, lit)
