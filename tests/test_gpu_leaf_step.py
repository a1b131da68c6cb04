"""The leaf / instance step of the traversal loops (kernels/trace.h trav_other_kind, kernels/quadtrace.h quad_transition) on the
smallest scenes that reach each way out of an instance.

The lean quad kernels' one-ray-per-lane loops take that step in its FUSE form: a leaf first, then ONE site that leaves an instance
-- for a sentinel met at the top of the step as for one the leaf's pop uncovers -- with the exit marker tested behind it, then the
instance entry.  The order of a ray's node visits and triangle tests is what it was, so the per-sample radiance of the lean quad
megakernel must be bit for bit that of the renderings that do not run this form: the one-ray-per-lane megakernel (GBL_MK_QUAD=0)
and the wavefront schedule, with and without exact_ties, under the path tracer and AO.  (The wavefront schedule covers the path
tracer only -- gbl_render turns it away for AO -- so AO has the first reference alone.)

Scenes (tests/meshes.py, written to a temporary directory, nothing committed), each checked for the property it is here for:
  one-triangle   few1 over the floor quad: every BLAS root is a leaf (gbl_info: 0 BLAS nodes), so the leaf's pop uncovers the
                 sentinel and then, for a ray that met nothing else, the exit marker
  all-missed     few9: scattered triangles under BLAS nodes, so a ray inside a node's box misses all four children and the
                 INTERIOR step pops the sentinel, which the next leaf / instance step meets at its top
  two-instances  few5 twice, the second shifted by a fraction of its size: a sentinel is followed by another TLAS leaf
  300-instances  meshes.instances_doc(300): world boxes overlapping at every scale
Frames (the render window is the film's own pixels, without the filter's margin): 4 x 4 px x 1 spp -- 16 paths, never more than
GBL_QUAD_MAX rays in a wave, so every query is a quad phase from its first step -- and 16 x 16 px x 4 spp, 1024 paths: the
one-ray-per-lane phase and the migration.  Every sample must be written exactly once (li[:, 3] == 1 over a buffer that starts at
zero).
"""
import json
import os

import pytest

import meshes
from goblin_amd import scene as gs

pytestmark = pytest.mark.gpu
SEED = 90210
FRAMES = {"16-paths": ((4, 4), 1), "1024-paths": ((16, 16), 4)}
SCENES = ("one-triangle", "all-missed", "two-instances", "300-instances")
AO_RAYS = 5


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("leaf_step")
    meshes.write_meshes(d, ["few1", "few5", "few9"])
    return str(d)


def _doc(name, method, resolution, spp):
    ao = AO_RAYS if method == "ao" else None
    if name == "one-triangle":
        return meshes.scene_doc("few1", method=method, resolution=resolution, spp=spp, depth=5, ao_samples=ao)
    if name == "all-missed":
        return meshes.scene_doc("few9", method=method, resolution=resolution, spp=spp, depth=5, ao_samples=ao)
    if name == "two-instances":
        doc = meshes.scene_doc("few5", method=method, resolution=resolution, spp=spp, depth=5, ao_samples=ao)
        doc["primitives"].append({"type": "instance", "name": "i_few5_again", "model": "m_few5", "position": [0.1, 0.05, -0.05],
                                  "orientation": meshes.TILT, "scale": [1.0] * 3})
        return doc
    doc = meshes.instances_doc(300, resolution=resolution, spp=spp, depth=5)
    if method == "ao":
        doc["render_setting"]["render_method"] = "ao"
        doc["render_setting"]["ao_sample_num"] = AO_RAYS
    return doc


def _film_window(r, resolution):
    """The film's own pixels within the renderer's sample window (which adds the filter's margin all round)."""
    x0, x1, y0, y1 = r.window
    mx, my = (x1 - x0 - resolution[0]) // 2, (y1 - y0 - resolution[1]) // 2
    assert mx >= 0 and my >= 0
    return (x0 + mx, x0 + mx + resolution[0], y0 + my, y0 + my + resolution[1])


def _render(r, exact, window, schedule="megakernel", env=None):
    for k, v in (env or {}).items():
        os.environ[k] = v
    try:
        return r.render(seed=SEED, want_li=True, window=window, schedule=schedule, exact_ties=exact)["li"]
    finally:
        for k in (env or {}):
            os.environ.pop(k, None)


def _check_scene(name, info):
    """The property the scene is in the list for, read from what the library built."""
    if name == "one-triangle":
        assert info.blas_nodes == 0 and info.instances == 2, (info.blas_nodes, info.instances)   # leaf roots: floor, few1
    elif name == "all-missed":
        assert info.blas_nodes >= 1 and info.triangles == 2 + 9, (info.blas_nodes, info.triangles)
    elif name == "two-instances":
        assert info.instances == 3 and info.instanced_triangles == 2 + 5 + 5, (info.instances, info.instanced_triangles)
    else:
        assert info.instances == 301, info.instances


@pytest.mark.parametrize("method", ["path_tracing", "ao"])
@pytest.mark.parametrize("frame", list(FRAMES))
@pytest.mark.parametrize("name", SCENES)
def test_leaf_step_radiance_is_bit_identical(torch, scene_dir, name, frame, method):
    from goblin_amd.renderer import HipPathTracer
    resolution, spp = FRAMES[frame]
    r = HipPathTracer(gs.load_scene_text(json.dumps(_doc(name, method, resolution, spp)), scene_dir), 0)
    _check_scene(name, r.info)
    window = _film_window(r, resolution)
    lit = False
    for exact in (False, True):
        li = _render(r, exact, window)
        assert li.shape[0] == resolution[0] * resolution[1] * spp
        assert bool((li[:, 3] == 1).all()), (name, frame, method, exact)     # every sample written, once
        assert torch.isfinite(li).all()
        one_ray = _render(r, exact, window, env={"GBL_MK_QUAD": "0"})
        assert torch.equal(li, one_ray), (name, frame, method, exact, "one ray per lane")
        if method == "path_tracing":
            wavefront = _render(r, exact, window, schedule="wavefront")
            assert torch.equal(li, wavefront), (name, frame, method, exact, "wavefront")
        lit = lit or float(li[:, :3].sum()) > 0.0
    assert lit, "the frame is black: nothing was hit or nothing is lit"
