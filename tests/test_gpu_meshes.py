"""Both BVH builders on meshes that are hard to build over (tests/meshes.py): per-sample radiance against the oracle -- which
tests/test_meshes_cpu.py pins to the compiled reference, bit for bit, on these very scenes -- and the device-built tree's
node count and depth against a serial restatement of kernels/lbvh.h.

Frames are 48x48 at 4 spp, depth 5.  Bars: radiance bit-identical (flips == 0, relL2 == 0) for either builder under either
schedule, with and without `exact_ties`; gbl_info's blas_nodes / blas_depth EQUAL to the restatement's.

Measured on an MI355X (device / host builder): the deep spiral builds 23 / 25 four-wide levels (297 / 828 nodes) under a
TLAS of depth 2, 73 / 74 traversal stack entries (scene_stack_entries).  Either tree takes the scene past 64: no primary
pass, more than 64 KB of LDS stacks per megakernel workgroup.  Every test passed on its first run; no
kernel changed.
"""
import json

import numpy as np
import pytest

import helpers
import meshes
import oracle_binding as ob
from goblin_amd import scene as gs

pytestmark = pytest.mark.gpu
SEED = 31337
BUILDERS = ("host", "device")
_scenes = {}


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("meshes")
    meshes.write_meshes(d, meshes.ALL)
    return str(d)


class Case:
    """A loaded scene with its oracle and, computed once, the oracle's radiance of the native sampler's records."""

    def __init__(self, doc, scene_dir):
        self.doc = doc
        self.scene = gs.load_scene_text(json.dumps(doc), scene_dir)
        self.oracle = ob.Oracle(self.scene)
        self._ref = None

    def samples(self):
        return self.oracle.native_samples(SEED)

    def li_ref(self):
        if self._ref is None:
            self._ref, _ = self.oracle.li_replay(self.samples(), threads=4)
            assert np.isfinite(self._ref).all() and self._ref[:, :3].max() > 0
            self._ref.setflags(write=False)
        return self._ref


def case(scene_dir, names, method=None, ao_samples=None):
    key = (tuple(names) if not isinstance(names, str) else names, method)
    if key not in _scenes:
        _scenes[key] = Case(meshes.scene_doc(names, method=method, ao_samples=ao_samples), scene_dir)
    return _scenes[key]


def assert_equals_oracle(li, li_ref, what):
    assert np.isfinite(li).all(), what
    flips = helpers.li_mismatch_fraction(li, li_ref)
    rel = helpers.rel_l2(li[:, :3], li_ref[:, :3])
    print(*what, "flips %.5f relL2 %.2e" % (flips, rel))
    assert flips == 0.0 and rel == 0.0, (what, flips, rel)


def restated(scene):
    shapes = [meshes.lbvh_shape(P, I) for P, I in meshes.scene_meshes(scene)]
    return sum(s["nodes"] for s in shapes), max(s["depth"] for s in shapes), sum(len(s["order"]) for s in shapes)


# ---------------------------------------------------------------------------
# radiance
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", meshes.ALL)
def test_mesh_radiance_equals_oracle_for_both_builders(torch, scene_dir, name):
    """Every mesh x builder x schedule x exact_ties: the radiance of every sample equals the oracle's, and the host-built
    and device-built trees give the same tensor."""
    from goblin_amd.renderer import HipPathTracer
    c = case(scene_dir, name)
    li_ref = c.li_ref()
    tracers = {bvh: HipPathTracer(c.scene, 0, bvh=bvh) for bvh in BUILDERS}
    for schedule in ("megakernel", "wavefront"):
        for exact in (False, True):
            li = {bvh: tracers[bvh].render(seed=SEED, want_li=True, schedule=schedule, exact_ties=exact)["li"] for bvh in BUILDERS}
            for bvh in BUILDERS:
                assert_equals_oracle(li[bvh].cpu().numpy(), li_ref, (name, bvh, schedule, "exact_ties" if exact else "lean"))
            assert torch.equal(li["host"], li["device"]), (name, schedule, exact)


@pytest.mark.parametrize("method", ["ao", "whitted"])
def test_all_meshes_under_ao_and_whitted(torch, scene_dir, method):
    """All meshes in one scene under the AO renderer with 9 rays (any-hit traversal) and the Whitted renderer, both builders."""
    from goblin_amd.renderer import HipPathTracer
    c = case(scene_dir, meshes.ALL, method=method, ao_samples=9 if method == "ao" else None)
    li_ref = c.li_ref()
    li = {}
    for bvh in BUILDERS:
        li[bvh] = HipPathTracer(c.scene, 0, bvh=bvh).render(seed=SEED, want_li=True)["li"]
        assert_equals_oracle(li[bvh].cpu().numpy(), li_ref, (method, bvh))
    assert torch.equal(li["host"], li["device"])


def test_all_meshes_under_the_path_tracer(torch, scene_dir):
    from goblin_amd.renderer import HipPathTracer
    c = case(scene_dir, meshes.ALL)
    li_ref = c.li_ref()
    for bvh in BUILDERS:
        r = HipPathTracer(c.scene, 0, bvh=bvh)
        for schedule in ("megakernel", "wavefront"):
            assert_equals_oracle(r.render(seed=SEED, want_li=True, schedule=schedule)["li"].cpu().numpy(), li_ref, ("all", bvh, schedule))


@pytest.mark.parametrize("name", [meshes.DEEP, "urchin"])
def test_stream_sampler_film_equals_the_reference_render(torch, scene_dir, name):
    """The reference's own sample stream generated on the device against the oracle's whole render (the bars of
    tests/test_gpu_fuzz.py: weights rtol 1e-5, normalised film relL2 <= 3e-5)."""
    from goblin_amd.renderer import HipPathTracer
    c = case(scene_dir, name)
    ref = c.oracle.render(threads=1)["film"]
    for bvh in BUILDERS:
        film = HipPathTracer(c.scene, 0, bvh=bvh).render(sampler="stream")["film"].numpy()
        rel = helpers.rel_l2(ob.normalize_film(film), ob.normalize_film(ref))
        print(name, bvh, "stream film relL2 %.2e" % rel)
        np.testing.assert_allclose(film[..., 3], ref[..., 3], rtol=1e-5, atol=1e-6)
        assert rel <= 3e-5, (name, bvh, rel)


@pytest.mark.parametrize("name", [meshes.DEEP, "urchin"])
def test_replayed_records_equal_oracle_with_counters(torch, scene_dir, name):
    """Replay mode with per-sample radiance and counters: the instrumented (EXT) kernel builds, both schedules and builders."""
    from goblin_amd.renderer import HipPathTracer
    c = case(scene_dir, name)
    samples, li_ref = c.samples(), c.li_ref()
    for bvh in BUILDERS:
        r = HipPathTracer(c.scene, 0, bvh=bvh)
        for schedule in ("megakernel", "wavefront"):
            out = r.render(replay_samples=samples, want_li=True, stats=True, schedule=schedule)
            assert_equals_oracle(out["li"].cpu().numpy(), li_ref, (name, bvh, schedule, "replay"))
            assert out["stats"]["paths"] == c.scene.num_paths()


# ---------------------------------------------------------------------------
# the device tree
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", meshes.ALL + ["all"])
def test_device_tree_shape_equals_the_restatement(torch, scene_dir, name):
    from goblin_amd.renderer import HipPathTracer
    c = case(scene_dir, meshes.ALL if name == "all" else name)
    nodes, depth, tris = restated(c.scene)
    dev, host = HipPathTracer(c.scene, 0, bvh="device").info, HipPathTracer(c.scene, 0, bvh="host").info
    print(name, "device nodes", dev.blas_nodes, "depth", dev.blas_depth, "restated", nodes, depth, "host nodes", host.blas_nodes, "depth", host.blas_depth)
    assert dev.blas_nodes == nodes
    assert dev.blas_depth == depth
    assert dev.triangles == host.triangles == tris


BUNNY_VN = {"geometries": [{"name": "bunny", "type": "mesh", "file": "models/bunny_vn.obj"},
                           {"name": "plane", "type": "mesh", "file": "models/plane.obj"},
                           {"name": "sphere", "type": "sphere", "radius": 0.05}]}


@pytest.mark.parametrize("scene_name,extra", [("bunny", {}), ("cornell", {}), ("bunny", BUNNY_VN)], ids=["bunny", "cube", "bunny_vn"])
def test_device_tree_shape_of_the_bundled_meshes(torch, scene_name, extra):
    """bunny.obj, cube.obj (in the Cornell box, with the bunny) and bunny_vn.obj."""
    from goblin_amd.renderer import HipPathTracer
    ov = gs.config_overrides(resolution=(16, 16), spp=1, depth=2)
    ov.update(extra)
    scene = gs.load_scene(scene_name, ov)
    nodes, depth, tris = restated(scene)
    dev, host = HipPathTracer(scene, 0, bvh="device").info, HipPathTracer(scene, 0, bvh="host").info
    print(scene_name, "device nodes", dev.blas_nodes, "depth", dev.blas_depth, "restated", nodes, depth)
    assert dev.blas_nodes == nodes
    assert dev.blas_depth == depth
    assert dev.triangles == host.triangles == tris


def test_deep_tree_renders_past_the_64_entry_stack(torch, scene_dir, monkeypatch):
    """The deep spiral's device-built tree needs more than 64 traversal stack entries: no primary pass (api_render.hip), per-lane
    stacks beyond GBL_PACKET_STACK, more than 64 KB of LDS per megakernel workgroup and the wavefront stacks' spill -- and still
    inside the 160 KB refusal.  Radiance equals the oracle under both schedules and with the wavefront's launches serialised."""
    from goblin_amd.renderer import HipPathTracer
    c = case(scene_dir, meshes.DEEP)
    li_ref = c.li_ref()
    r = HipPathTracer(c.scene, 0, bvh="device")
    host = HipPathTracer(c.scene, 0, bvh="host").info
    print("deep spiral: device blas_depth", r.info.blas_depth, "tlas_depth", r.info.tlas_depth, "per-level stack entries",
          3 * (r.info.tlas_depth + r.info.blas_depth) + 2, "| host blas_depth", host.blas_depth, "tlas_depth", host.tlas_depth,
          "per-level stack entries", 3 * (host.tlas_depth + host.blas_depth) + 2)
    assert 3 * r.info.blas_depth + 2 > 64
    assert 3 * (r.info.tlas_depth + r.info.blas_depth) + 2 <= 160 * 1024 // (256 * 4)
    for schedule in ("megakernel", "wavefront"):
        assert_equals_oracle(r.render(seed=SEED, want_li=True, schedule=schedule)["li"].cpu().numpy(), li_ref, ("deep", schedule))
    monkeypatch.setenv("GBL_WF_NO_OVERLAP", "1")
    fresh = HipPathTracer(c.scene, 0, bvh="device")
    assert_equals_oracle(fresh.render(seed=SEED, want_li=True, schedule="wavefront")["li"].cpu().numpy(), li_ref, ("deep", "wavefront, no overlap"))


# ---------------------------------------------------------------------------
# several hundred instances
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bvh", BUILDERS)
def test_three_hundred_overlapping_instances(torch, scene_dir, bvh):
    """300 instances of few5 on a geometrically spaced line (world boxes overlap at every scale): radiance against the oracle,
    and after gbl_update_instances moves the first 10 against a fresh context of the edited scene."""
    from goblin_amd.renderer import HipPathTracer
    scene = gs.load_scene_text(json.dumps(meshes.instances_doc(300)), scene_dir)
    edited = gs.load_scene_text(json.dumps(meshes.instances_doc(300, moved=10)), scene_dir)
    assert scene.desc.num_instances == 301
    o = ob.Oracle(scene)
    li_ref, _ = o.li_replay(o.native_samples(SEED), threads=4)
    r = HipPathTracer(scene, 0, bvh=bvh)
    print(bvh, "tlas nodes", r.info.tlas_nodes, "depth", r.info.tlas_depth)
    for schedule in ("megakernel", "wavefront"):
        assert_equals_oracle(r.render(seed=SEED, want_li=True, schedule=schedule)["li"].cpu().numpy(), li_ref, ("instances", bvh, schedule))
    before = r.render(seed=SEED, want_li=True)["li"].cpu().numpy()
    r.update_instances(1, meshes.moved_transforms(10))   # (instance 0 is the floor)
    fresh = HipPathTracer(edited, 0, bvh=bvh)
    for schedule in ("megakernel", "wavefront"):
        after = r.render(seed=SEED, want_li=True, schedule=schedule)["li"].cpu().numpy()
        want = fresh.render(seed=SEED, want_li=True, schedule=schedule)["li"].cpu().numpy()
        assert not np.allclose(before, after)
        assert helpers.li_mismatch_fraction(after, want) <= 0.0
        assert helpers.rel_l2(after[:, :3], want[:, :3]) <= 1e-5
    oe = ob.Oracle(edited)
    assert_equals_oracle(after, oe.li_replay(oe.native_samples(SEED), threads=4)[0], ("instances, edited", bvh))
