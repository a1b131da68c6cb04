"""gbl_update_vertices, gbl_get_vertices and gbl_selftest_geometry on the device: a mesh's BLAS refitted in place.

The bar is the project's usual one and every tolerance is zero: an edited context holds, byte for byte, the tables the numpy
restatement (tests/refit_reference.py, pinned to the host packer by tests/test_refit_cpu.py) makes of the tables it held
before, and renders, bit for bit, what a freshly created context of the edited scene renders and what the oracle says.

Frames are tests/meshes.py's 48 x 48 at 4 spp, depth 5, SEED 31337.  The edited scene is the same document loaded from a
second directory in which the deformed mesh was written under the same file name (its index arrays are asserted identical),
and that scene's positions are what update_vertices is fed.  Two deformations (refit_reference.jitter / stretch): every
coordinate moved by up to a tenth of the mesh's radius of interest; and a scale by (1, 1.6, 0.7) with the odd vertices pushed
out, which takes the mesh bound out of its old box.

Two things the byte comparisons know.  A vertex edit rebuilds the TLAS as gbl_update_instances does, and a
host-built context's first TLAS refers to the hot prefix's copies where a rebuilt one refers to the nodes themselves: "the tables
before" are read after an instance edit that moves nothing (`settled`), and BLAS records are compared apart from the TLAS's
reserved ones.  And node records no reference leads to (a device build reserves more than it uses) hold whatever the allocation
held: two contexts are compared on the records their mesh roots lead to.

Measured on an MI355X: the 37 tests take 4.7 s; every radiance comparison printed flips 0.00000, relL2 0.00e+00.
"""
import ctypes as C
import json
import os
import shutil

import numpy as np
import pytest

import helpers
import meshes
import oracle_binding as ob
import refit_reference as rr
from goblin_amd import _abi
from goblin_amd import scene as gs

pytestmark = pytest.mark.gpu
SEED = 31337
BUILDERS = ("host", "device")
SCHEDULES = ("megakernel", "wavefront")
HOWS = ("jitter", "stretch")
TABLES = ("nodes", "tris", "tri_bounds", "tri_order")
RADIANCE_MESHES = ["few1", "few5", "few9", "spiral", "deep_spiral", "urchin", "flatgrid", "slivers", "tiny", "degenerate"]


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def deformed(name, how):
    V, F = meshes.mesh(name)
    radius = meshes.MESHES[name][1]
    return (rr.jitter(V, radius) if how == "jitter" else rr.stretch(V, radius)), F


@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    """Scene directories: "a" holds the meshes as generated, "jitter" / "stretch" every mesh deformed that way, "one" the
    meshes as generated but for a jittered spiral."""
    out = {}
    for key in ("a", "one") + HOWS:
        d = tmp_path_factory.mktemp("refit_" + key)
        meshes.write_meshes(d, meshes.ALL)
        if key in HOWS:
            for name in meshes.ALL:
                meshes.write_obj(os.path.join(str(d), name + ".obj"), *deformed(name, key))
        if key == "one":
            meshes.write_obj(os.path.join(str(d), "spiral.obj"), *deformed("spiral", "jitter"))
        out[key] = str(d)
    return out


def load(doc, scene_dir):
    return gs.load_scene_text(json.dumps(doc), scene_dir)


def same_topology(a, b):
    da, db = a.desc, b.desc
    assert da.num_triangles == db.num_triangles and da.num_vertices == db.num_vertices and da.num_meshes == db.num_meshes
    ia = np.ctypeslib.as_array(da.indices, shape=(da.num_triangles * 3,))
    ib = np.ctypeslib.as_array(db.indices, shape=(db.num_triangles * 3,))
    assert np.array_equal(ia, ib)


def mesh_positions(scene):
    """Per mesh of the scene (every mesh of these documents is a triangle mesh) its positions as loaded."""
    return [P for P, _ in meshes.scene_meshes(scene)]


def tables(r):
    return {t: r._geometry(t) for t in TABLES}


def assert_same_tables(got, want, what):
    for t in TABLES:
        assert got[t].tobytes() == want[t].tobytes(), (what, t, int((got[t].view(np.uint8).reshape(len(got[t]), -1) != want[t].view(np.uint8).reshape(len(want[t]), -1)).any(axis=1).sum()))


def tlas_slice(r, bvh):
    """Where the TLAS sits in the node array: its reserved records (one per instance) come behind the BLAS nodes of a host-built
    scene (device_scene.h) and ahead of them when the device builds the BLASes (api_context.hip)."""
    cap, n = max(1, int(r.info.instances)), len(r._geometry("nodes"))
    return slice(n - cap, n) if bvh == "host" else slice(0, cap)


def tlas_facts(r):
    """What an edit's TLAS tail publishes besides the tables: gbl_info's tlas_nodes and tlas_depth, and stack_entries.  An edited
    context is compared with a fresh one under the device builder, where neither holds a hot prefix, and on few5, whose one-node
    tree a refit cannot leave at another depth than a fresh build's."""
    return int(r.info.tlas_nodes), int(r.info.tlas_depth), int(r._instances_raw()["stack_entries"])


def blas_bytes(nodes, where):
    """The node array's bytes without the TLAS's reserved records."""
    keep = np.ones(len(nodes), bool)
    keep[where] = False
    return nodes[keep].tobytes()


def settled(r, bvh):
    """The tables once the TLAS is in its REBUILT form.  A vertex edit rebuilds the TLAS as gbl_update_instances does, and a
    host-built scene's first TLAS differs from any rebuilt one: gbl_create points its child references at the hot prefix's
    copies, a rebuild at the nodes themselves.  So "the tables before" are read after an instance edit that moves nothing;
    it may change TLAS records only, which is asserted."""
    t0 = tables(r)
    r.update_instances(0, r.instances()[:1])
    t1 = tables(r)
    for t in ("tris", "tri_bounds", "tri_order"):
        assert t0[t].tobytes() == t1[t].tobytes(), t
    assert blas_bytes(t0["nodes"], tlas_slice(r, bvh)) == blas_bytes(t1["nodes"], tlas_slice(r, bvh))
    return t1


def edit_all(r, scene_b, only=None):
    """Feed the tracer scene_b's positions, mesh by mesh (all of them, or the indices in `only`)."""
    for m, P in enumerate(mesh_positions(scene_b)):
        if only is None or m in only:
            r.update_vertices(m, P)


def shade_table(scene):
    """tri_shade as pack_blas fills it: absolute vertex ids per original triangle."""
    d = scene.desc
    I = np.ctypeslib.as_array(d.indices, shape=(d.num_triangles * 3,)).reshape(-1, 3)
    out = np.zeros(d.num_triangles, rr.SHADE)
    for m in range(d.num_meshes):
        gm = d.meshes[m]
        out["v"][gm.tri_offset:gm.tri_offset + gm.tri_count] = I[gm.tri_offset:gm.tri_offset + gm.tri_count] + gm.vertex_offset
    return out


def all_positions(scene):
    d = scene.desc
    return np.ctypeslib.as_array(d.positions, shape=(d.num_vertices * 3,)).reshape(-1, 3).astype(np.float32)


def restated(r, scene_a, scene_b, before):
    """The restatement applied to the tables read back before the edit, over scene_b's positions."""
    nodes, tris, bounds = before["nodes"].copy(), before["tris"].copy(), before["tri_bounds"].copy()
    roots = r._geometry("mesh_root")
    shade, P = shade_table(scene_a), all_positions(scene_b)
    tri_first = 0
    for m in range(scene_a.desc.num_meshes):
        gm = scene_a.desc.meshes[m]
        rr.refit_mesh(nodes, tris, bounds, shade, P, roots[m], tri_first, gm.tri_count)
        tri_first += gm.tri_count
    return {"nodes": nodes, "tris": tris, "tri_bounds": bounds}


def li_of(r, **kw):
    return r.render(seed=SEED, want_li=True, **kw)["li"]


def oracle_li(scene):
    o = ob.Oracle(scene)
    ref, _ = o.li_replay(o.native_samples(SEED), threads=4)
    assert np.isfinite(ref).all() and ref[:, :3].max() > 0
    return ref


def assert_equals_oracle(li, li_ref, what):
    li = li.cpu().numpy()
    assert np.isfinite(li).all(), what
    flips, rel = helpers.li_mismatch_fraction(li, li_ref), helpers.rel_l2(li[:, :3], li_ref[:, :3])
    print(*what, "flips %.5f relL2 %.2e" % (flips, rel))
    assert flips == 0.0 and rel == 0.0, (what, flips, rel)


# ---------------------------------------------------------------------------
# 1, 2: the tables
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bvh", BUILDERS)
@pytest.mark.parametrize("names", [meshes.ALL, [meshes.DEEP]], ids=["all", "deep_spiral"])
def test_identity_edit_rewrites_every_byte_with_its_value(torch, dirs, names, bvh):
    from goblin_amd.renderer import HipPathTracer
    scene = load(meshes.scene_doc(names), dirs["a"])
    r = HipPathTracer(scene, 0, bvh=bvh)
    li_before = li_of(r)
    before = settled(r, bvh)
    touched = 0
    for m in range(scene.desc.num_meshes):
        P = r.vertices(m)
        touched += len(P)
        r.update_vertices(m, P)
    assert touched == scene.desc.num_vertices
    assert_same_tables(tables(r), before, ("identity", bvh))
    assert torch.equal(li_of(r), li_before)


@pytest.mark.parametrize("bvh", BUILDERS)
@pytest.mark.parametrize("how", HOWS)
def test_device_refit_equals_the_restatement(torch, dirs, how, bvh):
    from goblin_amd.renderer import HipPathTracer
    doc = meshes.scene_doc(meshes.ALL)
    scene_a, scene_b = load(doc, dirs["a"]), load(doc, dirs[how])
    same_topology(scene_a, scene_b)
    r = HipPathTracer(scene_a, 0, bvh=bvh)
    before = tables(r)
    edit_all(r, scene_b)
    after = tables(r)
    want = restated(r, scene_a, scene_b, before)
    for t in ("tris", "tri_bounds"):
        assert after[t].tobytes() != before[t].tobytes(), t
        assert after[t].tobytes() == want[t].tobytes(), (how, bvh, t)
    where = tlas_slice(r, bvh)   # (the TLAS is rebuilt on the host: the radiance tests below are its check)
    assert blas_bytes(after["nodes"], where) != blas_bytes(before["nodes"], where)
    assert blas_bytes(after["nodes"], where) == blas_bytes(want["nodes"], where), (how, bvh, "nodes")
    fresh = HipPathTracer(scene_b, 0, bvh="host")
    assert after["tri_order"].tobytes() == fresh._geometry("tri_order").tobytes()
    if bvh == "host":   # (a fresh host tree over the deformed mesh is another tree; its triangle bounds by id are the same set)
        assert sorted(after["tri_bounds"].tobytes()[i:i + 32] for i in range(0, 32 * len(after["tri_bounds"]), 32)) == \
               sorted(fresh._geometry("tri_bounds").tobytes()[i:i + 32] for i in range(0, 32 * len(after["tri_bounds"]), 32))


# ---------------------------------------------------------------------------
# 3: edited == fresh == oracle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("how", HOWS)
@pytest.mark.parametrize("name", RADIANCE_MESHES)
def test_edited_context_renders_what_a_fresh_one_and_the_oracle_do(torch, dirs, name, how):
    from goblin_amd.renderer import HipPathTracer
    doc = meshes.scene_doc(name)
    scene_a, scene_b = load(doc, dirs["a"]), load(doc, dirs[how])
    same_topology(scene_a, scene_b)
    li_ref = oracle_li(scene_b)
    edited = {bvh: HipPathTracer(scene_a, 0, bvh=bvh) for bvh in BUILDERS}
    fresh = {bvh: HipPathTracer(scene_b, 0, bvh=bvh) for bvh in BUILDERS}
    before = {(bvh, s): li_of(edited[bvh], schedule=s, exact_ties=True) for bvh in BUILDERS for s in SCHEDULES}
    for bvh in BUILDERS:
        edit_all(edited[bvh], scene_b, only=[1])   # mesh 0 is the floor
    if name == "few5":
        assert tlas_facts(edited["device"]) == tlas_facts(fresh["device"]), (how, tlas_facts(edited["device"]), tlas_facts(fresh["device"]))
    for schedule in SCHEDULES:
        for bvh in BUILDERS:
            li = li_of(edited[bvh], schedule=schedule, exact_ties=True)
            assert torch.equal(li, li_of(fresh[bvh], schedule=schedule, exact_ties=True)), (name, how, bvh, schedule)
            assert_equals_oracle(li, li_ref, (name, how, bvh, schedule, "exact_ties"))
            assert not torch.equal(li, before[(bvh, schedule)]), (name, how, bvh, schedule)
        # lean kernels: their tie order follows the tree.  The precondition, on code this change does not touch: the two
        # builders' fresh trees agree; then the refitted trees must agree with them
        lean = {bvh: li_of(fresh[bvh], schedule=schedule) for bvh in BUILDERS}
        assert torch.equal(lean["host"], lean["device"]), ("precondition", name, how, schedule)
        for bvh in BUILDERS:
            assert torch.equal(li_of(edited[bvh], schedule=schedule), lean[bvh]), (name, how, bvh, schedule, "lean")


# ---------------------------------------------------------------------------
# 4: the other kernels
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bvh", BUILDERS)
def test_other_kernels_follow_the_edit(torch, dirs, bvh):
    """AO with 9 rays, Whitted, a replay render with counters and the first-hit records, on all meshes with the spiral jittered."""
    from goblin_amd.renderer import HipPathTracer
    spiral = 1 + meshes.ALL.index("spiral")
    for method, ao in (("ao", 9), ("whitted", None), (None, None)):
        doc = meshes.scene_doc(meshes.ALL, method=method, ao_samples=ao)
        scene_a, scene_b = load(doc, dirs["a"]), load(doc, dirs["one"])
        same_topology(scene_a, scene_b)
        r, fresh = HipPathTracer(scene_a, 0, bvh=bvh), HipPathTracer(scene_b, 0, bvh=bvh)
        before = li_of(r)
        edit_all(r, scene_b, only=[spiral])
        o = ob.Oracle(scene_b)
        samples = o.native_samples(SEED)
        li_ref, _ = o.li_replay(samples, threads=4)
        li = li_of(r)
        assert torch.equal(li, li_of(fresh)) and not torch.equal(li, before), (method, bvh)
        assert_equals_oracle(li, li_ref, (method or "path", bvh, "edited"))
        if method is None:
            for schedule in SCHEDULES:
                out = r.render(replay_samples=samples, want_li=True, stats=True, schedule=schedule)
                want = fresh.render(replay_samples=samples, want_li=True, stats=True, schedule=schedule)
                assert torch.equal(out["li"], want["li"]), (bvh, schedule, "replay")
                assert_equals_oracle(out["li"], li_ref, (bvh, schedule, "replay"))
                assert out["stats"]["paths"] == scene_b.num_paths()
            for exact in (False, True):
                got = r.render_aov(want_samples=True, seed=SEED, exact_ties=exact)
                want = fresh.render_aov(want_samples=True, seed=SEED, exact_ties=exact)
                assert torch.equal(got["samples_i32"], want["samples_i32"]), (bvh, exact, "aov records")


# ---------------------------------------------------------------------------
# 5: sequences and ranges
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bvh", BUILDERS)
def test_sequences_and_vertex_ranges(torch, dirs, bvh):
    from goblin_amd.renderer import HipPathTracer
    doc = meshes.scene_doc("spiral")
    A, B, Cc = load(doc, dirs["a"]), load(doc, dirs["jitter"]), load(doc, dirs["stretch"])
    same_topology(A, B)
    same_topology(A, Cc)
    r = HipPathTracer(A, 0, bvh=bvh)
    li_a = li_of(r, exact_ties=True)
    t_a = settled(r, bvh)
    PA, PB, PC = mesh_positions(A)[1], mesh_positions(B)[1], mesh_positions(Cc)[1]
    r.update_vertices(1, PB)
    t_b = tables(r)
    r.update_vertices(1, PC)
    assert torch.equal(li_of(r, exact_ties=True), li_of(HipPathTracer(Cc, 0, bvh=bvh), exact_ties=True))      # A -> B -> C == fresh C
    r.update_vertices(1, PB)
    assert_same_tables(tables(r), t_b, ("C -> B", bvh))
    r.update_vertices(1, PA)
    assert_same_tables(tables(r), t_a, ("A -> B -> C -> B -> A", bvh))                                         # ... -> A restores every byte
    assert torch.equal(li_of(r, exact_ties=True), li_a)
    # a sub-range at a time (first > 0) is the full edit
    k = len(PB) // 3
    r.update_vertices(1, PB[:k])
    r.update_vertices(1, PB[k:2 * k + 1], first=k)
    r.update_vertices(1, PB[2 * k + 1:], first=2 * k + 1)
    assert_same_tables(tables(r), t_b, ("sub-ranges", bvh))
    assert np.array_equal(r.vertices(1), PB)


@pytest.mark.parametrize("bvh", BUILDERS)
def test_instances_of_one_mesh_follow_and_instance_edits_commute(torch, dirs, bvh):
    from goblin_amd.renderer import HipPathTracer
    n, moved = 6, 2
    base_a, base_b = load(meshes.instances_doc(n), dirs["a"]), load(meshes.instances_doc(n), dirs["jitter"])
    moved_b = load(meshes.instances_doc(n, moved=moved), dirs["jitter"])
    same_topology(base_a, base_b)
    assert base_a.desc.num_instances == n + 1 and base_a.desc.num_meshes == 2
    PB = mesh_positions(base_b)[1]
    r = HipPathTracer(base_a, 0, bvh=bvh)
    before = li_of(r, exact_ties=True)
    r.update_vertices(1, PB)
    li = li_of(r, exact_ties=True)
    assert torch.equal(li, li_of(HipPathTracer(base_b, 0, bvh=bvh), exact_ties=True)) and not torch.equal(li, before)
    assert_equals_oracle(li, oracle_li(base_b), ("instances", bvh))
    want = {s: li_of(HipPathTracer(moved_b, 0, bvh=bvh), schedule=s, exact_ties=True) for s in SCHEDULES}
    r.update_instances(1, meshes.moved_transforms(moved))                       # vertices, then instances
    other = HipPathTracer(base_a, 0, bvh=bvh)
    other.update_instances(1, meshes.moved_transforms(moved))                   # instances, then vertices
    other.update_vertices(1, PB)
    for s in SCHEDULES:
        assert torch.equal(li_of(r, schedule=s, exact_ties=True), want[s]), (bvh, s, "vertices then instances")
        assert torch.equal(li_of(other, schedule=s, exact_ties=True), want[s]), (bvh, s, "instances then vertices")
    # the same tables either way (node records no reference leads to are never written and hold whatever the allocation held)
    got, want = tables(r), tables(other)
    for t in ("tris", "tri_bounds", "tri_order"):
        assert got[t].tobytes() == want[t].tobytes(), (bvh, t)
    live = np.concatenate([rr.plan_walk(got["nodes"], root)[0]["node"] for root in r._geometry("mesh_root")])
    assert len(live) > 0 and got["nodes"][live].tobytes() == want["nodes"][live].tobytes(), bvh


# ---------------------------------------------------------------------------
# 6: normals
# ---------------------------------------------------------------------------
def write_bunny_vn(src, dst, positions, normals):
    """bunny_vn.obj with its v (and, if given, vn) lines replaced, in file order."""
    vi = ni = 0
    with open(src) as f, open(dst, "w") as g:
        for line in f:
            if line.startswith("v "):
                g.write("v %.9g %.9g %.9g\n" % tuple(float(x) for x in positions[vi]))
                vi += 1
            elif line.startswith("vn ") and normals is not None:
                g.write("vn %.9g %.9g %.9g\n" % tuple(float(x) for x in normals[ni]))
                ni += 1
            else:
                g.write(line)
    assert vi == len(positions) and (normals is None or ni == len(normals))


def test_vertex_normals_follow_or_stay(torch, tmp_path):
    from goblin_amd.renderer import HipPathTracer
    models = os.path.join(gs.SCENE_DIR, "models")
    with open(os.path.join(gs.SCENE_DIR, "bunny.json")) as f:
        doc = json.load(f)
    gs._merge(doc, gs.config_overrides(resolution=(16, 16), spp=1, depth=2))
    doc["geometries"][0]["file"] = "models/bunny_vn.obj"
    doc["primitives"][0]["material"] = "white"   # a Lambert bunny: its shading normal is in every sample that meets it
    V = np.array([[float(x) for x in l.split()[1:4]] for l in open(os.path.join(models, "bunny_vn.obj")) if l.startswith("v ")], np.float32)
    N = np.array([[float(x) for x in l.split()[1:4]] for l in open(os.path.join(models, "bunny_vn.obj")) if l.startswith("vn ")], np.float32)
    c, s = np.float32(np.cos(0.4)), np.float32(np.sin(0.4))
    turn = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float32)
    V2 = ((V * np.array([1.0, 1.25, 1.0], np.float32)) @ turn.T).astype(np.float32)
    N2 = (N @ turn.T).astype(np.float32)
    scenes = {}
    for key, normals in (("both", N2), ("positions", None)):
        d = tmp_path / key
        (d / "models").mkdir(parents=True)
        shutil.copy(os.path.join(models, "plane.obj"), str(d / "models" / "plane.obj"))
        write_bunny_vn(os.path.join(models, "bunny_vn.obj"), str(d / "models" / "bunny_vn.obj"), V2, normals)
        scenes[key] = load(doc, str(d))
    scene_a = load(doc, gs.SCENE_DIR)
    assert scene_a.desc.meshes[0].has_normal
    va, vc = scene_a.desc.meshes[0].vertex_offset, scene_a.desc.meshes[0].vertex_count

    def normals_of(scene):
        return np.ctypeslib.as_array(scene.desc.normals, shape=(scene.desc.num_vertices * 3,)).reshape(-1, 3)[va:va + vc].astype(np.float32)
    for bvh in BUILDERS:
        results = {}
        for key in ("both", "positions"):
            same_topology(scene_a, scenes[key])
            r = HipPathTracer(scene_a, 0, bvh=bvh)
            before = li_of(r)
            P = mesh_positions(scenes[key])[0]
            r.update_vertices(0, P, normals=normals_of(scenes[key]) if key == "both" else None)
            results[key] = li_of(r)
            assert torch.equal(results[key], li_of(HipPathTracer(scenes[key], 0, bvh=bvh))), (bvh, key)
            assert not torch.equal(results[key], before)
        assert not torch.equal(results["both"], results["positions"])   # the old normals are visible


# ---------------------------------------------------------------------------
# 7, 8: refusals, vertices()
# ---------------------------------------------------------------------------
def refused(r, status, needle, *args):
    st = r.lib.gbl_update_vertices(r.handle, *args)
    msg = r.lib.gbl_last_error(r.handle).decode()
    assert st == status and needle in msg, (st, msg)


def test_refusals_leave_the_context_untouched(torch, dirs):
    from goblin_amd.renderer import HipPathTracer
    INVALID, UNSUPPORTED = _abi.GBL_ERR_INVALID, _abi.GBL_ERR_UNSUPPORTED
    ov = gs.config_overrides(resolution=(16, 16), spp=1, depth=2)
    good = np.zeros((4, 3), np.float32)
    ptr = good.ctypes.data
    # bunny.json: mesh 0 the bunny (no vertex normals), mesh 1 the floor
    r = HipPathTracer(gs.load_scene("bunny", ov), 0)
    before, t_before = li_of(r), tables(r)
    assert r.lib.gbl_update_vertices(None, 0, 0, 4, ptr, None) == INVALID
    refused(r, INVALID, "positions is NULL", 0, 0, 4, None, None)
    refused(r, INVALID, "out of range", 2, 0, 4, ptr, None)
    n = int(r.scene.desc.meshes[0].vertex_count)
    refused(r, INVALID, "vertex range", 0, n - 3, 4, ptr, None)
    refused(r, INVALID, "vertex range", 0, 0xffffffff, 4, ptr, None)
    for bad in (np.nan, np.inf, -np.inf):
        p = good.copy()
        p[2, 1] = bad
        refused(r, INVALID, "not finite", 0, 0, 4, p.ctypes.data, None)
    refused(r, INVALID, "has_normal", 0, 0, 4, ptr, ptr)
    assert_same_tables(tables(r), t_before, "bunny after refusals")
    assert torch.equal(li_of(r), before) and np.array_equal(r.vertices(0)[:4], mesh_positions(r.scene)[0][:4])
    # cornell.json: mesh 0 is the quad its area light emits from
    r = HipPathTracer(gs.load_scene("cornell", ov), 0)
    before = li_of(r)
    refused(r, UNSUPPORTED, "area light", 0, 0, 4, ptr, None)
    assert torch.equal(li_of(r), before)
    # ibl.json: an image based light is sized by the scene bound
    r = HipPathTracer(gs.load_scene("ibl", ov), 0)
    before = li_of(r)
    m = next(i for i in range(r.scene.desc.num_meshes) if r.scene.desc.meshes[i].shape == 0)
    refused(r, UNSUPPORTED, "scene bound", m, 0, 1, ptr, None)
    for i in range(r.scene.desc.num_meshes):   # its sphere and its disk have no vertices
        if r.scene.desc.meshes[i].shape != 0:
            refused(r, INVALID, "sphere or a disk", i, 0, 1, ptr, None)
    with pytest.raises(_abi.GoblinError) as e:
        r.update_vertices(m, good[:1])
    assert e.value.status == UNSUPPORTED
    assert torch.equal(li_of(r), before)
    # a directional light
    doc = meshes.scene_doc("few5")
    doc["lights"].append({"name": "sun", "type": "directional", "radiance": [1, 1, 1], "direction": [0, -1, 0]})
    r = HipPathTracer(load(doc, dirs["a"]), 0)
    refused(r, UNSUPPORTED, "directional", 1, 0, 4, ptr, None)


def test_vertices_returns_what_the_context_holds(torch, dirs):
    from goblin_amd.renderer import HipPathTracer
    doc = meshes.scene_doc(["few5", "spiral"])
    A, B = load(doc, dirs["a"]), load(doc, dirs["jitter"])
    r = HipPathTracer(A, 0, bvh="device")
    for m, P in enumerate(mesh_positions(A)):
        assert np.array_equal(r.vertices(m), P)
    PB = mesh_positions(B)
    r.update_vertices(2, PB[2])
    assert np.array_equal(r.vertices(2), PB[2]) and np.array_equal(r.vertices(1), mesh_positions(A)[1])
    buf = np.zeros((3, 3), np.float32)
    assert r.lib.gbl_get_vertices(r.handle, 2, 5, 3, buf.ctypes.data) == _abi.GBL_OK and np.array_equal(buf, PB[2][5:8])
    for args in ((None, 2, 0, 1, buf.ctypes.data), (r.handle, 2, 0, 1, None), (r.handle, 3, 0, 1, buf.ctypes.data),
                 (r.handle, 2, len(PB[2]), 1, buf.ctypes.data)):
        assert r.lib.gbl_get_vertices(*args) == _abi.GBL_ERR_INVALID, args
    total = C.c_uint64()
    assert r.lib.gbl_selftest_geometry(r.handle, 1, 0, 0, None, C.byref(total)) == _abi.GBL_OK and total.value == r.info.triangles
    assert r.lib.gbl_selftest_geometry(r.handle, 5, 0, 0, None, C.byref(total)) == _abi.GBL_ERR_INVALID
    assert r.lib.gbl_selftest_geometry(r.handle, 1, total.value, 1, buf.ctypes.data, None) == _abi.GBL_ERR_INVALID
