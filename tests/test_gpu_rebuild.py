"""gbl_rebuild_mesh and gbl_mesh_tree_stats on the device: a deformed mesh's BLAS built again in place, and what its tree costs.

The bar is tests/test_gpu_refit.py's, whose frame and helpers these tests use (48 x 48, 4 spp, depth 5, SEED 31337, both
builders), and every radiance tolerance is zero:

- after a rebuild the mesh's slice of `tris` and `tri_bounds` is byte for byte a fresh DEVICE-built context's over the same
  positions, whichever builder made the rebuilt context, and the tree equals the fresh one slot by slot up to where its nodes
  are stored (lbvh_collapse numbers nodes through an atomic counter: node indices are never compared);
- it renders, bit for bit, what that fresh context renders and what the oracle says, under the tie rule and without it;
- tri_order and a deferred order are left alone; refusals leave every table's bytes alone;
- tree_stats' counts are meshes.lbvh_shape's, its sums the numpy restatement's (tests/rebuild_reference.py) over the node table
  read back, within N * 2^-52 relative -- the bound of a sum of N non-negative doubles in any order -- and two calls agree in
  every bit.  Which of a refitted and a rebuilt tree is cheaper is tools/rebuild_bench.py's finding and is not asserted.

The teeth are asserted, not assumed (both were checked with meshes.lbvh_shape on the CPU): on spiral, deep_spiral, urchin,
flatgrid and slivers either deformation changes the Morton order, so a rebuild that kept the old order cannot pass, and on the
jittered spiral and deep_spiral the tree needs more nodes than it had (59 -> 67, 297 -> 347), so a rebuild into the old
records cannot either.

Measured on an MI355X: the 54 tests take 7.6 s, the slowest 0.33 s; of the 200 tree_stats sums compared 185 are bit-equal to the
restatement's and the rest within 3.1e-16 relative.
"""
import numpy as np
import pytest

import meshes
import oracle_binding as ob
import rebuild_reference as rb
import refit_reference as rr
import test_gpu_refit as base
from test_gpu_refit import dirs, torch   # noqa: F401  (module fixtures)
from goblin_amd import _abi
from goblin_amd import scene as gs

pytestmark = pytest.mark.gpu
SEED, BUILDERS, SCHEDULES, HOWS = base.SEED, base.BUILDERS, base.SCHEDULES, base.HOWS
ORDER_CHANGES = ("spiral", "deep_spiral", "urchin", "flatgrid", "slivers")
NODES_GROW = {("spiral", "jitter"): (59, 67), ("deep_spiral", "jitter"): (297, 347)}
SMALLEST = ["few1", "few4", "few5", "few9", "urchin", "deep_spiral", "degenerate", "tiny"]
INVALID, UNSUPPORTED = _abi.GBL_ERR_INVALID, _abi.GBL_ERR_UNSUPPORTED
load, li_of, mesh_positions, same_topology = base.load, base.li_of, base.mesh_positions, base.same_topology
ALL_TABLES = base.TABLES + ("mesh_root",)


def tracer(scene, bvh="host"):
    from goblin_amd.renderer import HipPathTracer
    return HipPathTracer(scene, 0, bvh=bvh)


def all_tables(r):
    return {t: r._geometry(t) for t in ALL_TABLES}


def mesh_range(scene, m):
    """The mesh's records of `tris`: the running sum of the triangle meshes' counts, under either builder."""
    d = scene.desc
    first = sum(int(d.meshes[k].tri_count) for k in range(m) if d.meshes[k].shape == 0)
    return slice(first, first + int(d.meshes[m].tri_count))


def assert_mesh_equals(got, want, scene, m, what):
    """Mesh m of two contexts' tables: its triangles and bounds byte for byte, its tree up to numbering."""
    k = mesh_range(scene, m)
    for t in ("tris", "tri_bounds"):
        assert got[t][k].tobytes() == want[t][k].tobytes(), (what, m, t)
    return rb.same_tree(got["nodes"], got["mesh_root"][m], want["nodes"], want["mesh_root"][m])


def shapes(scene):
    """meshes.lbvh_shape per mesh of the scene (every mesh of these documents is a triangle mesh)."""
    return [meshes.lbvh_shape(P, I) for P, I in meshes.scene_meshes(scene)]


def assert_stats_are_the_restatement(r, m, what):
    got = r.tree_stats(m)
    assert got == r.tree_stats(m), (what, "two calls")          # (floats compared by value: no NaN on a valid tree, -0 never arises)
    want = rb.tree_stats(r._geometry("nodes"), r._geometry("mesh_root")[m])
    for f in ("nodes", "levels", "leaves"):
        assert got[f] == want[f], (what, f, got[f], want[f])
    assert got["root_area"] == want["root_area"], (what, got["root_area"], want["root_area"])
    for f, n in (("node_area", want["terms"][0]), ("tri_area", want["terms"][1])):
        err = abs(got[f] - want[f])
        print(*what, f, "terms", n, "got %.17g want %.17g rel %.2e bound %.2e" % (got[f], want[f], err / want[f] if want[f] else 0.0, n * 2.0 ** -52))
        assert err <= n * 2.0 ** -52 * want[f], (what, f, got[f], want[f], n)
    node_cost, tri_cost = rb.costs(got)
    assert (got["node_cost"], got["tri_cost"]) == (node_cost, tri_cost)
    return got


# ---------------------------------------------------------------------------
# 1: a rebuild without an edit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bvh", BUILDERS)
def test_rebuild_without_an_edit(torch, dirs, bvh):
    scene = load(meshes.scene_doc(meshes.ALL), dirs["a"])
    r = tracer(scene, bvh)
    li = {s: li_of(r, schedule=s, exact_ties=True) for s in SCHEDULES}
    before = all_tables(r)
    for m in range(scene.desc.num_meshes):
        r.rebuild_mesh(m)
    after = all_tables(r)
    assert after["tri_order"].tobytes() == before["tri_order"].tobytes()
    for s in SCHEDULES:
        assert torch.equal(li_of(r, schedule=s, exact_ties=True), li[s]), (bvh, s)
    compared = 0
    if bvh == "device":   # the same builder over the same positions
        for t in ("tris", "tri_bounds"):
            assert after[t].tobytes() == before[t].tobytes(), t
        for m in range(scene.desc.num_meshes):
            compared += assert_mesh_equals(after, before, scene, m, "no edit")
        assert compared > 400
    for m, shape in enumerate(shapes(scene)):
        got = r.tree_stats(m)
        assert (got["nodes"], got["levels"]) == (shape["nodes"], shape["depth"]), (bvh, m, got, shape["nodes"], shape["depth"])
        assert got["leaves"] == len(shape["leaves"])


# ---------------------------------------------------------------------------
# 2: edited, rebuilt == fresh
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("how", HOWS)
@pytest.mark.parametrize("name", base.RADIANCE_MESHES)
def test_an_edited_and_rebuilt_context_equals_a_fresh_device_built_one(torch, dirs, name, how):
    doc = meshes.scene_doc(name)
    scene_a, scene_b = load(doc, dirs["a"]), load(doc, dirs[how])
    same_topology(scene_a, scene_b)
    li_ref = base.oracle_li(scene_b)
    fresh = {bvh: tracer(scene_b, bvh) for bvh in BUILDERS}
    want = all_tables(fresh["device"])
    k = mesh_range(scene_a, 1)
    edited = {}
    for bvh in BUILDERS:
        r = edited[bvh] = tracer(scene_a, bvh)
        created = all_tables(r)
        nodes_created = r.tree_stats(1)["nodes"]
        base.edit_all(r, scene_b, only=[1])   # mesh 0 is the floor
        refitted = all_tables(r)
        r.rebuild_mesh(1)
        got = all_tables(r)
        assert_mesh_equals(got, want, scene_a, 1, (name, how, bvh))
        assert got["tri_order"].tobytes() == refitted["tri_order"].tobytes()
        if name in ORDER_CHANGES:   # the teeth
            assert got["tris"][k].tobytes() != refitted["tris"][k].tobytes(), (name, how, bvh)
            if bvh == "device":
                assert not np.array_equal(got["tris"]["shade"][k], created["tris"]["shade"][k]), (name, how, "the Morton order")
        if (name, how) in NODES_GROW and bvh == "device":
            assert (nodes_created, r.tree_stats(1)["nodes"]) == NODES_GROW[(name, how)]
    for schedule in SCHEDULES:
        li_fresh = li_of(fresh["device"], schedule=schedule, exact_ties=True)
        base.assert_equals_oracle(li_fresh, li_ref, (name, how, schedule, "fresh"))
        for bvh in BUILDERS:
            assert torch.equal(li_of(edited[bvh], schedule=schedule, exact_ties=True), li_fresh), (name, how, bvh, schedule)
        # lean kernels: their tie order follows the tree.  The precondition, on code this change does not touch: the two
        # builders' fresh trees agree; then the rebuilt trees must agree with the fresh device-built one
        lean = {bvh: li_of(fresh[bvh], schedule=schedule) for bvh in BUILDERS}
        assert torch.equal(lean["host"], lean["device"]), ("precondition", name, how, schedule)
        for bvh in BUILDERS:
            assert torch.equal(li_of(edited[bvh], schedule=schedule), lean["device"]), (name, how, bvh, schedule, "lean")


# ---------------------------------------------------------------------------
# 3: the smallest shapes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bvh", BUILDERS)
@pytest.mark.parametrize("name", SMALLEST)
def test_smallest_shapes(torch, dirs, name, bvh):
    """few1, few4: the root is a leaf and no slot is made; few5: the smallest tree; urchin: 64 triangles under one Morton code;
    deep_spiral: more than 64 stack entries, which the TLAS rebuild must follow (stretched: its tree keeps its 23 levels, where
    the jittered one has 21)."""
    how = "stretch" if name == meshes.DEEP else "jitter"
    scene_a, scene_b = load(meshes.scene_doc(name), dirs["a"]), load(meshes.scene_doc(name), dirs[how])
    tri_count = int(scene_a.desc.meshes[1].tri_count)
    r, fresh = tracer(scene_a, bvh), tracer(scene_b, "device")
    length = len(r._geometry("nodes"))
    base.edit_all(r, scene_b, only=[1])
    r.rebuild_mesh(1)
    got = all_tables(r)
    assert len(got["nodes"]) == length + (tri_count if tri_count > 4 else 0)
    assert_mesh_equals(got, all_tables(fresh), scene_a, 1, (name, bvh))
    shape = shapes(scene_b)[1]
    stats = assert_stats_are_the_restatement(r, 1, (name, bvh))
    assert (stats["nodes"], stats["levels"], stats["leaves"]) == (shape["nodes"], shape["depth"], len(shape["leaves"]))
    if tri_count <= 4:
        assert got["mesh_root"][1] < 0 and rr.leaf_range(got["mesh_root"][1]) == (mesh_range(scene_a, 1).start, tri_count)
        assert stats == {"nodes": 0, "levels": 0, "leaves": 1, "root_area": 0.0, "node_area": 0.0, "tri_area": 0.0, "node_cost": 0.0, "tri_cost": 0.0}
    if name == "few5":
        assert stats["nodes"] == 1
        if bvh == "device":
            assert base.tlas_facts(r) == base.tlas_facts(fresh), (base.tlas_facts(r), base.tlas_facts(fresh))
    assert r.info.blas_depth >= shape["depth"]
    if name == "deep_spiral":
        assert 3 * shape["depth"] > 64
    for schedule in SCHEDULES:
        assert torch.equal(li_of(r, schedule=schedule, exact_ties=True), li_of(fresh, schedule=schedule, exact_ties=True)), (name, bvh, schedule)


# ---------------------------------------------------------------------------
# 4: sequences
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bvh", BUILDERS)
def test_edits_and_rebuilds_in_sequence(torch, dirs, bvh):
    doc = meshes.scene_doc("spiral")
    A, B, Cc = load(doc, dirs["a"]), load(doc, dirs["jitter"]), load(doc, dirs["stretch"])
    PA, PB, PC = mesh_positions(A)[1], mesh_positions(B)[1], mesh_positions(Cc)[1]
    r = tracer(A, bvh)
    r.rebuild_mesh(1)
    first_a, li_a = all_tables(r), li_of(r, exact_ties=True)
    length = len(first_a["nodes"])
    # edit, rebuild, edit again: the refit over the rebuilt tree is the restatement applied to the tables read back after the rebuild
    r.update_vertices(1, PB)
    r.rebuild_mesh(1)
    rebuilt = all_tables(r)
    assert len(rebuilt["nodes"]) == length                       # the slot is reused
    r.update_vertices(1, PC)
    got = all_tables(r)
    nodes, tris, bounds = rebuilt["nodes"].copy(), rebuilt["tris"].copy(), rebuilt["tri_bounds"].copy()
    k = mesh_range(A, 1)
    records, _ = rr.refit_mesh(nodes, tris, bounds, base.shade_table(A), base.all_positions(Cc), rebuilt["mesh_root"][1], k.start, k.stop - k.start)
    assert len(records) == 67
    assert got["tris"].tobytes() == tris.tobytes() and got["tri_bounds"].tobytes() == bounds.tobytes()
    assert got["nodes"][records["node"]].tobytes() == nodes[records["node"]].tobytes()
    assert got["nodes"][records["node"]].tobytes() != rebuilt["nodes"][records["node"]].tobytes()
    assert torch.equal(li_of(r, exact_ties=True), li_of(tracer(Cc, bvh), exact_ties=True))
    # an identity edit after a rebuild rewrites every byte with its value
    r.rebuild_mesh(1)
    settled = all_tables(r)
    r.update_vertices(1, r.vertices(1))
    again = all_tables(r)
    for t in ALL_TABLES:
        if t != "nodes":
            assert again[t].tobytes() == settled[t].tobytes(), t
    live = rr.plan_walk(settled["nodes"], settled["mesh_root"][1])[0]["node"]
    assert again["nodes"][live].tobytes() == settled["nodes"][live].tobytes()
    # A -> B -> A, rebuilt at each step, is the first rebuild of A
    r.update_vertices(1, PB)
    r.rebuild_mesh(1)
    r.update_vertices(1, PA)
    r.rebuild_mesh(1)
    back = all_tables(r)
    assert len(back["nodes"]) == length
    assert_mesh_equals(back, first_a, A, 1, "A -> B -> A")
    assert back["tri_order"].tobytes() == first_a["tri_order"].tobytes()
    assert torch.equal(li_of(r, exact_ties=True), li_a)


@pytest.mark.parametrize("bvh", BUILDERS)
def test_two_meshes_rebuilt_in_either_order(torch, dirs, bvh):
    doc = meshes.scene_doc(["spiral", "urchin"])
    A, B = load(doc, dirs["a"]), load(doc, dirs["jitter"])
    want = tracer(B, "device")
    t_want = all_tables(want)
    length = len(tracer(A, bvh)._geometry("nodes"))
    for order in ((1, 2), (2, 1)):
        r = tracer(A, bvh)
        base.edit_all(r, B)
        for m in order:
            r.rebuild_mesh(m)
        got = all_tables(r)
        assert len(got["nodes"]) == length + 400 + 64, (bvh, order)     # one slot per mesh
        for m in (1, 2):
            assert_mesh_equals(got, t_want, A, m, (bvh, order))
        for s in SCHEDULES:
            assert torch.equal(li_of(r, schedule=s, exact_ties=True), li_of(want, schedule=s, exact_ties=True)), (bvh, order, s)


@pytest.mark.parametrize("bvh", BUILDERS)
def test_every_instance_follows_the_new_root(torch, dirs, bvh):
    doc = meshes.instances_doc(300)
    A, B = load(doc, dirs["a"]), load(doc, dirs["jitter"])
    same_topology(A, B)
    assert A.desc.num_instances == 301 and A.desc.num_meshes == 2
    r, want = tracer(A, bvh), tracer(B, "device")
    root = r._geometry("mesh_root")[1]
    r.update_vertices(1, mesh_positions(B)[1])
    r.rebuild_mesh(1)
    assert r._geometry("mesh_root")[1] != root
    li = li_of(r, exact_ties=True)
    assert torch.equal(li, li_of(want, exact_ties=True)), bvh
    base.assert_equals_oracle(li, base.oracle_li(B), ("300 instances", bvh))
    assert torch.equal(li_of(r), li_of(want)), (bvh, "lean")


@pytest.mark.parametrize("bvh", BUILDERS)
def test_rebuild_and_instance_edits_commute(torch, dirs, bvh):
    n, moved = 6, 2
    A, B = load(meshes.instances_doc(n), dirs["a"]), load(meshes.instances_doc(n), dirs["jitter"])
    want_r = tracer(load(meshes.instances_doc(n, moved=moved), dirs["jitter"]), "device")
    PB = mesh_positions(B)[1]
    one, other = tracer(A, bvh), tracer(A, bvh)
    one.update_vertices(1, PB)
    one.rebuild_mesh(1)
    one.update_instances(1, meshes.moved_transforms(moved))      # rebuild, then instances
    other.update_vertices(1, PB)
    other.update_instances(1, meshes.moved_transforms(moved))    # instances, then rebuild
    other.rebuild_mesh(1)
    for s in SCHEDULES:
        want = li_of(want_r, schedule=s, exact_ties=True)
        assert torch.equal(li_of(one, schedule=s, exact_ties=True), want), (bvh, s, "rebuild then instances")
        assert torch.equal(li_of(other, schedule=s, exact_ties=True), want), (bvh, s, "instances then rebuild")
    assert_mesh_equals(all_tables(one), all_tables(other), A, 1, bvh)
    assert one.instances() == other.instances()


# ---------------------------------------------------------------------------
# 5: a deferred tie order stays deferred
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bvh", BUILDERS)
def test_a_deferred_order_stays_deferred(torch, dirs, bvh):
    doc = meshes.scene_doc("spiral")
    A, B = load(doc, dirs["a"]), load(doc, dirs["jitter"])
    fresh = tracer(B, "device")
    assert fresh._geometry("tri_order").tobytes() != tracer(A, bvh)._geometry("tri_order").tobytes()   # the order is worth making
    r = tracer(A, bvh)
    r.update_vertices(1, torch.from_numpy(mesh_positions(B)[1]).to("cuda:0"), defer_order=True)
    assert r.order_pending(1) == 1
    r.rebuild_mesh(1)
    assert r.order_pending(1) == 1
    assert torch.equal(li_of(r), li_of(fresh)) and r.order_pending(1) == 1          # a lean render leaves it
    assert torch.equal(li_of(r, exact_ties=True), li_of(fresh, exact_ties=True)) and r.order_pending(1) == 0
    assert r._geometry("tri_order").tobytes() == fresh._geometry("tri_order").tobytes()


# ---------------------------------------------------------------------------
# 6: the other kernels
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bvh", BUILDERS)
def test_other_kernels_follow_the_rebuild(torch, dirs, bvh):
    """AO with 9 rays, Whitted, a replay render with counters and the first-hit records, on all meshes with the spiral jittered."""
    spiral = 1 + meshes.ALL.index("spiral")
    for method, ao in (("ao", 9), ("whitted", None), (None, None)):
        doc = meshes.scene_doc(meshes.ALL, method=method, ao_samples=ao)
        scene_a, scene_b = load(doc, dirs["a"]), load(doc, dirs["one"])
        r, fresh = tracer(scene_a, bvh), tracer(scene_b, "device")
        base.edit_all(r, scene_b, only=[spiral])
        r.rebuild_mesh(spiral)
        assert torch.equal(li_of(r), li_of(fresh)), (method, bvh)
        if method is None:
            samples = ob.Oracle(scene_b).native_samples(SEED)
            for schedule in SCHEDULES:
                out = r.render(replay_samples=samples, want_li=True, stats=True, schedule=schedule)
                want = fresh.render(replay_samples=samples, want_li=True, stats=True, schedule=schedule)
                assert torch.equal(out["li"], want["li"]), (bvh, schedule, "replay")
                assert out["stats"]["paths"] == want["stats"]["paths"] == scene_b.num_paths()
                if bvh == "device":   # every tree is the fresh context's up to numbering: the same nodes visited, the same triangles tested
                    assert {k: v for k, v in out["stats"].items() if k != "kernel_ms"} == {k: v for k, v in want["stats"].items() if k != "kernel_ms"}
            for exact in (False, True):
                got = r.render_aov(want_samples=True, seed=SEED, exact_ties=exact)
                want = fresh.render_aov(want_samples=True, seed=SEED, exact_ties=exact)
                assert torch.equal(got["samples_i32"], want["samples_i32"]), (bvh, exact, "aov records")


def test_scenes_beyond_the_lean_set_render_the_same_after_a_rebuild(torch, dirs):
    """A bundled image-textured scene and a scene with a directional light (not refused: nothing that light reads changes)."""
    ov = gs.config_overrides(resolution=(16, 16), spp=1, depth=3)
    doc = meshes.scene_doc("few9")
    doc["lights"].append({"name": "sun", "type": "directional", "radiance": [1, 1, 1], "direction": [0, -1, 0]})
    for what, scene in (("imagetex", gs.load_scene("imagetex", ov)), ("directional", load(doc, dirs["a"]))):
        r = tracer(scene, "host")
        before = li_of(r, exact_ties=True)
        rebuilt = 0
        for m in range(scene.desc.num_meshes):
            st = r.lib.gbl_rebuild_mesh(r.handle, m, 0)
            assert st == _abi.GBL_OK or (what == "imagetex" and st in (INVALID, UNSUPPORTED)), (what, m, st, r.lib.gbl_last_error(r.handle))
            rebuilt += st == _abi.GBL_OK
        assert rebuilt > 0, what
        assert torch.equal(li_of(r, exact_ties=True), before), what


# ---------------------------------------------------------------------------
# 7: refusals
# ---------------------------------------------------------------------------
def refused(r, status, needle, mesh, flags=0):
    before = all_tables(r)
    st = r.lib.gbl_rebuild_mesh(r.handle, mesh, flags)
    msg = r.lib.gbl_last_error(r.handle).decode()
    assert st == status and needle in msg, (st, msg)
    after = all_tables(r)
    for t in ALL_TABLES:
        assert after[t].tobytes() == before[t].tobytes(), (needle, t)


def test_refusals_leave_every_table_alone(torch):
    ov = gs.config_overrides(resolution=(16, 16), spp=1, depth=2)
    for bvh in BUILDERS:
        r = tracer(gs.load_scene("bunny", ov), bvh)          # mesh 0 the bunny, mesh 1 the floor
        before = li_of(r)
        assert r.lib.gbl_rebuild_mesh(None, 0, 0) == INVALID
        refused(r, INVALID, "out of range", 2)
        refused(r, INVALID, "out of range", 0xffffffff)
        refused(r, INVALID, "flags", 0, 1)
        refused(r, INVALID, "flags", 1, 0x80000000)
        with pytest.raises(_abi.GoblinError) as e:
            r.rebuild_mesh(2)
        assert e.value.status == INVALID
        assert torch.equal(li_of(r), before)
    r = tracer(gs.load_scene("cornell", ov))                  # mesh 0 is the quad its area light emits from
    before = li_of(r)
    refused(r, UNSUPPORTED, "area light", 0)
    assert torch.equal(li_of(r), before)
    r = tracer(gs.load_scene("ibl", ov))                      # its sphere and its disk have no tree
    shapes_ = [i for i in range(r.scene.desc.num_meshes) if r.scene.desc.meshes[i].shape != 0]
    assert shapes_
    for i in shapes_:
        refused(r, INVALID, "sphere or a disk", i)
        out = _abi.gbl_tree_stats()
        assert r.lib.gbl_mesh_tree_stats(r.handle, i, out) == INVALID
    assert r.lib.gbl_mesh_tree_stats(r.handle, 0, None) == INVALID
    assert r.lib.gbl_mesh_tree_stats(r.handle, r.scene.desc.num_meshes, _abi.gbl_tree_stats()) == INVALID


# ---------------------------------------------------------------------------
# 8: tree_stats
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bvh", BUILDERS)
def test_tree_stats_are_the_restatement(torch, dirs, bvh):
    """Fresh, after a refit and after a rebuild, on every mesh: more than one workgroup of plan records on deep_spiral (297 and
    347 nodes), a single lane on few5, none on few1."""
    doc = meshes.scene_doc(meshes.ALL)
    A, B = load(doc, dirs["a"]), load(doc, dirs["jitter"])
    r = tracer(A, bvh)
    n = A.desc.num_meshes
    fresh = [assert_stats_are_the_restatement(r, m, (bvh, "fresh", m)) for m in range(n)]
    assert max(s["nodes"] for s in fresh) > 256 and min(s["nodes"] for s in fresh) == 0
    base.edit_all(r, B)
    refitted = [assert_stats_are_the_restatement(r, m, (bvh, "refitted", m)) for m in range(n)]
    for a, b in zip(fresh, refitted):
        assert (a["nodes"], a["levels"], a["leaves"]) == (b["nodes"], b["levels"], b["leaves"])   # a refit keeps the tree's shape
    assert any(a["node_area"] != b["node_area"] for a, b in zip(fresh, refitted))
    for m in range(n):
        r.rebuild_mesh(m)
    rebuilt = [assert_stats_are_the_restatement(r, m, (bvh, "rebuilt", m)) for m in range(n)]
    for s, shape in zip(rebuilt, shapes(B)):
        assert (s["nodes"], s["levels"], s["leaves"]) == (shape["nodes"], shape["depth"], len(shape["leaves"]))
