"""gbl_update_vertices_device, gbl_get_vertices_device, gbl_order_pending and gbl_render_motion_deform_device on the device.

The bar is tests/test_gpu_refit.py's, whose frame and helpers these tests use (48 x 48, 4 spp, depth 5, SEED 31337, both
builders), and every tolerance is zero:

- a context edited through update_vertices(tensor) holds, byte for byte, the tables of a twin edited through
  update_vertices(numpy): the five geometry tables (every node record a mesh root leads to and the TLAS's used records; the
  whole node array too where the host built it -- records no reference leads to hold whatever a device build's allocation
  held), the instances and gbl_info; vertices() and vertices(device=True) return the input;
- it renders, bit for bit, what a fresh context of the edited scene renders and what the oracle says;
- a deferred tie order stays pending through every lean call and is made by the first call that reads it;
- the lazy host mirror and the device form of the deforming-mesh motion planes equal their host forms bit for bit;
- every refusal leaves the tables' bytes alone and words itself as the host entry does where that has the refusal.

Instance records and instance bounds have no read-back hook: the TLAS records quantised from them are compared, and the
renders.  The mesh bound's own bits (+0 against -0) reach the tables only where the instance transform and the quantiser's
nudge keep them; test_the_bound_breaks_ties_on_the_lower_vertex feeds both orders and compares what the tables do carry.

The precondition of the deferred-order tests is asserted, not assumed: the jittered spiral's tri_order slice differs from the
undeformed one's, so a context that never made the order cannot pass.

Measured on an MI355X: the 41 tests take 5.1 s, the slowest 0.4 s; every radiance comparison printed flips 0.00000, relL2 0.00e+00.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import meshes
import oracle_binding as ob
import refit_reference as rr
import test_gpu_refit as base
from test_gpu_refit import dirs, torch   # noqa: F401  (module fixtures)
from goblin_amd import _abi
from goblin_amd import scene as gs

pytestmark = pytest.mark.gpu
SEED, BUILDERS, SCHEDULES, HOWS = base.SEED, base.BUILDERS, base.SCHEDULES, base.HOWS
TABLE_MESHES = ["few1", "few5", "spiral", "deep_spiral", "flatgrid", "degenerate"]
ALL_TABLES = base.TABLES + ("mesh_root",)
INVALID, UNSUPPORTED = _abi.GBL_ERR_INVALID, _abi.GBL_ERR_UNSUPPORTED
load, li_of, mesh_positions, same_topology = base.load, base.li_of, base.mesh_positions, base.same_topology


def tracer(scene, bvh="host"):
    from goblin_amd.renderer import HipPathTracer
    return HipPathTracer(scene, 0, bvh=bvh)


def all_tables(r):
    return {t: r._geometry(t) for t in ALL_TABLES}


def used_nodes(r, t, bvh):
    """The node records something refers to: each mesh root's subtree and the TLAS's used records."""
    live = np.concatenate([rr.plan_walk(t["nodes"], root)[0]["node"] for root in t["mesh_root"]])
    where = base.tlas_slice(r, bvh)
    tlas = np.arange(where.start, where.start + int(r.info.tlas_nodes))
    return t["nodes"][np.concatenate([live, tlas])].tobytes()


def assert_twins(a, b, bvh, what):
    """Two contexts hold the same tables, instances and scene facts."""
    ta, tb = all_tables(a), all_tables(b)
    for t in ("tris", "tri_bounds", "tri_order", "mesh_root"):
        assert ta[t].tobytes() == tb[t].tobytes(), (what, t)
    assert used_nodes(a, ta, bvh) == used_nodes(b, tb, bvh), (what, "nodes")
    if bvh == "host":
        assert ta["nodes"].tobytes() == tb["nodes"].tobytes(), (what, "the whole node array")
    assert a.instances() == b.instances(), what
    for f, _ in _abi.gbl_info._fields_:
        if f not in ("build_ms", "window"):
            assert getattr(a.info, f) == getattr(b.info, f), (what, f)
    return ta


def on_device(torch, P, offset=5):
    """P as a tensor on the device that does not start at its storage's start."""
    buf = torch.zeros((len(P) + offset, 3), dtype=torch.float32, device="cuda:0")
    buf[offset:] = torch.from_numpy(np.ascontiguousarray(P, np.float32))
    t = buf[offset:]
    assert t.storage_offset() == 3 * offset and t.is_contiguous()
    return t


# ---------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bvh", BUILDERS)
@pytest.mark.parametrize("how", HOWS)
def test_a_device_edit_leaves_the_host_edits_tables(torch, dirs, how, bvh):
    doc = meshes.scene_doc(TABLE_MESHES)
    scene_a, scene_b = load(doc, dirs["a"]), load(doc, dirs[how])
    same_topology(scene_a, scene_b)
    host, dev = tracer(scene_a, bvh), tracer(scene_a, bvh)
    before = all_tables(dev)
    for m, P in enumerate(mesh_positions(scene_b)):
        host.update_vertices(m, P)
        dev.update_vertices(m, on_device(torch, P))
        assert dev.order_pending(m) == 0
    after = assert_twins(host, dev, bvh, (how, bvh))
    for t in ("tris", "tri_bounds", "tri_order"):
        assert after[t].tobytes() != before[t].tobytes(), t
    for m, P in enumerate(mesh_positions(scene_b)):
        assert np.array_equal(dev.vertices(m), P) and np.array_equal(dev.vertices(m, device=True).cpu().numpy(), P), m
    assert torch.equal(li_of(dev, exact_ties=True), li_of(host, exact_ties=True))


@pytest.mark.parametrize("bvh", BUILDERS)
def test_the_bound_breaks_ties_on_the_lower_vertex(torch, dirs, bvh):
    """few5's fifteen vertices moved so that the lowest x, y and z and the highest x, y and z are each a zero met twice: +0 at
    one vertex and -0 at another, in both orders.  mesh_object_bound keeps the first vertex's bits."""
    scene = load(meshes.scene_doc("few5"), dirs["a"])
    P0 = mesh_positions(scene)[1]
    for flip in (False, True):
        for side in (1.0, -1.0):   # all coordinates >= 0: the zeros are the lowest; all <= 0: the highest
            P = (np.abs(P0) * np.float32(side) + np.float32(side * 0.25)).astype(np.float32)
            zeros = np.array([0.0, -0.0], np.float32)[::-1 if flip else 1]
            P[3], P[11] = zeros[0], zeros[1]
            assert np.signbit(P[3, 0]) != np.signbit(P[11, 0]) and (P * side >= 0).all()
            host, dev = tracer(scene, bvh), tracer(scene, bvh)
            host.update_vertices(1, P)
            dev.update_vertices(1, on_device(torch, P))
            assert_twins(host, dev, bvh, ("zeros", flip, side))
            assert np.array_equal(dev.vertices(1).view(np.uint32), P.view(np.uint32))
            assert torch.equal(li_of(dev), li_of(host))


@pytest.mark.parametrize("bvh", BUILDERS)
def test_sub_ranges_at_the_wave_and_workgroup_edges(torch, dirs, bvh):
    doc = meshes.scene_doc("spiral")
    A, B = load(doc, dirs["a"]), load(doc, dirs["jitter"])
    same_topology(A, B)
    PA, PB = mesh_positions(A)[1], mesh_positions(B)[1]
    n = len(PA)
    assert n > 257
    host, dev = tracer(A, bvh), tracer(A, bvh)
    want = PA.copy()
    for count in (0, 1, 63, 64, 65, 257):
        for first in (0, n - count):
            src = PB if (count + first) % 2 else PA   # (alternate, so that every edit changes something)
            part = src[first:first + count]
            host.update_vertices(1, part, first=first)
            dev.update_vertices(1, on_device(torch, part, offset=7), first=first)
            want[first:first + count] = part
            assert_twins(host, dev, bvh, (count, first))
            assert np.array_equal(dev.vertices(1), want) and np.array_equal(dev.vertices(1, device=True).cpu().numpy(), want), (count, first)
    buf = torch.zeros((3, 3), dtype=torch.float32, device="cuda:0")
    assert dev.lib.gbl_get_vertices_device(dev.handle, 1, 5, 3, buf.data_ptr()) == _abi.GBL_OK and np.array_equal(buf.cpu().numpy(), want[5:8])
    for args in ((None, 1, 0, 1, buf.data_ptr()), (dev.handle, 1, 0, 1, None), (dev.handle, 9, 0, 1, buf.data_ptr()), (dev.handle, 1, n, 1, buf.data_ptr())):
        assert dev.lib.gbl_get_vertices_device(*args) == INVALID, args


# ---------------------------------------------------------------------------
# radiance
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("how", HOWS)
@pytest.mark.parametrize("name", TABLE_MESHES)
def test_a_device_edit_renders_what_a_fresh_context_and_the_oracle_do(torch, dirs, name, how):
    doc = meshes.scene_doc(name)
    scene_a, scene_b = load(doc, dirs["a"]), load(doc, dirs[how])
    same_topology(scene_a, scene_b)
    li_ref = base.oracle_li(scene_b)
    PB = on_device(torch, mesh_positions(scene_b)[1])
    for bvh in BUILDERS:
        edited, fresh = tracer(scene_a, bvh), tracer(scene_b, bvh)
        before = li_of(edited, exact_ties=True)
        edited.update_vertices(1, PB)   # mesh 0 is the floor
        if name == "few5" and bvh == "device":
            assert base.tlas_facts(edited) == base.tlas_facts(fresh), (how, base.tlas_facts(edited), base.tlas_facts(fresh))
        for schedule in SCHEDULES:
            li = li_of(edited, schedule=schedule, exact_ties=True)
            assert torch.equal(li, li_of(fresh, schedule=schedule, exact_ties=True)), (name, how, bvh, schedule)
            base.assert_equals_oracle(li, li_ref, (name, how, bvh, schedule, "exact_ties"))
            assert not torch.equal(li, before), (name, how, bvh, schedule)
            assert torch.equal(li_of(edited, schedule=schedule), li_of(fresh, schedule=schedule)), (name, how, bvh, schedule, "lean")


@pytest.mark.parametrize("bvh", BUILDERS)
def test_other_kernels_follow_a_device_edit(torch, dirs, bvh):
    """AO with 9 rays, Whitted, a replay render with counters and the first-hit records, on all meshes with the spiral jittered."""
    spiral = 1 + meshes.ALL.index("spiral")
    for method, ao in (("ao", 9), ("whitted", None), (None, None)):
        doc = meshes.scene_doc(meshes.ALL, method=method, ao_samples=ao)
        scene_a, scene_b = load(doc, dirs["a"]), load(doc, dirs["one"])
        same_topology(scene_a, scene_b)
        r, fresh = tracer(scene_a, bvh), tracer(scene_b, bvh)
        before = li_of(r)
        r.update_vertices(spiral, on_device(torch, mesh_positions(scene_b)[spiral]))
        o = ob.Oracle(scene_b)
        samples = o.native_samples(SEED)
        li_ref, _ = o.li_replay(samples, threads=4)
        li = li_of(r)
        assert torch.equal(li, li_of(fresh)) and not torch.equal(li, before), (method, bvh)
        base.assert_equals_oracle(li, li_ref, (method or "path", bvh, "edited"))
        if method is None:
            for schedule in SCHEDULES:
                out = r.render(replay_samples=samples, want_li=True, stats=True, schedule=schedule)
                want = fresh.render(replay_samples=samples, want_li=True, stats=True, schedule=schedule)
                assert torch.equal(out["li"], want["li"]), (bvh, schedule, "replay")
                base.assert_equals_oracle(out["li"], li_ref, (bvh, schedule, "replay"))
                assert out["stats"]["paths"] == scene_b.num_paths()
            for exact in (False, True):
                got = r.render_aov(want_samples=True, seed=SEED, exact_ties=exact)
                want = fresh.render_aov(want_samples=True, seed=SEED, exact_ties=exact)
                assert torch.equal(got["samples_i32"], want["samples_i32"]), (bvh, exact, "aov records")


@pytest.mark.parametrize("bvh", BUILDERS)
def test_there_and_back_returns_the_first_renders_bits(torch, dirs, bvh):
    doc = meshes.scene_doc("spiral")
    A, B = load(doc, dirs["a"]), load(doc, dirs["stretch"])
    PA, PB = on_device(torch, mesh_positions(A)[1]), on_device(torch, mesh_positions(B)[1])
    r = tracer(A, bvh)
    li_a, lean_a = li_of(r, exact_ties=True), li_of(r)
    t_a = base.settled(r, bvh)
    r.update_vertices(1, PB)
    assert not torch.equal(li_of(r, exact_ties=True), li_a)
    r.update_vertices(1, PA)
    base.assert_same_tables(base.tables(r), t_a, ("A -> B -> A", bvh))
    assert torch.equal(li_of(r, exact_ties=True), li_a) and torch.equal(li_of(r), lean_a)


# ---------------------------------------------------------------------------
# the deferred tie order
# ---------------------------------------------------------------------------
def spiral_pair(dirs):
    doc = meshes.scene_doc(["few5", "spiral"])
    A, B = load(doc, dirs["a"]), load(doc, dirs["one"])   # "one": the spiral jittered, everything else as generated
    same_topology(A, B)
    return A, B


def order_slice(r, m):
    gm = r.scene.desc.meshes[m]
    return r._geometry("tri_order")[gm.tri_offset:gm.tri_offset + gm.tri_count].tobytes()


READERS = ("exact_ties", "replay", "collect_stats", "tri_order", "host_update", "ext_scene")


@pytest.mark.parametrize("bvh", BUILDERS)
@pytest.mark.parametrize("reader", READERS)
def test_a_deferred_order_waits_for_its_first_reader(torch, dirs, reader, bvh):
    A, B = spiral_pair(dirs)
    few5, spiral = 1, 2
    r, fresh = tracer(A, bvh), tracer(B, bvh)
    PB = mesh_positions(B)
    # the precondition: without it nothing below could fail
    assert order_slice(tracer(A, bvh), spiral) != order_slice(fresh, spiral)
    assert [r.order_pending(m) for m in range(3)] == [0, 0, 0]
    r.update_vertices(spiral, on_device(torch, PB[spiral]), defer_order=True)
    assert r.order_pending(spiral) == 1 and r.order_pending(few5) == 0
    r.update_vertices(few5, on_device(torch, PB[few5]))   # another mesh, undeferred: the spiral stays pending
    assert r.order_pending(spiral) == 1 and r.order_pending(few5) == 0
    # lean calls: right, and the order stays pending
    cam = r.camera()
    for schedule in SCHEDULES:
        assert torch.equal(li_of(r, schedule=schedule), li_of(fresh, schedule=schedule)), (schedule, "lean render")
        assert r.order_pending(spiral) == 1, (schedule, "lean render")
    got, want = r.render_aov(want_samples=True, seed=SEED), fresh.render_aov(want_samples=True, seed=SEED)
    assert torch.equal(got["samples_i32"], want["samples_i32"]) and r.order_pending(spiral) == 1
    assert torch.equal(r.motion(cam, None), fresh.motion(cam, None)) and r.order_pending(spiral) == 1
    assert torch.equal(r.motion(cam, None, prev_vertices={spiral: on_device(torch, mesh_positions(A)[spiral])}),
                       fresh.motion(cam, None, prev_vertices={spiral: mesh_positions(A)[spiral]})) and r.order_pending(spiral) == 1
    # the first reader
    if reader == "exact_ties":
        assert torch.equal(li_of(r, exact_ties=True), li_of(fresh, exact_ties=True))
    elif reader == "replay":
        o = ob.Oracle(B)
        samples = o.native_samples(SEED)
        for schedule in SCHEDULES[:1]:
            assert torch.equal(r.render(replay_samples=samples, want_li=True, schedule=schedule)["li"],
                               fresh.render(replay_samples=samples, want_li=True, schedule=schedule)["li"])
    elif reader == "collect_stats":
        assert torch.equal(r.render(seed=SEED, want_li=True, stats=True)["li"], fresh.render(seed=SEED, want_li=True, stats=True)["li"])
    elif reader == "tri_order":
        assert r._geometry("tri_order").tobytes() == fresh._geometry("tri_order").tobytes()
    elif reader == "host_update":
        r.update_vertices(spiral, PB[spiral][:10])
    elif reader == "ext_scene":   # a thin lens takes every call to the EXT kernels
        for t in (r, fresh):
            t.update_camera(lens_radius=0.01)
        assert torch.equal(li_of(r), li_of(fresh))
    assert r.order_pending(spiral) == 0, reader
    assert order_slice(r, spiral) == order_slice(fresh, spiral), reader
    if reader == "ext_scene":
        for t in (r, fresh):
            t.update_camera(lens_radius=0.0)
    li_ref = base.oracle_li(B)
    for schedule in SCHEDULES:
        li = li_of(r, schedule=schedule, exact_ties=True)
        assert torch.equal(li, li_of(fresh, schedule=schedule, exact_ties=True)), (reader, schedule)
        base.assert_equals_oracle(li, li_ref, (reader, bvh, schedule, "after the deferred order"))
    assert r.order_pending(spiral) == 0


# ---------------------------------------------------------------------------
# the host mirror
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bvh", BUILDERS)
def test_the_host_mirror_follows_device_edits(torch, dirs, bvh):
    A, B = spiral_pair(dirs)
    spiral = 2
    PA, PB = mesh_positions(A)[spiral], mesh_positions(B)[spiral]
    dev, host = tracer(A, bvh), tracer(A, bvh)
    dev.update_vertices(spiral, on_device(torch, PB), defer_order=True)
    host.update_vertices(spiral, PB)
    assert np.array_equal(dev.vertices(spiral), PB) and dev.order_pending(spiral) == 1   # (reading the mirror is no reader of the order)
    # previous poses from the host, after a device edit
    cam = dev.camera()
    assert torch.equal(dev.motion(cam, None, prev_vertices={spiral: PA}), host.motion(cam, None, prev_vertices={spiral: PA}))
    # a host edit of a sub-range lands on the device edit
    dev2 = tracer(A, bvh)
    dev2.update_vertices(spiral, on_device(torch, PB), defer_order=True)
    k = len(PA) // 3
    for t in (dev2, host):
        t.update_vertices(spiral, PA[k:2 * k], first=k)
    union = PB.copy()
    union[k:2 * k] = PA[k:2 * k]
    assert np.array_equal(dev2.vertices(spiral), union) and np.array_equal(dev2.vertices(spiral, device=True).cpu().numpy(), union)
    assert dev2.order_pending(spiral) == 0
    assert_twins(host, dev2, bvh, "host sub-range over a device edit")
    assert torch.equal(li_of(dev2, exact_ties=True), li_of(host, exact_ties=True))


# ---------------------------------------------------------------------------
# motion planes from device poses
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bvh", BUILDERS)
def test_device_poses_give_the_host_forms_planes(torch, dirs, bvh):
    A, B = spiral_pair(dirs)
    few5, spiral = 1, 2
    PA, PB = mesh_positions(A), mesh_positions(B)
    r = tracer(A, bvh)
    r.update_vertices(spiral, on_device(torch, PB[spiral]), defer_order=True)
    cam = r.camera()
    normal = r.render_aov(seed=SEED)["normal"]
    plain = r.motion(cam, None, normal=normal)
    dA = {m: on_device(torch, PA[m]) for m in (few5, spiral)}
    # a deformed mesh
    want = r.motion(cam, None, normal=normal, prev_vertices={spiral: PA[spiral]})
    assert not torch.equal(want, plain)
    assert torch.equal(r.motion(cam, None, normal=normal, prev_vertices={spiral: dA[spiral]}), want)
    assert torch.equal(r.motion(cam, None, normal=normal, prev_vertices={spiral: r.vertices(spiral, device=True)}), plain)   # listed, unchanged
    assert torch.equal(r.motion(cam, None, normal=normal, prev_vertices={few5: dA[few5]}), plain)                             # (few5 was never edited)
    # two meshes, one of them unchanged, in both orders
    for order in ((few5, spiral), (spiral, few5)):
        assert torch.equal(r.motion(cam, None, normal=normal, prev_vertices={m: dA[m] for m in order}),
                           r.motion(cam, None, normal=normal, prev_vertices={m: PA[m] for m in order})), order
        assert torch.equal(r.motion(cam, None, normal=normal, prev_vertices={m: dA[m] for m in order}), want), order
    # both deformed
    r.update_vertices(few5, on_device(torch, (PA[few5] * np.float32(1.1)).astype(np.float32)))
    both = r.motion(cam, None, prev_vertices={few5: PA[few5], spiral: PA[spiral]})
    assert torch.equal(r.motion(cam, None, prev_vertices={few5: dA[few5], spiral: dA[spiral]}), both)
    assert r.order_pending(spiral) == 1
    with pytest.raises(ValueError):
        r.motion(cam, None, prev_vertices={few5: dA[few5], spiral: PA[spiral]})
    bad = dA[spiral].clone()
    bad[-1, 2] = float("nan")
    with pytest.raises(_abi.GoblinError) as e:
        r.motion(cam, None, prev_vertices={few5: dA[few5], spiral: bad})
    assert e.value.status == INVALID and "prev_meshes[1]: a position of vertex %d is not finite" % (len(bad) - 1) in str(e.value)
    assert torch.equal(r.motion(cam, None, prev_vertices={few5: dA[few5], spiral: dA[spiral]}), both)


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------
def refused(r, status, needle, mesh, first, count, positions, normals, flags=0, host=None):
    """The device entry refuses with `status` and a message holding `needle`; `host` (positions, normals as arrays, or pointers)
    is what the host entry is given for the same call, whose message must then be the same."""
    ptr = lambda x: None if x is None else x if isinstance(x, int) else x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data
    st = r.lib.gbl_update_vertices_device(r.handle, mesh, first, count, ptr(positions), ptr(normals), flags)
    msg = r.lib.gbl_last_error(r.handle).decode()
    assert st == status and needle in msg, (st, msg)
    if host is not None:
        assert r.lib.gbl_update_vertices(r.handle, mesh, first, count, ptr(host[0]), ptr(host[1])) == status
        assert r.lib.gbl_last_error(r.handle).decode() == msg


def test_refusals_leave_the_tables_alone(torch, dirs, tmp_path):
    ov = gs.config_overrides(resolution=(16, 16), spp=1, depth=2)
    good_h = np.zeros((4, 3), np.float32)
    good = torch.zeros((4, 3), dtype=torch.float32, device="cuda:0")
    # bunny.json: mesh 0 the bunny (no vertex normals), mesh 1 the floor
    r = tracer(gs.load_scene("bunny", ov))
    before, t_before = li_of(r), all_tables(r)
    n = int(r.scene.desc.meshes[0].vertex_count)
    refused(r, INVALID, "positions is NULL", 0, 0, 4, None, None, host=(None, None))
    refused(r, INVALID, "out of range", 2, 0, 4, good, None, host=(good_h, None))
    refused(r, INVALID, "vertex range", 0, n - 3, 4, good, None, host=(good_h, None))
    refused(r, INVALID, "vertex range", 0, 0xffffffff, 4, good, None, host=(good_h, None))
    refused(r, INVALID, "has_normal", 0, 0, 4, good, good, host=(good_h, good_h))
    refused(r, INVALID, "flags", 0, 0, 4, good, None, flags=2)
    refused(r, INVALID, "flags", 0, 0, 4, good, None, flags=0x80000001)
    for where in ((0, 0), (3, 2)):   # the first and the last float
        for bad in (np.nan, np.inf, -np.inf):
            p_h = good_h.copy()
            p_h[where] = bad
            refused(r, INVALID, "a position of vertex %d is not finite" % where[0], 0, 0, 4, torch.from_numpy(p_h).cuda(), None, host=(p_h, None))
    # a tensor too short for the count: an allocation of its own, 4 bytes short of four vertices
    with open("/proc/self/maps") as f:   # the HIP runtime this process already runs on, not a second copy of it
        hip = C.CDLL(next(line.split()[-1] for line in f if "libamdhip64" in line))
    short = C.c_void_p()
    assert hip.hipMalloc(C.byref(short), C.c_size_t(44)) == 0
    try:
        refused(r, INVALID, "allocation ends", 0, 0, 4, short.value, None)
        refused(r, INVALID, "allocation ends", 0, 0, 3, short.value + 12, None)
        out = r.lib.gbl_get_vertices_device(r.handle, 0, 0, 4, short.value)
        assert out == INVALID and "allocation ends" in r.lib.gbl_last_error(r.handle).decode()
    finally:
        assert hip.hipFree(short) == 0
    # a tensor on the CPU handed straight to the C entry point.  What this pins: the pointer check comes ahead of every access
    # to the memory -- a kernel or a copy reading a host address as a device one is a fault, not a status
    refused(r, INVALID, "not device memory", 0, 0, 4, good_h, None)
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        r.update_vertices(0, torch.zeros((4, 3)))                                          # the CPU
    with pytest.raises(ValueError):
        r.update_vertices(0, torch.zeros((4, 3), dtype=torch.float64, device="cuda:0"))   # the dtype
    with pytest.raises(ValueError):
        r.update_vertices(0, torch.zeros((4, 6), dtype=torch.float32, device="cuda:0")[:, ::2])   # the layout
    with pytest.raises(ValueError):
        r.update_vertices(0, good, normals=good_h)
    base_tables = all_tables(r)
    for t in ALL_TABLES:
        assert base_tables[t].tobytes() == t_before[t].tobytes(), t
    assert torch.equal(li_of(r), before) and np.array_equal(r.vertices(0)[:4], mesh_positions(r.scene)[0][:4])
    assert np.array_equal(r.vertices(0, device=True).cpu().numpy(), mesh_positions(r.scene)[0])
    # normals only: bunny_vn.obj has vertex normals
    with open(os.path.join(gs.SCENE_DIR, "bunny.json")) as f:
        doc = json.load(f)
    gs._merge(doc, ov)
    doc["geometries"][0]["file"] = "models/bunny_vn.obj"
    r = tracer(load(doc, gs.SCENE_DIR))
    assert r.scene.desc.meshes[0].has_normal
    t_before = all_tables(r)
    for where in ((0, 0), (3, 2)):
        for bad in (np.nan, np.inf, -np.inf):
            n_h = good_h.copy()
            n_h[where] = bad
            refused(r, INVALID, "a normal of vertex %d is not finite" % (2 + where[0]), 0, 2, 4, good, torch.from_numpy(n_h).cuda(), host=(good_h, n_h))
    p_h, n_h = good_h.copy(), good_h.copy()
    p_h[2, 1], n_h[2, 1], n_h[1, 0] = np.nan, np.nan, np.inf   # the lowest float decides, a position before a normal at the same float
    refused(r, INVALID, "a normal of vertex 1 is not finite", 0, 0, 4, torch.from_numpy(p_h).cuda(), torch.from_numpy(n_h).cuda(), host=(p_h, n_h))
    refused(r, INVALID, "d_normals is not device memory", 0, 0, 4, good, good_h)   # (the CPU again, as the normals)
    n_h[1, 0] = 0.0
    refused(r, INVALID, "a position of vertex 2 is not finite", 0, 0, 4, torch.from_numpy(p_h).cuda(), torch.from_numpy(n_h).cuda(), host=(p_h, n_h))
    after = all_tables(r)
    for t in ALL_TABLES:
        assert after[t].tobytes() == t_before[t].tobytes(), t
    # cornell.json: mesh 0 is the quad its area light emits from
    r = tracer(gs.load_scene("cornell", ov))
    before = li_of(r)
    refused(r, UNSUPPORTED, "area light", 0, 0, 4, good, None, host=(good_h, None))
    assert torch.equal(li_of(r), before)
    # ibl.json: an image based light is sized by the scene bound; its sphere and its disk have no vertices
    r = tracer(gs.load_scene("ibl", ov))
    m = next(i for i in range(r.scene.desc.num_meshes) if r.scene.desc.meshes[i].shape == 0)
    refused(r, UNSUPPORTED, "scene bound", m, 0, 1, good, None, host=(good_h, None))
    for i in range(r.scene.desc.num_meshes):
        if r.scene.desc.meshes[i].shape != 0:
            refused(r, INVALID, "sphere or a disk", i, 0, 1, good, None, host=(good_h, None))
    with pytest.raises(_abi.GoblinError) as e:
        r.update_vertices(m, good[:1])
    assert e.value.status == UNSUPPORTED
    # a directional light
    doc = meshes.scene_doc("few5")
    doc["lights"].append({"name": "sun", "type": "directional", "radiance": [1, 1, 1], "direction": [0, -1, 0]})
    r = tracer(load(doc, dirs["a"]))
    t_before = all_tables(r)
    refused(r, UNSUPPORTED, "directional", 1, 0, 4, good, None, host=(good_h, None))
    after = all_tables(r)
    for t in ALL_TABLES:
        assert after[t].tobytes() == t_before[t].tobytes(), t
