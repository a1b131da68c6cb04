"""gbl_trace_rays on the device: batched scene queries, ray by ray.

Scenes: every mesh of tests/meshes.py in one scene, few1 alone, the 300-instance line, the bundled `shapes` (spheres and disks:
the EXT build).  Populations (tests/query_cases.py): (A) camera rays at the pixel centres of a 24 x 16 frame, (B) 2 000 rays
from a sphere of twice the scene radius aimed at uniform points of the scene bound, (C) 2 000 chords between uniform points
of the bound with maxt = 1, (D) invalid rays between valid ones.  The oracle's answers are computed once per scene.

1. exact mode (GBL_QUERY_EXACT_TIES | GBL_QUERY_SHADING_NORMAL) equals Oracle.intersect / Oracle.occluded bit for bit, and
   gbl_selftest_trace's records on the same rays (the first test of that hook);
2. lean against exact, every ray, no cap: the invariants kernels/trace.h states for the bare loop;
3. `primitive` and the barycentrics against the scene's own vertex arrays in float64, both builders and after gbl_rebuild_mesh;
4. edits are seen: host and device instance edits, a deferred vertex edit and its pending tie order;
5. the lean mode against a float64 brute force (tests/test_query_cpu.py shows the inputs keep the edge-ray cap);
6. invalid rays, the counts 1, 63, 64, 65, 257, 2 000, and a grid capped at one workgroup;
7. stream ordering;  8. every refusal.

Bounds: bit equality (1, 3 after a rebuild, 4, 6), the invariants of 2 for every ray, query_cases.tolerance -- float32 epsilon x scene
extent x 64 for every ray, derived there -- in 3 and 5.

Measured on an MI355X: the 19 tests take 3.4 s.  The new entry, the hook and the oracle agree on every one of the 4 x 4 384 rays;
lean and exact records differ on none of them; the largest distance between a hit's barycentric point and o + t d is 0.14 of the
tolerance (both builders, before and after the rebuild, which moves no lean hit to another triangle; 2 of the 2 725 hits have
|cos| < 0.01); the brute force: 15 and 0 edge rays of 2 000, largest |dt| |d| 0.16 / 0.13 of the tolerance.  The suite passes on the one-ray-per-lane measurement build of the kernel unit as well.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import meshes
import oracle_binding as ob
import query_cases as qc
import refit_reference as rr
from goblin_amd import _abi
from goblin_amd import scene as gs

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = _abi.GBL_ERR_INVALID, _abi.GBL_ERR_UNSUPPORTED
F32 = np.float32
_cases = {}


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    """Scene directories: "a" holds the meshes as generated, "jitter" the same with a jittered spiral."""
    out = {}
    for key in ("a", "jitter"):
        d = tmp_path_factory.mktemp("query_" + key)
        meshes.write_meshes(d, meshes.ALL)
        if key == "jitter":
            V, F = meshes.mesh("spiral")
            meshes.write_obj(os.path.join(str(d), "spiral.obj"), rr.jitter(V, meshes.MESHES["spiral"][1]), F)
        out[key] = str(d)
    return out


def load(doc, scene_dir):
    return gs.load_scene_text(json.dumps(doc), scene_dir)


class Case:
    """A scene with its oracle, its bound, the populations (A), (B), (C) in one array, and -- computed once -- the oracle's answer
    to every ray: intersect's (t, instance, normal) and occluded's flag."""

    def __init__(self, scene, skip_floor=True):
        self.scene, self.oracle = scene, ob.Oracle(scene)
        self.bound = qc.scene_bound(scene, skip_floor)
        self.parts = {"camera": qc.camera_rays(self.oracle), "sphere": qc.sphere_rays(self.bound), "chords": qc.chord_rays(self.bound)}
        self.rays = np.concatenate([self.parts[k] for k in ("camera", "sphere", "chords")])
        self.rays.setflags(write=False)
        self._ref = None

    def reference(self):
        if self._ref is None:
            self._ref = oracle_answers(self.oracle, self.rays)
        return self._ref


def oracle_answers(oracle, rays):
    n = len(rays)
    ref = {"t": np.full(n, -1.0, F32), "instance": np.full(n, -1, np.int32), "normal": np.zeros((n, 3), F32), "occluded": np.zeros(n, np.uint8)}
    for i, r in enumerate(rays):
        maxt = float(r[7]) if np.isfinite(r[7]) else -1.0   # (the oracle's spelling of +inf)
        h = oracle.intersect(r[0:3], r[4:7], float(r[3]), maxt)
        if h is not None:
            ref["t"][i], ref["instance"][i], ref["normal"][i] = h[0], int(h[11]), h[5:8]
        ref["occluded"][i] = oracle.occluded(r[0:3], r[4:7], float(r[3]), maxt)
    for v in ref.values():
        v.setflags(write=False)
    return ref


def case(dirs, key):
    if key not in _cases:
        if key == "all":
            _cases[key] = Case(load(meshes.scene_doc(meshes.ALL), dirs["a"]))
        elif key == "few1":
            _cases[key] = Case(load(meshes.scene_doc("few1"), dirs["a"]))
        elif key == "line":
            _cases[key] = Case(load(meshes.instances_doc(300), dirs["a"]))
        elif key == "shapes":
            _cases[key] = Case(gs.load_scene("shapes"), skip_floor=False)
        elif key == "benign":
            _cases[key] = Case(load(meshes.scene_doc(qc.BENIGN), dirs["a"]))
    return _cases[key]


SCENES = ("all", "few1", "line", "shapes")


def tracer(scene, bvh="host"):
    from goblin_amd.renderer import HipPathTracer
    return HipPathTracer(scene, 0, bvh=bvh)


def dev(torch, a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to("cuda:0")   # (a copy: the shared arrays are read-only)


def closest(torch, r, rays, **kw):
    """The (n, 8) records of a closest-hit query as a numpy structured view, after a synchronise."""
    out = r.trace(rays, **kw)["records"]
    torch.cuda.synchronize()
    return records(out.cpu().numpy())


REC = np.dtype([("t", "<f4"), ("b1", "<f4"), ("b2", "<f4"), ("instance", "<i4"), ("primitive", "<u4"), ("n", "<f4", 3)])


def records(a):
    return np.ascontiguousarray(a, F32).view(REC).reshape(-1)


def occluded(torch, r, rays, **kw):
    out = r.trace(rays, kind="any", **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def hook(torch, r, rays, kind):
    """gbl_selftest_trace on the same rays: (n, 8) float32 {t or -1 | occluded, instance or -1, normal(3), tangent(3)}."""
    rec = np.zeros((len(rays), 9), F32)
    rec[:, 0], rec[:, 1:4], rec[:, 4:7], rec[:, 7], rec[:, 8] = kind, rays[:, 0:3], rays[:, 4:7], rays[:, 3], rays[:, 7]
    d_rec = dev(torch, rec)
    out = torch.zeros((len(rays), 8), dtype=torch.float32, device="cuda:0")
    st = r.lib.gbl_selftest_trace(r.handle, d_rec.data_ptr(), out.data_ptr(), len(rays))
    assert st == _abi.GBL_OK, r.lib.gbl_last_error(r.handle).decode()
    return out.cpu().numpy()


# ---------------------------------------------------------------------------
# 1. exact mode equals the oracle and the self-test hook
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("key", SCENES)
def test_exact_mode_equals_the_oracle_and_the_hook(torch, dirs, key):
    c = case(dirs, key)
    ref = c.reference()
    r = tracer(c.scene)
    rays = dev(torch, c.rays)
    got = closest(torch, r, rays, exact_ties=True, normals=True)
    occ = occluded(torch, r, rays, exact_ties=True)
    hits = ref["instance"] >= 0
    print(key, "rays", len(c.rays), "hits", int(hits.sum()), "occluded", int(ref["occluded"].sum()))
    assert hits.sum() >= len(hits) // 8
    assert np.array_equal(got["instance"], ref["instance"]), np.flatnonzero(got["instance"] != ref["instance"])[:8]
    assert np.array_equal(bits(got["t"]), bits(ref["t"])), np.flatnonzero(bits(got["t"]) != bits(ref["t"]))[:8]
    assert np.array_equal(bits(got["n"]), bits(ref["normal"])), np.flatnonzero((bits(got["n"]) != bits(ref["normal"])).any(axis=1))[:8]
    miss = ~hits
    for f in ("b1", "b2", "primitive"):
        assert not got[f][miss].any(), f
    assert np.array_equal(occ, ref["occluded"]), np.flatnonzero(occ != ref["occluded"])[:8]
    # the hook: the same records bit for bit
    hk = hook(torch, r, c.rays, 0.0)
    assert np.array_equal(bits(hk[:, 0]), bits(got["t"])) and np.array_equal(hk[:, 1].astype(np.int32), got["instance"])
    assert np.array_equal(bits(hk[:, 2:5]), bits(got["n"]))
    ha = hook(torch, r, c.rays, 1.0)
    assert np.array_equal(ha[:, 0].astype(np.uint8), occ) and (ha[:, 1] == -1.0).all()


# ---------------------------------------------------------------------------
# 2. lean against exact: trace.h's invariants, every ray
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("key", SCENES)
def test_lean_mode_against_exact_mode(torch, dirs, key):
    c = case(dirs, key)
    r = tracer(c.scene)
    rays = dev(torch, c.rays)
    lean, exact = closest(torch, r, rays), closest(torch, r, rays, exact_ties=True)
    occ_lean, occ_exact = occluded(torch, r, rays), occluded(torch, r, rays, exact_ties=True)
    hl, he = lean["instance"] >= 0, exact["instance"] >= 0
    differ = (lean.view(np.uint32).reshape(-1, 8) != exact.view(np.uint32).reshape(-1, 8)).any(axis=1)
    print(key, "rays", len(rays), "records that differ", int(differ.sum()), "hit only lean", int((hl & ~he).sum()), "occluded only lean",
          int((occ_lean > occ_exact).sum()))
    assert (hl >= he).all(), np.flatnonzero(he & ~hl)[:8]
    both = hl & he
    assert (lean["t"][both] <= exact["t"][both]).all(), np.flatnonzero(both & (lean["t"] > exact["t"]))[:8]
    same = both & (bits(lean["t"]) == bits(exact["t"])) & (lean["instance"] == exact["instance"]) & (lean["primitive"] == exact["primitive"])
    assert np.array_equal(bits(lean["b1"])[same], bits(exact["b1"])[same]) and np.array_equal(bits(lean["b2"])[same], bits(exact["b2"])[same])
    assert (occ_lean >= occ_exact).all(), np.flatnonzero(occ_lean < occ_exact)[:8]
    assert not lean["n"].any() and not exact["n"].any()   # no flag, no normal


# ---------------------------------------------------------------------------
# 3. primitive and barycentrics
# ---------------------------------------------------------------------------
def assert_hits_lie_on_their_triangles(c, W, got, what):
    """The point v0 + b1 (v1 - v0) + b2 (v2 - v0) of triangle `primitive` of the hit instance's mesh, in world space and float64,
    within query_cases.tolerance of o + t d; and b1, b2, 1 - b1 - b2 >= -tol_b, where tol_b is that distance over the shorter of
    the triangle's two edges (a barycentric moves the point by an edge per unit) plus the triangle test's own 1e-7 slack."""
    d = c.scene.desc
    start = np.full(d.num_instances + 1, -1, np.int64)   # first row of W per instance
    first = np.flatnonzero(np.r_[True, W["inst"][1:] != W["inst"][:-1]])
    start[W["inst"][first]] = first
    hit = got["instance"] >= 0
    rays = c.rays[hit]
    g = got[hit]
    counts = np.array([d.meshes[d.instances[i].mesh].tri_count for i in g["instance"]])
    assert (g["primitive"] < counts).all(), what
    idx = start[g["instance"]] + g["primitive"]
    assert (W["inst"][idx] == g["instance"]).all() and (W["prim"][idx] == g["primitive"]).all()
    tri = W["tri"][idx]
    b1, b2 = g["b1"].astype(np.float64), g["b2"].astype(np.float64)
    p_bary = tri[:, 0] + b1[:, None] * (tri[:, 1] - tri[:, 0]) + b2[:, None] * (tri[:, 2] - tri[:, 0])
    R = rays.astype(np.float64)
    p_ray = R[:, 0:3] + g["t"].astype(np.float64)[:, None] * R[:, 4:7]
    tol = qc.tolerance(c.bound, rays, g["t"], tri)
    err = np.linalg.norm(p_bary - p_ray, axis=1)
    edge = np.minimum(np.linalg.norm(tri[:, 1] - tri[:, 0], axis=1), np.linalg.norm(tri[:, 2] - tri[:, 0], axis=1))
    assert (edge > 0).all(), what   # (a triangle with a zero edge has divisor == 0 exactly and is never accepted)
    tol_b = tol / edge + 1e-7
    lowest = np.minimum(np.minimum(b1, b2), 1.0 - b1 - b2)
    cos = qc.grazing(W, idx, rays)
    worst = int(np.argmax(err / tol))
    print(*what, "hits", int(hit.sum()), "largest error / tolerance %.3g" % float((err / tol).max()), "(its |cos| %.3g, instance %d, primitive %d)" %
          (cos[worst], g["instance"][worst], g["primitive"][worst]), "lowest barycentric / tolerance %.3g" % float((lowest / tol_b).min()),
          "hits with |cos| < 1e-2: %d" % int((cos < 1e-2).sum()))
    assert (err <= tol).all(), (what, np.flatnonzero(err > tol)[:8])
    assert (lowest >= -tol_b).all(), what


def test_primitive_and_barycentrics_for_both_builders_and_after_a_rebuild(torch, dirs):
    c = case(dirs, "all")
    W = qc.world_triangles(c.scene)
    rays = dev(torch, c.rays)
    exact = {}
    for bvh in ("host", "device"):
        r = tracer(c.scene, bvh)
        for ties in (False, True):
            got = closest(torch, r, rays, exact_ties=ties)
            assert_hits_lie_on_their_triangles(c, W, got, (bvh, "exact" if ties else "lean"))
            if ties:
                exact[bvh] = got
        # every mesh's tree built again on the device (a host-built context's triangle table is then in a new order): the same
        # rays report the same bits in exact mode; in lean mode the same t, and the same triangle but where two are met at
        # exactly one t (there the last one tested keeps the hit, and the new tree tests them in another order)
        lean = closest(torch, r, rays)
        before = r._geometry("tris")["shade"].copy()
        for m in range(c.scene.desc.num_meshes):
            r.rebuild_mesh(m)
        after = r._geometry("tris")["shade"]
        assert sorted(before) == sorted(after) and (bvh == "device" or (before != after).any())
        again = closest(torch, r, rays, exact_ties=True)
        assert again.tobytes() == exact[bvh].tobytes()
        lean_again = closest(torch, r, rays)
        assert_hits_lie_on_their_triangles(c, W, lean_again, (bvh, "rebuilt", "lean"))
        assert np.array_equal(bits(lean_again["t"]), bits(lean["t"]))
        moved = (lean_again["instance"] != lean["instance"]) | (lean_again["primitive"] != lean["primitive"])
        print(bvh, "lean hits on another triangle after the rebuild:", int(moved.sum()))
        assert not (moved & (lean["instance"] < 0)).any()
        assert lean_again[~moved].tobytes() == lean[~moved].tobytes()
    assert exact["host"].tobytes() == exact["device"].tobytes()


# ---------------------------------------------------------------------------
# 4. edits are seen
# ---------------------------------------------------------------------------
EXACT = dict(exact_ties=True, normals=True)


@pytest.mark.parametrize("device_tlas", [False, True], ids=["host_edit", "device_tlas"])
def test_instance_edits_are_seen(torch, dirs, device_tlas):
    n, moved = 300, 40
    fresh_scene = load(meshes.instances_doc(n, moved=moved), dirs["a"])
    fresh = Case(fresh_scene)
    rays = dev(torch, fresh.rays)
    want = closest(torch, tracer(fresh_scene), rays, **EXACT)
    want_occ = occluded(torch, tracer(fresh_scene), rays, exact_ties=True)
    r = tracer(case(dirs, "line").scene)
    stale = closest(torch, r, rays, **EXACT)
    T = meshes.moved_transforms(moved)
    if device_tlas:
        rows = np.array([list(p) + list(q) + list(s) for p, q, s in T], F32).reshape(-1, 10)
        r.update_instances(1, dev(torch, rows), device_tlas=True)
    else:
        r.update_instances(1, T)
    got = closest(torch, r, rays, **EXACT)
    assert stale.tobytes() != want.tobytes()   # (the edit moves what the rays see)
    assert got.tobytes() == want.tobytes(), np.flatnonzero((got.view(np.uint32).reshape(-1, 8) != want.view(np.uint32).reshape(-1, 8)).any(axis=1))[:8]
    assert np.array_equal(occluded(torch, r, rays, exact_ties=True), want_occ)


def test_a_deferred_vertex_edit_is_seen_and_its_order_waits_for_an_exact_query(torch, dirs):
    names = ["spiral", "few5"]
    scene_a, scene_b = load(meshes.scene_doc(names), dirs["a"]), load(meshes.scene_doc(names), dirs["jitter"])
    fresh = Case(scene_b)
    rays = dev(torch, fresh.rays)
    want = closest(torch, tracer(scene_b), rays, **EXACT)
    r = tracer(scene_a)
    stale = closest(torch, r, rays, **EXACT)
    spiral = 1   # (mesh 0 is the floor)
    r.update_vertices(spiral, meshes.scene_meshes(scene_b)[spiral][0], defer_order=True)
    assert r.order_pending(spiral) == 1
    lean = closest(torch, r, rays)
    assert r.order_pending(spiral) == 1   # a lean query leaves it pending
    got = closest(torch, r, rays, **EXACT)
    assert r.order_pending(spiral) == 0   # an exact one makes it
    assert stale.tobytes() != want.tobytes()
    assert got.tobytes() == want.tobytes()
    assert ((lean["instance"] >= 0) >= (got["instance"] >= 0)).all()


# ---------------------------------------------------------------------------
# 5. float64 brute force, lean mode
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("population", ["sphere", "chords"])
def test_lean_mode_against_a_float64_brute_force(torch, dirs, population):
    c = case(dirs, "benign")
    rays = c.parts[population]
    W = qc.world_triangles(c.scene)
    bf = qc.brute_force(W, rays)
    edge = bf["near_edge"]
    assert edge.sum() <= qc.EDGE_CAP * len(rays)   # a condition on the inputs (tests/test_query_cpu.py shows it holds)
    got = closest(torch, tracer(c.scene), dev(torch, rays))
    hit = got["instance"] >= 0
    print(population, "hit", int(bf["hit"].sum()), "of", len(rays), "edge rays", int(edge.sum()))
    assert np.array_equal(hit[~edge], bf["hit"][~edge]), np.flatnonzero((hit != bf["hit"]) & ~edge)[:8]
    both = hit & bf["hit"] & ~edge
    tol = qc.tolerance(c.bound, rays[both], bf["t"][both], W["tri"][bf["index"][both]])
    err = np.abs(got["t"][both].astype(np.float64) - bf["t"][both]) * np.linalg.norm(rays[both, 4:7].astype(np.float64), axis=1)
    print(population, "largest error / tolerance %.3g" % float((err / tol).max()))
    assert (err <= tol).all()
    assert np.array_equal(got["instance"][both], W["inst"][bf["index"][both]]) and np.array_equal(got["primitive"][both], W["prim"][bf["index"][both]])


# ---------------------------------------------------------------------------
# 6. invalid rays, counts, the capped grid
# ---------------------------------------------------------------------------
MODES = (dict(), EXACT)


def test_invalid_rays_are_misses_between_valid_ones(torch, dirs):
    c = case(dirs, "all")
    valid = c.parts["sphere"]
    mixed, ok = qc.mixed_rays(valid)
    assert (~ok).sum() >= len(qc.INVALID_RAYS)
    r = tracer(c.scene)
    for kw in MODES:
        want, got = closest(torch, r, dev(torch, valid), **kw), closest(torch, r, dev(torch, mixed), **kw)
        assert got[ok].tobytes() == want[ok].tobytes()
        bad = got[~ok]
        assert (bad["t"] == -1.0).all() and (bad["instance"] == -1).all()
        assert not bad["b1"].any() and not bad["b2"].any() and not bad["primitive"].any() and not bad["n"].any()
        assert (want["instance"][~ok] >= 0).sum() > 0   # (some of the replaced rays did hit)
    for ties in (False, True):
        want, got = occluded(torch, r, dev(torch, valid), exact_ties=ties), occluded(torch, r, dev(torch, mixed), exact_ties=ties)
        assert np.array_equal(got[ok], want[ok]) and not got[~ok].any()
    # every row alone, and all of them as one batch
    every = dev(torch, qc.INVALID_RAYS)
    assert (closest(torch, r, every)["instance"] == -1).all() and not occluded(torch, r, every).any()


@pytest.mark.parametrize("key", ["all", "shapes"])
def test_counts_and_a_grid_of_one_workgroup(torch, dirs, key):
    c = case(dirs, key)
    r = tracer(c.scene)
    rays = dev(torch, c.parts["sphere"])
    assert len(rays) == 2000
    for kw in MODES:
        whole = closest(torch, r, rays, **kw)
        for n in qc.COUNTS:
            part = closest(torch, r, rays[:n].contiguous(), **kw)
            assert part.tobytes() == whole[:n].tobytes(), (kw, n)
        capped = closest(torch, r, rays, _max_workgroups=1, **kw)
        assert capped.tobytes() == whole.tobytes(), kw
    for ties in (False, True):
        whole = occluded(torch, r, rays, exact_ties=ties)
        for n in qc.COUNTS:
            assert np.array_equal(occluded(torch, r, rays[:n].contiguous(), exact_ties=ties), whole[:n]), (ties, n)
        assert np.array_equal(occluded(torch, r, rays, exact_ties=ties, _max_workgroups=1), whole)
    assert r.trace(rays[:0]).get("records").shape == (0, 8) and r.trace(rays[:0], kind="any").shape == (0,)


# ---------------------------------------------------------------------------
# 7. asynchrony
# ---------------------------------------------------------------------------
def test_a_query_is_ordered_on_its_stream(torch, dirs):
    c = case(dirs, "all")
    r = tracer(c.scene)
    src = dev(torch, c.parts["sphere"])
    want = closest(torch, r, src, **EXACT)
    want_occ = occluded(torch, r, src)
    side = torch.cuda.Stream(device="cuda:0")
    rays = torch.zeros_like(src)           # all zeros: invalid rays, every answer a miss
    big = torch.ones((4096, 4096), device="cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(6):                 # work ahead of the write, so that a query on another stream would run before it
            big = big @ big * 1e-4
        rays.copy_(src)
        got = r.trace(rays, stream=side, **EXACT)["records"]
        # two calls on one stream into disjoint outputs
        out = torch.empty((2, len(src)), dtype=torch.uint8, device="cuda:0")
        r.trace(rays, kind="any", out=out[0], stream=side)
        r.trace(rays, kind="any", exact_ties=True, out=out[1], stream=side)
    side.synchronize()
    assert records(got.cpu().numpy()).tobytes() == want.tobytes()
    assert np.array_equal(out[0].cpu().numpy(), want_occ)
    assert np.array_equal(out[1].cpu().numpy(), occluded(torch, r, src, exact_ties=True))


# ---------------------------------------------------------------------------
# 8. refusals
# ---------------------------------------------------------------------------
def test_refusals(torch, dirs):
    c = case(dirs, "few1")
    r = tracer(c.scene)
    lib, h = r.lib, r.handle
    n = 64
    rays = dev(torch, c.parts["sphere"][:n])
    out = torch.full((n, 8), 7.0, dtype=torch.float32, device="cuda:0")
    CLOSEST, ANY, TIES, NORMAL = _abi.GBL_QUERY_CLOSEST, _abi.GBL_QUERY_ANY, _abi.GBL_QUERY_EXACT_TIES, _abi.GBL_QUERY_SHADING_NORMAL

    def refused(status, needle, kind, d_rays, count, d_out, flags):
        for call in (lambda: lib.gbl_trace_rays(h, kind, d_rays, count, d_out, flags, None),
                     lambda: lib.gbl_selftest_query(h, kind, d_rays, count, d_out, flags, 0)):
            assert call() == status, needle
            assert needle in lib.gbl_last_error(h).decode(), (needle, lib.gbl_last_error(h).decode())

    assert lib.gbl_trace_rays(None, CLOSEST, rays.data_ptr(), n, out.data_ptr(), 0, None) == INVALID
    assert lib.gbl_selftest_query(None, CLOSEST, rays.data_ptr(), n, out.data_ptr(), 0, 0) == INVALID
    refused(INVALID, "null pointer", CLOSEST, None, n, out.data_ptr(), 0)
    refused(INVALID, "null pointer", ANY, rays.data_ptr(), n, None, 0)
    refused(INVALID, "unknown kind", 2, rays.data_ptr(), n, out.data_ptr(), 0)
    refused(INVALID, "flags", CLOSEST, rays.data_ptr(), n, out.data_ptr(), 4)
    refused(INVALID, "flags", ANY, rays.data_ptr(), n, out.data_ptr(), 0x80000001)
    refused(INVALID, "GBL_QUERY_SHADING_NORMAL", ANY, rays.data_ptr(), n, out.data_ptr(), NORMAL)
    refused(UNSUPPORTED, "2^32", CLOSEST, rays.data_ptr(), 1 << 32, out.data_ptr(), 0)
    host_rays, host_out = np.ascontiguousarray(c.parts["sphere"][:n]), np.zeros((n, 8), F32)
    refused(INVALID, "d_rays is not device memory", CLOSEST, host_rays.ctypes.data, n, out.data_ptr(), 0)   # refused before anything reads it
    refused(INVALID, "d_out is not device memory", CLOSEST, rays.data_ptr(), n, host_out.ctypes.data, 0)
    both = torch.zeros((2 * n, 8), dtype=torch.float32, device="cuda:0")
    both[:n] = rays
    refused(INVALID, "overlaps", CLOSEST, both.data_ptr(), n, both.data_ptr() + 32 * (n - 1), 0)
    refused(INVALID, "overlaps", ANY, both.data_ptr(), n, both.data_ptr() + 32 * n - 1, 0)
    with open("/proc/self/maps") as f:   # the HIP runtime this process already runs on, not a second copy of it
        hip = C.CDLL(next(line.split()[-1] for line in f if "libamdhip64" in line))
    short = C.c_void_p()
    assert hip.hipMalloc(C.byref(short), C.c_size_t(32 * n - 4)) == 0   # 4 bytes short of n records; checked by the refusal, never launched
    try:
        refused(INVALID, "d_rays: its allocation ends", CLOSEST, short.value, n, out.data_ptr(), 0)
        refused(INVALID, "d_out: its allocation ends", CLOSEST, rays.data_ptr(), n, short.value, 0)
        many = torch.zeros((32 * n, 8), dtype=torch.float32, device="cuda:0")   # 32 n rays that are there: one byte of output each, 4 too many
        refused(INVALID, "d_out: its allocation ends", ANY, many.data_ptr(), 32 * n, short.value, 0)
        assert lib.gbl_trace_rays(h, ANY, rays.data_ptr(), n, short.value, 0, None) == _abi.GBL_OK   # ... which n rays fit
    finally:
        torch.cuda.synchronize()
        assert hip.hipFree(short) == 0
    torch.cuda.synchronize()
    assert (out == 7.0).all()   # nothing was launched
    # n == 0: GBL_OK whatever the pointers
    assert lib.gbl_trace_rays(h, CLOSEST, None, 0, None, 0, None) == _abi.GBL_OK
    assert lib.gbl_trace_rays(h, ANY, rays.data_ptr(), 0, out.data_ptr(), TIES, None) == _abi.GBL_OK
    # the Python face's own checks
    with pytest.raises(ValueError):
        r.trace(rays, kind="any", normals=True)
    with pytest.raises(ValueError):
        r.trace(rays.cpu())
    with pytest.raises(ValueError):
        r.trace(rays[:, :7])
    # the context still answers
    ref = c.reference()
    got = closest(torch, r, dev(torch, c.rays), **EXACT)
    assert np.array_equal(got["instance"], ref["instance"]) and np.array_equal(bits(got["t"]), bits(ref["t"]))
