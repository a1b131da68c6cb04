"""TEST INFRASTRUCTURE for gbl_trace_rays (tests/test_query_cpu.py, tests/test_gpu_query.py): the ray populations, the scene's
triangles in world space in float64, a float64 brute force over them, and the per-ray tolerance both tests use.

Rays are (n, 8) float32 rows {o, mint, d, maxt}: gbl_ray's layout.

The scene bound of the populations is the union of the instances' world boxes WITHOUT the stage floor of tests/meshes.py's
documents (instance 0, a quad 200 reaches wide: a bound that holds it is empty but for two triangles); a scene that brings
its own floor (the bundled `shapes`) keeps it.

The tolerance is float32 epsilon x scene extent x a stated factor, one constant for every ray:

    tol = FACTOR * eps32 * extent,    FACTOR = 64

extent is the largest coordinate magnitude among the scene bound, the ray's origin, the hit point and the hit triangle's three
vertices (the triangle test's operands: s = o - p0 is formed from them, and the stage floor's corners lie 200 reaches out).
FACTOR: Moller-Trumbore makes about twenty roundings on operands of that size, taking the ray into the instance's space with
an inverse composed in float32 about ten more; doubled.  It is a bound on a DISTANCE in world units; a bound on t divides it
by |d|.
"""
import numpy as np

import motion_reference as mr

F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)
FACTOR = 64.0
EDGE_BARY, EDGE_COS, EDGE_CAP = 1e-4, 1e-4, 0.05   # the brute-force comparison's excluded "edge rays" and their cap
N_RAYS = 2000
COUNTS = (1, 63, 64, 65, 257, 2000)


# ---------------------------------------------------------------------------
# the scene in world space, float64
# ---------------------------------------------------------------------------
def instance_transforms(scene):
    d = scene.desc
    return [(tuple(d.instances[i].to_world.position), tuple(d.instances[i].to_world.orientation), tuple(d.instances[i].to_world.scale))
            for i in range(d.num_instances)]


def mesh_arrays(scene):
    """Per mesh of the description: (positions float64 [V, 3], faces [T, 3]) or None for a sphere or a disk."""
    d = scene.desc
    P = np.ctypeslib.as_array(d.positions, shape=(d.num_vertices * 3,)).reshape(-1, 3)
    I = np.ctypeslib.as_array(d.indices, shape=(max(1, d.num_triangles) * 3,)).reshape(-1, 3)
    out = []
    for m in range(d.num_meshes):
        gm = d.meshes[m]
        if gm.shape != 0:
            out.append(None)
        else:
            out.append((P[gm.vertex_offset:gm.vertex_offset + gm.vertex_count].astype(np.float64),
                        I[gm.tri_offset:gm.tri_offset + gm.tri_count].astype(np.int64)))
    return out


def world_triangles(scene, transforms=None, positions=None):
    """dict(tri [N, 3, 3] float64 world vertices, inst [N], prim [N]) over every instanced triangle; `transforms` replaces the
    description's, `positions` (per mesh, or None entries) its vertex arrays."""
    d = scene.desc
    trs = transforms if transforms is not None else instance_transforms(scene)
    ms = mesh_arrays(scene)
    tri, inst, prim = [], [], []
    for i in range(d.num_instances):
        m = d.instances[i].mesh
        if ms[m] is None:
            continue
        V, Fc = ms[m]
        if positions is not None and positions[m] is not None:
            V = np.asarray(positions[m], np.float64)
        M, _ = mr.compose(trs[i])
        W = V @ M[:, :3].T + M[:, 3]
        tri.append(W[Fc])
        inst.append(np.full(len(Fc), i))
        prim.append(np.arange(len(Fc)))
    return {"tri": np.concatenate(tri), "inst": np.concatenate(inst), "prim": np.concatenate(prim)}


def scene_bound(scene, skip_floor=True):
    """(lo, hi) float64 of the instances' world boxes; a sphere's or a disk's object box is its radius around the origin."""
    d = scene.desc
    ms = mesh_arrays(scene)
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for i, trs in enumerate(instance_transforms(scene)):
        if skip_floor and i == 0:
            continue
        gm = d.meshes[d.instances[i].mesh]
        if gm.shape == 0:
            V = ms[d.instances[i].mesh][0]
            blo, bhi = V.min(axis=0), V.max(axis=0)
        else:
            r = float(gm.radius)
            blo, bhi = np.array([-r, -r, -r if gm.shape == 1 else 0.0]), np.array([r, r, r if gm.shape == 1 else 0.0])
        M, _ = mr.compose(trs)
        corners = np.array([[(blo, bhi)[(c >> a) & 1][a] for a in range(3)] for c in range(8)])
        W = corners @ M[:, :3].T + M[:, 3]
        lo, hi = np.minimum(lo, W.min(axis=0)), np.maximum(hi, W.max(axis=0))
    return lo, hi


# ---------------------------------------------------------------------------
# populations
# ---------------------------------------------------------------------------
def camera_rays(oracle, width=24, height=16):
    """(A) the camera's rays through the pixel centres of a width x height frame (Oracle.camera_ray's {o, d, mint, maxt})."""
    d = oracle.scene.desc
    sx, sy = d.film.xres / float(width), d.film.yres / float(height)
    out = np.zeros((width * height, 8), F32)
    for y in range(height):
        for x in range(width):
            r = oracle.camera_ray((x + 0.5) * sx, (y + 0.5) * sy)
            out[y * width + x] = [r[0], r[1], r[2], r[6], r[3], r[4], r[5], r[7]]
    return out


def sphere_rays(bound, n=N_RAYS, seed=7001):
    """(B) from a sphere of twice the bound's radius around its centre, aimed at uniform points of the bound; unnormalised
    directions (the whole segment origin -> point, so t = 1 is the point), maxt = +inf."""
    rng = np.random.default_rng(seed)
    lo, hi = bound
    c, radius = 0.5 * (lo + hi), 0.5 * float(np.linalg.norm(hi - lo))
    v = rng.normal(size=(n, 3))
    o = c + 2.0 * radius * v / np.linalg.norm(v, axis=1, keepdims=True)
    p = lo + rng.uniform(size=(n, 3)) * (hi - lo)
    out = np.zeros((n, 8), F32)
    out[:, 0:3], out[:, 3], out[:, 4:7], out[:, 7] = o, 1e-3, p - o, np.inf
    return out


def chord_rays(bound, n=N_RAYS, seed=7002):
    """(C) chords o = p, d = q - p, mint = 1e-3, maxt = 1 with p, q uniform in the bound: "does q see p"."""
    rng = np.random.default_rng(seed)
    lo, hi = bound
    p = lo + rng.uniform(size=(n, 3)) * (hi - lo)
    q = lo + rng.uniform(size=(n, 3)) * (hi - lo)
    out = np.zeros((n, 8), F32)
    out[:, 0:3], out[:, 3], out[:, 4:7], out[:, 7] = p, 1e-3, q - p, 1.0
    return out


INVALID_RAYS = np.array([
    [np.nan, 0, 0, 1e-3, 0, 0, 1, 10], [0, np.nan, 0, 1e-3, 0, 0, 1, 10], [0, 0, np.nan, 1e-3, 0, 0, 1, 10],
    [0, 0, 0, np.nan, 0, 0, 1, 10], [0, 0, 0, 1e-3, np.nan, 0, 1, 10], [0, 0, 0, 1e-3, 0, np.nan, 1, 10],
    [0, 0, 0, 1e-3, 0, 1, np.nan, 10], [0, 0, 0, 1e-3, 0, 0, 1, np.nan],
    [np.inf, 0, 0, 1e-3, 0, 0, 1, 10], [0, -np.inf, 0, 1e-3, 0, 0, 1, 10], [0, 0, np.inf, 1e-3, 0, 0, 1, 10],
    [0, 0, 0, 1e-3, np.inf, 0, 1, 10], [0, 0, 0, 1e-3, 0, -np.inf, 0, 10], [0, 0, 0, 1e-3, 0, 1, np.inf, 10],
    [0, 0, 0, 1e-3, 0, 0, 0, 10], [0, 0, 0, 1e-3, -0.0, 0.0, -0.0, np.inf],
    [0, 0, 0, 2.0, 0, -1, 0, 1.0], [0, 0, 0, np.inf, 0, -1, 0, 10.0], [0, 0, 0, 1e-3, 0, -1, 0, -np.inf],
], F32)


def mixed_rays(valid, seed=7003):
    """(D) every row of INVALID_RAYS several times over, at seeded positions between the rows of `valid` (their origins moved
    to the valid neighbour's, so that an invalid ray that did enter traversal would find the scene).  Returns (rays, is_valid)."""
    rng = np.random.default_rng(seed)
    n = len(valid)
    reps = max(1, n // (8 * len(INVALID_RAYS)))
    where = np.sort(rng.choice(n, size=reps * len(INVALID_RAYS), replace=False))
    rays, ok = valid.copy(), np.ones(n, bool)
    for k, i in enumerate(where):
        bad = INVALID_RAYS[k % len(INVALID_RAYS)].copy()
        bad[0:3] = np.where(np.isfinite(bad[0:3]), valid[i, 0:3], bad[0:3])
        rays[i], ok[i] = bad, False
    return rays, ok


# ---------------------------------------------------------------------------
# float64 brute force: Moller-Trumbore over every world triangle
# ---------------------------------------------------------------------------
def brute_force(W, rays, chunk=256):
    """Closest hit of every ray over W["tri"] in float64, inclusive [mint, maxt], no barycentric slack: dict(hit [n] bool, t, index
    (into W), b1, b2, cos (|n.d| / |n||d| at the hit), near_edge)."""
    tri = W["tri"]
    p0, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    nrm = np.cross(e1, e2)
    n = len(rays)
    out = {k: np.zeros(n) for k in ("t", "b1", "b2", "cos")}
    out["hit"], out["index"] = np.zeros(n, bool), np.full(n, -1)
    R = rays.astype(np.float64)
    for a in range(0, n, chunk):
        o, mint, d, maxt = R[a:a + chunk, None, 0:3], R[a:a + chunk, None, 3], R[a:a + chunk, None, 4:7], R[a:a + chunk, None, 7]
        s1 = np.cross(d, e2[None])
        div = (s1 * e1[None]).sum(-1)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / div
            s = o - p0[None]
            b1 = (s * s1).sum(-1) * inv
            s2 = np.cross(s, e1[None])
            b2 = (d * s2).sum(-1) * inv
            t = (e2[None] * s2).sum(-1) * inv
            ok = (div != 0) & (b1 >= 0) & (b2 >= 0) & (b1 + b2 <= 1) & (t >= mint) & (t <= maxt)
        t = np.where(ok, t, np.inf)
        j = t.argmin(axis=1)
        r = np.arange(len(j))
        got = np.isfinite(t[r, j])
        out["hit"][a:a + chunk], out["index"][a:a + chunk] = got, np.where(got, j, -1)
        out["t"][a:a + chunk], out["b1"][a:a + chunk], out["b2"][a:a + chunk] = t[r, j], b1[r, j], b2[r, j]
        dd = R[a:a + chunk, 4:7]
        nn = nrm[j]
        with np.errstate(divide="ignore", invalid="ignore"):
            out["cos"][a:a + chunk] = np.abs((nn * dd).sum(-1)) / (np.linalg.norm(nn, axis=1) * np.linalg.norm(dd, axis=1))
    b0 = 1.0 - out["b1"] - out["b2"]
    out["near_edge"] = out["hit"] & ((np.minimum(np.minimum(out["b1"], out["b2"]), b0) < EDGE_BARY) | (out["cos"] < EDGE_COS))
    return out


def grazing(W, index, rays):
    """|n . d| / (|n| |d|) of rays against the triangles W["tri"][index] (the edge rays' second criterion)."""
    tri = W["tri"][index]
    nn = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    dd = rays[:, 4:7].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.abs((nn * dd).sum(-1)) / (np.linalg.norm(nn, axis=1) * np.linalg.norm(dd, axis=1))


def tolerance(bound, rays, t, tri):
    """The module docstring's bound, a distance in world units per ray; tri [n, 3, 3]: the world vertices of the triangle each ray hits."""
    R = rays.astype(np.float64)
    p = R[:, 0:3] + np.asarray(t, np.float64)[:, None] * R[:, 4:7]
    extent = np.maximum(np.maximum(np.abs(R[:, 0:3]).max(axis=1), np.abs(p).max(axis=1)), max(np.abs(bound[0]).max(), np.abs(bound[1]).max()))
    extent = np.maximum(extent, np.abs(np.asarray(tri, np.float64)).reshape(len(R), -1).max(axis=1))
    return FACTOR * EPS32 * extent


# the benign scene of the brute-force comparison (tests/meshes.py names); the CPU test shows the populations keep its caps
BENIGN = ["few5", "few9", "flatgrid"]
