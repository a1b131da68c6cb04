"""TEST INFRASTRUCTURE: the contract of gbl_render_motion_deform (include/goblin_hip.h) in numpy, in the kernel's
operation order, on top of tests/motion_reference.py.

``deform_planes`` evaluates the two planes from the hit distance and instance of every pixel's centre ray, as ``motion_planes``
does, and follows a hit of a deformed mesh through the triangle's previous pose.  The records do not name the triangle, so it is
found by brute force in float64 -- the triangle of the instance's mesh the object-space ray meets at the record's ``t`` -- and the
barycentrics are then taken by the device's own Moeller-Trumbore (kernels/trace.h tri_test_regs) in precision ``T``.  The tests
deform meshes continuously across shared edges (vertices move as a function of their position, so vertices that coincide stay
together), so which of two triangles is chosen at an edge does not matter.

``barycentric_uncertainty`` is a first-order running error bound of those float32 barycentrics, operation by operation;
``deform_planes(..., nudge=(db1, db2))`` evaluates the planes at displaced barycentrics, which gives the restatement's own
sensitivity to them by a difference.  ``normal_rule`` is the normal's carry alone.

``deforming_sequence`` is the analytic pair of frames the tests accumulate, in ``moving_sequence``'s manner.
"""
import functools

import numpy as np

import motion_reference as mr
from denoise_reference import lum
from motion_reference import F, compose, project, xf_normal, xf_point
from temporal_reference import SEQUENCE_PARAMS, camera, camera_ray, pack_camera, prepare

EPS32 = float(np.finfo(np.float32).eps) / 2.0      # unit roundoff


def xf_vector(m, v):
    """kernels/vecmath.h xf_vector."""
    return tuple((m[k, 0] * v[0] + m[k, 1] * v[1]) + m[k, 2] * v[2] for k in range(3))


def cross(a, b):
    """kernels/vecmath.h cross."""
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def length(a):
    return np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])


def edges(V, faces):
    """(p0, e1, e2), three (m, 3) float32 arrays: DevTri's fields, the edges being float32 differences."""
    V = np.asarray(V, F)
    p0, p1, p2 = V[faces[:, 0]], V[faces[:, 1]], V[faces[:, 2]]
    return p0, (p1 - p0).astype(F), (p2 - p0).astype(F)


def deformed_meshes(meshes):
    """The meshes of {mesh: (current positions, previous positions, faces)} whose previous positions differ bitwise."""
    return {m: v for m, v in (meshes or {}).items() if np.asarray(v[0], F).tobytes() != np.asarray(v[1], F).tobytes()}


def find_triangles(o, d, t, p0, e1, e2):
    """Per ray (n of them; o, d: tuples of three float64 arrays) the triangle it meets at ``t``, by brute force in float64: the
    one whose own hit distance lies closest to ``t`` among those the ray meets inside the triangle.  (index, |t - t_tri|)."""
    n = len(t)
    if n > 256:          # in blocks of rays: the (rays, triangles, 3) temporaries stay small
        parts = [find_triangles(tuple(c[k:k + 256] for c in o), tuple(c[k:k + 256] for c in d), t[k:k + 256], p0, e1, e2) for k in range(0, n, 256)]
        return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    O = np.stack(o, -1)[:, None, :]
    D = np.stack(d, -1)[:, None, :]
    P0, E1, E2 = (a.astype(np.float64)[None] for a in (p0, e1, e2))
    with np.errstate(all="ignore"):
        s1 = np.cross(D, E2)
        div = (s1 * E1).sum(-1)
        s = O - P0
        b1 = (s * s1).sum(-1) / div
        s2 = np.cross(s, E1)
        b2 = (D * s2).sum(-1) / div
        tt = (E2 * s2).sum(-1) / div
        slack = 1e-6
        inside = (div != 0) & (b1 >= -slack) & (b2 >= -slack) & (b1 + b2 <= 1 + slack)
        miss = np.where(inside, np.abs(tt - t[:, None]), np.inf)
    idx = miss.argmin(1)
    return idx, miss[np.arange(len(idx)), idx]


def barycentrics(o, d, p0, e1, e2, T):
    """tri_test_regs: (b1, b2) of rays (o, d) on their triangles (p0, e1, e2: tuples of arrays), in ``T``."""
    one = T(1.0)
    s1 = cross(d, e2)
    inv = one / dot(s1, e1)
    s = tuple(o[k] - p0[k] for k in range(3))
    b1 = dot(s, s1) * inv
    s2 = cross(s, e1)
    b2 = dot(d, s2) * inv
    return b1, b2


def barycentric_uncertainty(inv_m, o_w, d_w, p0, e1, e2):
    """A first-order bound of the rounding error of the float32 ``barycentrics`` of object-space rays made from world rays by
    xf_point / xf_vector(inv_m): every operation contributes its result's magnitude times the unit roundoff, and carries the
    bounds of its operands (float64 throughout).  (eb1, eb2)."""
    u = EPS32
    A = np.abs(inv_m.astype(np.float64))
    ow, dw = [np.abs(c) for c in o_w], [np.abs(c) for c in d_w]
    o = xf_point(inv_m.astype(np.float64), o_w)
    d = xf_vector(inv_m.astype(np.float64), d_w)
    eo = tuple(3 * u * (A[k, 0] * ow[0] + A[k, 1] * ow[1] + A[k, 2] * ow[2] + A[k, 3]) for k in range(3))
    ed = tuple(3 * u * (A[k, 0] * dw[0] + A[k, 1] * dw[1] + A[k, 2] * dw[2]) for k in range(3))
    ab = lambda v: tuple(np.abs(c) for c in v)                                    # noqa: E731
    adot = lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2]                   # noqa: E731
    acr = lambda a, b: (a[1] * b[2] + a[2] * b[1], a[2] * b[0] + a[0] * b[2], a[0] * b[1] + a[1] * b[0])   # noqa: E731
    s = tuple(o[k] - p0[k] for k in range(3))
    es = tuple(eo[k] + u * np.abs(s[k]) for k in range(3))
    s1 = cross(d, e2)
    es1 = tuple(2 * u * a + b for a, b in zip(acr(ab(d), ab(e2)), acr(ed, ab(e2))))
    div = dot(s1, e1)
    ediv = 3 * u * adot(ab(s1), ab(e1)) + adot(es1, ab(e1))
    num1 = dot(s, s1)
    en1 = 3 * u * adot(ab(s), ab(s1)) + adot(es, ab(s1)) + adot(ab(s), es1)
    s2 = cross(s, e1)
    es2 = tuple(2 * u * a + b for a, b in zip(acr(ab(s), ab(e1)), acr(es, ab(e1))))
    num2 = dot(d, s2)
    en2 = 3 * u * adot(ab(d), ab(s2)) + adot(ed, ab(s2)) + adot(ab(d), es2)
    with np.errstate(all="ignore"):
        b1, b2 = num1 / div, num2 / div
        eb1 = (en1 + np.abs(b1) * ediv) / np.abs(div) + 2 * u * np.abs(b1)
        eb2 = (en2 + np.abs(b2) * ediv) / np.abs(div) + 2 * u * np.abs(b2)
    return eb1, eb2


def normal_rule(u, e1, e2, e1p, e2p, T=F):
    """The covector ``u`` (object space, current pose) carried to the previous pose by the inverse transpose of the map that takes
    (e1, e2, g^) to (e1', e2', g^'): tuples of arrays in ``T``.  ``u`` itself where either triangle has no area."""
    with np.errstate(all="ignore"):
        g, gp = cross(e1, e2), cross(e1p, e2p)
        L, Lp = length(g), length(gp)
        gh = tuple(c / L for c in g)
        ghp = tuple(c / Lp for c in gp)
        c1, c2, c3 = dot(e1, u), dot(e2, u), dot(gh, u)
        a, b = cross(e2p, ghp), cross(ghp, e1p)
        x = tuple((a[k] * (c1 / Lp) + b[k] * (c2 / Lp)) + ghp[k] * c3 for k in range(3))
        area = (L > 0) & (Lp > 0)
    return tuple(np.where(area, x[k], u[k]).astype(T) for k in range(3))


def deform_planes(t, inst, cur_camera, prev_camera, cur_instances, prev_instances=None, normal=None, instance_mesh=None, meshes=None, T=F,
                  nudge=None, info=None, found=None):
    """gbl_render_motion_deform's planes (2, H, W, 4) in ``T``: ``motion_planes`` with ``instance_mesh`` (the mesh of every
    instance) and ``meshes`` {mesh: (current positions, previous positions, faces)}.  ``nudge`` = (db1, db2), (H, W) arrays added
    to the barycentrics; ``info``: a dict that receives ``on`` (pixels on a deformed mesh), ``tri``, ``t_miss`` (how far the
    chosen triangle's own hit distance lies from the record's), ``b1`` / ``b2`` and their ``eb1`` / ``eb2``; ``found``: a dict that
    keeps the triangle search per instance between calls over the same records and current pose."""
    deformed = deformed_meshes(meshes)
    t = np.asarray(t, F).astype(T)
    inst = np.asarray(inst)
    H, W = inst.shape
    hit = inst >= 0
    zero = T(0.0)
    moved = mr.moved_instances(cur_instances, prev_instances)
    rec = {k: np.zeros((H, W)) for k in ("b1", "b2", "eb1", "eb2", "t_miss")}
    rec["on"], rec["tri"] = np.zeros((H, W), bool), np.full((H, W), -1)
    with np.errstate(all="ignore"):
        ys, xs = np.mgrid[0:H, 0:W]
        cam = pack_camera(cur_camera, W, H)
        o, d = camera_ray(cam, xs.astype(F).astype(T) + T(0.5), ys.astype(F).astype(T) + T(0.5), T)
        o64, d64 = camera_ray(cam, xs + 0.5, ys + 0.5, np.float64)
        P = tuple(o[k] + d[k] * t for k in range(3))
        n = np.zeros((H, W, 3), T)
        if normal is not None:
            ones = np.ones((H, W, 4), F)
            n = prepare(ones, None, normal, ones)["n"].astype(T)
        nn = tuple(n[..., k] for k in range(3))
        nb = nn
        for i in sorted(set(moved) | {i for i in range(len(cur_instances)) if instance_mesh is not None and instance_mesh[i] in deformed}):
            sel = inst == i
            if not sel.any():
                continue
            m_cur, inv_cur = compose(cur_instances[i], T)
            m_prev, inv_prev = compose(prev_instances[i], T) if i in moved else (m_cur, inv_cur)
            if instance_mesh is not None and instance_mesh[i] in deformed:
                V, Vp, faces = deformed[instance_mesh[i]]
                p0, e1, e2 = edges(V, faces)
                q0, f1, f2 = edges(Vp, faces)
                inv64 = compose(cur_instances[i], np.float64)[1]
                oo = xf_point(inv64, tuple(c[sel] for c in o64))
                dd = xf_vector(inv64, tuple(c[sel] for c in d64))
                if found is None or i not in found:
                    hold = (found if found is not None else {})
                    hold[i] = find_triangles(oo, dd, t[sel].astype(np.float64), p0, e1, e2)
                    tri, miss = hold[i]
                else:
                    tri, miss = found[i]
                col = lambda a: tuple(a[tri, k].astype(T) for k in range(3))       # noqa: E731
                ot = xf_point(inv_cur, tuple(c[sel] for c in o))
                dt = xf_vector(inv_cur, tuple(c[sel] for c in d))
                b1, b2 = barycentrics(ot, dt, col(p0), col(e1), col(e2), T)
                eb1, eb2 = barycentric_uncertainty(inv64, tuple(c[sel] for c in o64), tuple(c[sel] for c in d64),
                                                   *(tuple(a[tri, k].astype(np.float64) for k in range(3)) for a in (p0, e1, e2)))
                for key, val in (("b1", b1), ("b2", b2), ("eb1", eb1), ("eb2", eb2), ("t_miss", miss), ("tri", tri), ("on", True)):
                    rec[key][sel] = val
                if nudge is not None:
                    b1, b2 = b1 + nudge[0][sel].astype(T), b2 + nudge[1][sel].astype(T)
                v0, e1p, e2p = col(q0), col(f1), col(f2)
                Q = tuple((v0[k] + e1p[k] * b1) + e2p[k] * b2 for k in range(3))
                Pm = xf_point(m_prev, Q)
                P = tuple(_put(P[k], sel, Pm[k]) for k in range(3))
                if normal is not None:
                    u = xf_normal(m_cur, tuple(c[sel] for c in nn))
                    x = normal_rule(u, col(e1), col(e2), e1p, e2p, T)
                    w = xf_normal(inv_prev, x)
                    ln = length(w)
                    nb = tuple(_put(nb[k], sel, np.where(ln > 0, w[k] / ln, zero)) for k in range(3))
            else:               # motion_planes' moved instance
                Pm = xf_point(m_prev, xf_point(inv_cur, P))
                P = tuple(np.where(sel, Pm[k], P[k]) for k in range(3))
                if normal is not None:
                    u = xf_normal(inv_prev, xf_normal(m_cur, nn))
                    ln = length(u)
                    nb = tuple(np.where(sel, np.where(ln > 0, u[k] / ln, zero), nb[k]) for k in range(3))
        pr = project(P, prev_camera, W, H, T)
        ok = hit & pr["front"] & np.isfinite(pr["image_x"]) & np.isfinite(pr["image_y"]) & np.isfinite(pr["z_exp"])
        out = np.zeros((2, H, W, 4), T)
        for k, plane in enumerate((pr["image_x"], pr["image_y"], pr["z_exp"], np.ones((H, W), T))):
            out[0, ..., k] = np.where(ok, plane, zero)
        for k in range(3):
            out[1, ..., k] = nb[k]
        out[1, ..., 3] = np.where(hit, (inst + 1).astype(F).astype(T), zero)
    if info is not None:
        info.update(rec)
    return out


def _put(plane, sel, values):
    out = np.array(plane, copy=True)
    out[sel] = values
    return out


# ---- the fixture -------------------------------------------------------------------------------------------------------
SHEET_HALF = (1.5, 1.0)
SHEET_FACES = np.array([[0, 1, 2], [0, 2, 3]], np.int64)
SHEAR = mr.SHIFT            # the far (upper) edge's travel per frame: half a stripe period


def sheet_vertices(shear):
    """The sheet in object space: a rectangle in z = 0 whose upper edge is pushed by ``shear`` along x, float32."""
    hx, hy = SHEET_HALF
    return np.array([[-hx, -hy, 0.0], [hx, -hy, 0.0], [hx + shear, hy, 0.0], [-hx + shear, hy, 0.0]], F)


def _frame(cam, width, height, sheet_x, V):
    """Per pixel centre, in float64: hit distance, instance (0 wall, 1 sheet, -1 nothing) and colour.  The stripes are fixed in
    the sheet's own parametrisation: they are a function of the unsheared x."""
    c = pack_camera(cam, width, height)
    ys, xs = np.mgrid[0:height, 0:width]
    o, d = camera_ray(c, xs + 0.5, ys + 0.5, np.float64)
    t_sh, t_wall = (mr.SQUARE_Z - o[2]) / d[2], (mr.WALL_Z - o[2]) / d[2]
    P_sh = tuple(o[k] + t_sh * d[k] for k in range(3))
    P_wall = tuple(o[k] + t_wall * d[k] for k in range(3))
    hx, hy = SHEET_HALF
    shear = float(V[3, 0]) - float(V[0, 0])
    u = (P_sh[0] - sheet_x) - shear * (P_sh[1] + hy) / (2.0 * hy)
    on_sh = (np.abs(u) < hx) & (np.abs(P_sh[1]) < hy)
    on_wall = ~on_sh & (P_wall[0] < mr.WALL_X_MAX)
    inst = np.where(on_sh, 1, np.where(on_wall, 0, -1)).astype(np.int32)
    t = np.where(on_sh, t_sh, np.where(on_wall, t_wall, 0.0))
    colour = np.where(on_sh[..., None], mr._stripes(u), np.where(on_wall[..., None], mr._wall(P_wall), 0.1))
    return t.astype(F), inst, colour.astype(F)


@functools.lru_cache(maxsize=None)
def deforming_sequence(width=37, height=23, shear=SHEAR, seed=20261021):
    """Two analytic frames under one still camera at the origin looking down +z: a striped sheet of two triangles (instance 1,
    mesh 1) in front of a wall (instance 0, mesh 0), neither instance moving.  The sheet's upper edge travels by ``shear`` along x
    between the frames, so the stripes travel with the surface while its depth and normal stay what they were.

    As ``moving_sequence``: the current frame's film / normal / depth / variance, ``history`` of the previous frame, cameras,
    ``instances``, ``t`` / ``inst`` / ``prev_inst``, ``analytic`` / ``prev_analytic``, ``params``; and ``instance_mesh``,
    ``meshes`` {1: (current, previous, faces)}, ``motion_static`` -- ``motion_planes``' planes, the sheet treated as static --
    and ``motion``, ``deform_planes``' for the pair."""
    rng = np.random.default_rng(seed)
    H, W = height, width
    cam = camera()
    instances = (mr.IDENTITY, ((-0.25, 0.0, mr.SQUARE_Z), mr.IDENTITY[1], mr.IDENTITY[2]))
    V_prev, V_cur = sheet_vertices(0.0), sheet_vertices(shear)
    nrm = np.broadcast_to(np.array([0.0, 0.0, -1.0], F), (H, W, 3))

    def films(t, inst, colour, w):
        cov = (inst >= 0).astype(F)
        film = np.concatenate([colour * w[..., None], w[..., None]], -1).astype(F)
        normal = np.concatenate([nrm * (cov * w)[..., None], w[..., None]], -1).astype(F)
        depth = np.stack([t * cov * w, cov * w, np.zeros((H, W), F), w], -1).astype(F)
        return film, normal, depth
    t0, inst0, colour0 = _frame(cam, W, H, instances[1][0][0], V_prev)
    t1, inst1, colour1 = _frame(cam, W, H, instances[1][0][0], V_cur)
    w = np.exp2(rng.integers(-1, 3, (H, W))).astype(F)
    film, normal, depth = films(t1, inst1, colour1, w)
    variance = rng.uniform(0.0, 0.1, (H, W)).astype(F)
    max_history = SEQUENCE_PARAMS["max_history"]
    N = rng.uniform(1.0, max_history, (H, W)).astype(F)
    N[rng.uniform(0.0, 1.0, (H, W)) < 0.06] = 0.0        # holes
    hl = lum(colour0[..., 0], colour0[..., 1], colour0[..., 2])
    history = np.zeros((3, H, W, 4), F)
    history[0] = np.concatenate([colour0, N[..., None]], -1)
    history[1] = np.stack([hl, hl * hl + rng.uniform(0.0, 0.02, (H, W)).astype(F), rng.uniform(0.0, 0.02, (H, W)).astype(F), t0], -1)
    history[2] = np.concatenate([nrm * (inst0 >= 0)[..., None], (inst0 >= 0).astype(F)[..., None]], -1)
    history[:, N == 0] = 0.0
    instance_mesh = (0, 1)
    meshes = {1: (V_cur, V_prev, SHEET_FACES)}
    motion_static = mr.motion_planes(t1, inst1, cam, cam, instances, instances, normal)
    motion = deform_planes(t1, inst1, cam, cam, instances, instances, normal, instance_mesh, meshes)
    out = dict(film=film, normal=normal, depth=depth, variance=variance, history=history, cur_camera=cam, prev_camera=cam, instances=instances,
               t=t1, inst=inst1, prev_t=t0, prev_inst=inst0, analytic=colour1, prev_analytic=colour0, instance_mesh=instance_mesh, meshes=meshes,
               motion_static=motion_static, motion=motion, params=dict(SEQUENCE_PARAMS))
    for arr in out.values():
        if isinstance(arr, np.ndarray):
            arr.setflags(write=False)
    return out
