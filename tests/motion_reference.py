"""TEST INFRASTRUCTURE: the contracts of gbl_render_motion and gbl_film_accumulate_motion (include/goblin_hip.h)
in numpy, in the kernels' operation order.

``project`` is the projection of a previous-frame point through the previous camera (kernels/temporal.h tp_project);
``motion_planes`` evaluates the two planes from the hit distance and instance of every pixel's centre ray, whoever traced it;
``accumulate_motion`` is tests/temporal_reference.py ``accumulate`` with the reprojection swapped for the planes.  With ``dtype``
float32 every add, mul, div, sqrt and floor of ``accumulate_motion`` is the kernel's, so its outputs are the device's bit for
bit.  ``compose`` builds a transform and its inverse in float64 and rounds them: the device's are composed in float32 on the host
(scene_prep.cpp), so planes of a moved instance are compared under ``bound``, never bit for bit.

``moving_sequence`` is the analytic pair of frames the tests accumulate; computed once per shape and shared read-only.
"""
import functools

import numpy as np

from denoise_reference import lum, shift
from temporal_reference import F, SEQUENCE_PARAMS, bound, camera, camera_ray, pack_camera, prepare, quat_rotate  # noqa: F401

IDENTITY = ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


def trs_words(t):
    """The ten floats of a (position, orientation, scale) transform as the ABI holds them."""
    return np.array([v for part in t for v in part], F)


def compose(trs, T=np.float64):
    """scene_prep.cpp compose: (m, inv), the 3 x 4 rows of toWorld = T R S and of its inverse, from float32 inputs, evaluated in
    float64 and rounded to T."""
    pos, q, scale = (np.array(part, F).astype(np.float64) for part in trs)
    w, x, y, z = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    m = np.eye(4)
    m[:3, :3] = R * scale[None, :]
    m[:3, 3] = pos
    return m[:3].astype(T), np.linalg.inv(m)[:3].astype(T)


def xf_point(m, p):
    """kernels/vecmath.h xf_point: rows of a 3 x 4 matrix on a point, summed left to right."""
    return tuple(((m[k, 0] * p[0] + m[k, 1] * p[1]) + m[k, 2] * p[2]) + m[k, 3] for k in range(3))


def xf_normal(m, n):
    """kernels/vecmath.h xf_normal: the transposed 3 x 3 of a 3 x 4 matrix on a vector."""
    return tuple((m[0, k] * n[0] + m[1, k] * n[1]) + m[2, k] * n[2] for k in range(3))


def project(P_prev, prev_camera, W, H, T=F):
    """tp_project: dict(image_x, image_y, z_exp, front) of the points ``P_prev`` (three arrays) under ``prev_camera``."""
    prv = pack_camera(prev_camera, W, H)
    one = T(1.0)
    with np.errstate(all="ignore"):
        w = tuple(P_prev[k] - T(prv["pos"][k]) for k in range(3))
        qp = [T(prv["q"][0]), -T(prv["q"][1]), -T(prv["q"][2]), -T(prv["q"][3])]
        v = quat_rotate(qp, w, T)
        if prv["type"] == 1:
            front = v[2] >= 0
            xndc = v[0] / (T(0.5) * T(prv["film_w"]))
            yndc = v[1] / (T(0.5) * T(prv["film_h"]))
            z_exp = v[2]
        else:
            front = v[2] > 0
            xndc = (v[0] / v[2]) * T(prv["proj00"])
            yndc = (v[1] / v[2]) * T(prv["proj11"])
            z_exp = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
        image_x = ((xndc + one) * T(0.5)) * T(F(W))
        image_y = ((one - yndc) * T(0.5)) * T(F(H))
    return dict(image_x=image_x, image_y=image_y, z_exp=z_exp, front=front)


def moved_instances(cur_instances, prev_instances):
    """Indices whose ten floats differ bitwise (gbl_render_motion's host-side comparison)."""
    if prev_instances is None:
        return []
    return [i for i, (a, b) in enumerate(zip(cur_instances, prev_instances)) if trs_words(a).tobytes() != trs_words(b).tobytes()]


def motion_planes(t, inst, cur_camera, prev_camera, cur_instances=None, prev_instances=None, normal=None, T=F):
    """gbl_render_motion's planes (2, H, W, 4) in ``T`` from the centre rays' hit distance ``t`` (H, W) and instance ``inst``
    (H, W; < 0: a miss).  ``normal``: the current frame's normal film or None."""
    t = np.asarray(t, F).astype(T)
    inst = np.asarray(inst)
    H, W = inst.shape
    hit = inst >= 0
    zero = T(0.0)
    with np.errstate(all="ignore"):
        ys, xs = np.mgrid[0:H, 0:W]
        o, d = camera_ray(pack_camera(cur_camera, W, H), xs.astype(F).astype(T) + T(0.5), ys.astype(F).astype(T) + T(0.5), T)
        P = tuple(o[k] + d[k] * t for k in range(3))
        n = np.zeros((H, W, 3), T)
        if normal is not None:
            ones = np.ones((H, W, 4), F)
            n = prepare(ones, None, normal, ones)["n"].astype(T)
        nb = tuple(n[..., k] for k in range(3))
        for i in moved_instances(cur_instances, prev_instances):
            m_cur, inv_cur = compose(cur_instances[i], T)
            m_prev, inv_prev = compose(prev_instances[i], T)
            sel = inst == i
            Pm = xf_point(m_prev, xf_point(inv_cur, P))
            P = tuple(np.where(sel, Pm[k], P[k]) for k in range(3))
            if normal is not None:
                u = xf_normal(inv_prev, xf_normal(m_cur, tuple(n[..., k] for k in range(3))))
                length = np.sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2])
                nb = tuple(np.where(sel, np.where(length > 0, u[k] / length, zero), nb[k]) for k in range(3))
        pr = project(P, prev_camera, W, H, T)
        ok = hit & pr["front"] & np.isfinite(pr["image_x"]) & np.isfinite(pr["image_y"]) & np.isfinite(pr["z_exp"])
        out = np.zeros((2, H, W, 4), T)
        for k, plane in enumerate((pr["image_x"], pr["image_y"], pr["z_exp"], np.ones((H, W), T))):
            out[0, ..., k] = np.where(ok, plane, zero)
        for k in range(3):
            out[1, ..., k] = nb[k]
        out[1, ..., 3] = np.where(hit, (inst + 1).astype(F).astype(T), zero)
    return out


def accumulate_motion(film, depth, motion, variance=None, normal=None, history=None, dtype=np.float32, alpha_min=0.1, max_history=64.0,
                      sigma_depth=0.05, cos_normal=0.9):
    """gbl_film_accumulate_motion: temporal_reference.accumulate with (image_x, image_y, z_exp) = M0.xyz, no history where
    M0.w == 0 and, with a normal film, M1.xyz in the tap test.  Same return value."""
    T = dtype
    p = prepare(film, variance, normal, depth)
    valid, surf = p["valid"], p["surf"]
    H, W = valid.shape
    c, l, n, z, v_cur = (p[k].astype(T) for k in ("c", "l", "n", "z", "v"))
    one, zero = T(1.0), T(0.0)
    sd, cn = T(F(sigma_depth)), T(F(cos_normal))
    taps = {k: np.zeros((4, H, W), bool) for k in ("inside", "live", "depth_ok", "normal_ok", "accepted")}
    ws = np.zeros((H, W), T)
    prev = {k: np.zeros((H, W), T) for k in ("r", "g", "b", "N", "m1", "m2", "v")}
    with np.errstate(all="ignore"):
        if history is not None:
            hist = np.asarray(history, F).reshape(3, H, W, 4)
            mo = np.asarray(motion, F).reshape(2, H, W, 4).astype(T)
            image_x, image_y, z_exp, front = mo[0, ..., 0], mo[0, ..., 1], mo[0, ..., 2], mo[0, ..., 3] != 0
            nt = mo[1, ..., :3]
            fx, fy = image_x - T(0.5), image_y - T(0.5)
            x0f, y0f = np.floor(fx), np.floor(fy)
            ok = (valid & surf & front & np.isfinite(fx) & np.isfinite(fy) & np.isfinite(z_exp) & (x0f >= -1) & (x0f < W) & (y0f >= -1) & (y0f < H))
            tx, ty = fx - x0f, fy - y0f
            x0 = np.where(ok, x0f, 0).astype(np.int64)
            y0 = np.where(ok, y0f, 0).astype(np.int64)
            ztol = sd * z_exp
            for j in (0, 1):
                for i in (0, 1):
                    qx, qy = x0 + i, y0 + j
                    inside = ok & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                    h = hist[:, np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)].astype(T)       # (3, H, W, 4)
                    live = (h[0, ..., 3] > 0) & (h[2, ..., 3] != 0)
                    depth_ok = np.abs(h[1, ..., 3] - z_exp) <= ztol
                    normal_ok = np.ones((H, W), bool)
                    if normal is not None:
                        normal_ok = (nt[..., 0] * h[2, ..., 0] + nt[..., 1] * h[2, ..., 1]) + nt[..., 2] * h[2, ..., 2] >= cn
                    use = inside & live & depth_ok & normal_ok
                    k = 2 * j + i
                    taps["inside"][k], taps["live"][k], taps["depth_ok"][k] = inside, inside & live, inside & depth_ok
                    taps["normal_ok"][k], taps["accepted"][k] = inside & normal_ok, use
                    b = (tx if i else one - tx) * (ty if j else one - ty)
                    ws = np.where(use, ws + b, ws)
                    for key, val in (("r", h[0, ..., 0]), ("g", h[0, ..., 1]), ("b", h[0, ..., 2]), ("N", h[0, ..., 3]), ("m1", h[1, ..., 0]),
                                     ("m2", h[1, ..., 1]), ("v", h[1, ..., 2])):
                        prev[key] = np.where(use, prev[key] + b * val, prev[key])
        has = ws > 0
        prev = {k: a / ws for k, a in prev.items()}
        N = np.where(has, np.minimum(prev["N"] + one, T(F(max_history))), one)
        alpha = np.where(has, np.maximum(one / N, T(F(alpha_min))), one)
        pc = np.stack([prev["r"], prev["g"], prev["b"]], -1)
        c_out = np.where(has[..., None], pc + alpha[..., None] * (c - pc), c)
        m1 = np.where(has, prev["m1"] + alpha * (l - prev["m1"]), l)
        m2 = np.where(has, prev["m2"] + alpha * (l * l - prev["m2"]), l * l)
        if variance is not None:
            ia = one - alpha
            v_out = np.where(has, (alpha * alpha) * v_cur + (ia * ia) * prev["v"], v_cur)
        else:
            ztol = sd * z
            total, m = np.zeros((H, W), T), np.zeros((H, W), np.int32)

            def counts(dy, dx):
                q = shift(valid, dy, dx) & (shift(surf, dy, dx) == surf)
                return q & (~surf | (np.abs(shift(z, dy, dx) - z) <= ztol))
            for dy in (-2, -1, 0, 1, 2):
                for dx in (-2, -1, 0, 1, 2):
                    q = counts(dy, dx)
                    total = np.where(q, total + shift(l, dy, dx), total)
                    m += q
            mf = m.astype(F).astype(T)
            mean = total / mf
            ss = np.zeros((H, W), T)
            for dy in (-2, -1, 0, 1, 2):
                for dx in (-2, -1, 0, 1, 2):
                    dl = shift(l, dy, dx) - mean
                    ss = np.where(counts(dy, dx), ss + dl * dl, ss)
            spatial = np.where(m >= 2, ss / (mf - one), zero)
            s2 = np.where(N >= 4, np.maximum(zero, m2 - m1 * m1), spatial)
            v_out = s2 / N
        out_film = np.zeros((H, W, 4), T)
        out_film[..., :3] = np.where(valid[..., None], c_out, zero)
        out_film[..., 3] = np.where(valid, one, zero)
        out_hist = np.zeros((3, H, W, 4), T)
        out_hist[0, ..., :3] = out_film[..., :3]
        out_hist[0, ..., 3] = np.where(valid, N, zero)
        for k, plane in enumerate((m1, m2, v_out, z)):
            out_hist[1, ..., k] = np.where(valid, plane, zero)
        out_hist[2, ..., :3] = np.where(valid[..., None], n, zero)
        out_hist[2, ..., 3] = np.where(valid & surf, one, zero)
        out_var = np.where(valid, v_out, zero).astype(T)
    return dict(film=out_film, variance=out_var, history=out_hist, has_history=has & valid, N=out_hist[0, ..., 3], valid=valid, surf=surf, taps=taps)


# ---- the fixture -------------------------------------------------------------------------------------------------------
SQUARE_Z, WALL_Z, WALL_X_MAX = 5.0, 8.0, 6.0     # a square at z = 5 in front of a wall z = 8 that ends at x = 6; beyond it: nothing
SQUARE_HALF = (1.5, 1.0)
PERIOD = 1.6                                     # of the square's stripes, in object space
SHIFT = 0.5 * PERIOD                             # the slide per frame: half a period, so a stale texel is the opposite stripe


def _stripes(x_obj):
    s = np.cos(2.0 * np.pi * x_obj / PERIOD)
    return np.stack([0.5 + 0.4 * s, 0.5 - 0.4 * s, np.full_like(s, 0.25)], -1)


def _wall(P):
    return np.stack([0.55 + 0.3 * np.sin(0.7 * P[0]), 0.5 + 0.3 * np.cos(0.9 * P[1] + 0.3 * P[0]), np.full_like(P[0], 0.6)], -1)


def _frame(cam, width, height, square_x):
    """Per pixel centre, in float64: hit distance, instance (0 wall, 1 square, -1 nothing) and colour."""
    c = pack_camera(cam, width, height)
    ys, xs = np.mgrid[0:height, 0:width]
    o, d = camera_ray(c, xs + 0.5, ys + 0.5, np.float64)
    t_sq, t_wall = (SQUARE_Z - o[2]) / d[2], (WALL_Z - o[2]) / d[2]
    P_sq = tuple(o[k] + t_sq * d[k] for k in range(3))
    P_wall = tuple(o[k] + t_wall * d[k] for k in range(3))
    on_sq = (np.abs(P_sq[0] - square_x) < SQUARE_HALF[0]) & (np.abs(P_sq[1]) < SQUARE_HALF[1])
    on_wall = ~on_sq & (P_wall[0] < WALL_X_MAX)
    inst = np.where(on_sq, 1, np.where(on_wall, 0, -1)).astype(np.int32)
    t = np.where(on_sq, t_sq, np.where(on_wall, t_wall, 0.0))
    colour = np.where(on_sq[..., None], _stripes(P_sq[0] - square_x), np.where(on_wall[..., None], _wall(P_wall), 0.1))
    return t.astype(F), inst, colour.astype(F)


@functools.lru_cache(maxsize=None)
def moving_sequence(width=37, height=23, shift_x=SHIFT, seed=20261020):
    """Two analytic frames under one still camera at the origin looking down +z: a striped square (instance 1) slides by
    ``shift_x`` along x in front of a wall (instance 0).  Its previous left edge lies 1.2 pixels outside the image, so the leading
    pixels of the square reproject past the border and the wall pixels behind its trailing edge are disoccluded; right of the
    wall's end the rays hit nothing.  ``shift_x`` = 0 is the static scene.

    dict of the current frame's float32 accumulators film / normal / depth (H, W, 4) and variance (H, W); their weights are powers
    of two, so the films resolve to the centre ray's colour, normal and hit distance exactly; the previous frame's prev_film /
    prev_normal / prev_depth; ``history`` (3, H, W, 4): the previous frame's colour, depth and normal with N in [1, max_history],
    holes (N = 0) and a block of N = 1; the camera (``cur_camera`` = ``prev_camera``), ``cur_instances`` / ``prev_instances``
    (position, orientation, scale), the centre rays' ``t`` and ``inst`` of both frames, ``analytic`` (H, W, 3) -- the current
    frame's exact colour -- and ``motion`` (2, H, W, 4), the planes of ``motion_planes`` for them, and ``params``.  The current
    frame has one NaN colour and one pixel of weight 0 where they fit."""
    rng = np.random.default_rng(seed)
    H, W = height, width
    cam = camera()
    c = pack_camera(cam, W, H)
    pixel = 2.0 * SQUARE_Z / float(c["proj00"]) / W                      # world units per pixel at the square's depth
    x_prev = float(F(-SQUARE_Z / float(c["proj00"]) - 1.2 * pixel + SQUARE_HALF[0]))
    x_cur = float(F(x_prev + shift_x))
    prev_instances = (IDENTITY, ((x_prev, 0.0, 0.0), IDENTITY[1], IDENTITY[2]))
    cur_instances = (IDENTITY, ((x_cur, 0.0, 0.0), IDENTITY[1], IDENTITY[2]))
    big = W >= 12 and H >= 16
    nrm = np.broadcast_to(np.array([0.0, 0.0, -1.0], F), (H, W, 3))

    def films(t, inst, colour, w):
        cov = (inst >= 0).astype(F)
        film = np.concatenate([colour * w[..., None], w[..., None]], -1).astype(F)
        normal = np.concatenate([nrm * (cov * w)[..., None], w[..., None]], -1).astype(F)
        depth = np.stack([t * cov * w, cov * w, np.zeros((H, W), F), w], -1).astype(F)
        return film, normal, depth
    t0, inst0, colour0 = _frame(cam, W, H, x_prev)
    t1, inst1, colour1 = _frame(cam, W, H, x_cur)
    prev_film, prev_normal, prev_depth = films(t0, inst0, colour0, np.ones((H, W), F))
    w = np.exp2(rng.integers(-1, 3, (H, W))).astype(F)
    film, normal, depth = films(t1, inst1, colour1, w)
    variance = rng.uniform(0.0, 0.1, (H, W)).astype(F)
    if W >= 4 and H >= 3:
        film[H // 2, (3 * W) // 4] = 0.0                 # weight 0
        film[1, W // 2, 1] = np.nan                      # a NaN colour
    max_history = SEQUENCE_PARAMS["max_history"]
    N = rng.uniform(1.0, max_history, (H, W)).astype(F)
    N[rng.uniform(0.0, 1.0, (H, W)) < 0.06] = 0.0        # holes
    if big:
        N[15:21, 20:27] = 1.0                            # a young block: N stays below 4 after the blend
    hl = lum(colour0[..., 0], colour0[..., 1], colour0[..., 2])
    history = np.zeros((3, H, W, 4), F)
    history[0] = np.concatenate([colour0, N[..., None]], -1)
    history[1] = np.stack([hl, hl * hl + rng.uniform(0.0, 0.02, (H, W)).astype(F), rng.uniform(0.0, 0.02, (H, W)).astype(F), t0], -1)
    history[2] = np.concatenate([nrm * (inst0 >= 0)[..., None], (inst0 >= 0).astype(F)[..., None]], -1)
    history[:, N == 0] = 0.0
    motion = motion_planes(t1, inst1, cam, cam, cur_instances, prev_instances, normal)
    out = dict(film=film, normal=normal, depth=depth, variance=variance, history=history, cur_camera=cam, prev_camera=cam,
               prev_film=prev_film, prev_normal=prev_normal, prev_depth=prev_depth, cur_instances=cur_instances, prev_instances=prev_instances,
               t=t1, inst=inst1, prev_t=t0, prev_inst=inst0, analytic=colour1, prev_analytic=colour0, motion=motion, params=dict(SEQUENCE_PARAMS))
    for arr in out.values():
        if isinstance(arr, np.ndarray):
            arr.setflags(write=False)
    return out
