"""TEST INFRASTRUCTURE: the contract of gbl_film_accumulate (include/goblin_hip.h) in numpy.

``accumulate`` restates kernels/temporal.h operation by operation, in the kernel's order.  With ``dtype`` float32 (the default)
every add, mul, div, sqrt and floor is the kernel's, so the outputs are the device's bit for bit: there is no transcendental
function in the contract.  The one the host evaluates, tanf of half the field of view in ``pack_camera``, is taken from the C
library the device library's host side calls.  ``prepare`` always runs in float32; with ``dtype`` float64 the arithmetic after it
runs in double -- a diagnostic of how far float32's rounding moves a value, never a reference for a decision.

``synthetic_sequence`` is the pair of frames the tests accumulate; computed once per shape and shared read-only.
"""
import ctypes
import ctypes.util
import functools

import numpy as np

from denoise_reference import lum, shift

F = np.float32
K_PI = F(3.14159265358979323)
DEFAULTS = dict(alpha_min=0.1, max_history=64.0, sigma_depth=0.05, cos_normal=0.9)
CAMERA_FIELDS = ("position", "orientation", "fov_degrees", "near_plane", "far_plane", "lens_radius", "focal_distance", "type", "film_width")


@functools.lru_cache(maxsize=None)
def _libm():
    lib = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    lib.tanf.restype = ctypes.c_float
    lib.tanf.argtypes = [ctypes.c_float]
    return lib


def camera(position=(0.0, 0.0, 0.0), orientation=(1.0, 0.0, 0.0, 0.0), fov_degrees=60.0, type=0, film_width=35.0, lens_radius=0.0,
           focal_distance=1.0, near_plane=0.1, far_plane=100.0):
    """A camera description with gbl_camera's fields, as a dict."""
    return dict(position=tuple(float(F(v)) for v in position), orientation=tuple(float(F(v)) for v in orientation),
                fov_degrees=float(F(fov_degrees)), near_plane=near_plane, far_plane=far_plane, lens_radius=float(F(lens_radius)),
                focal_distance=focal_distance, type=int(type), film_width=float(F(film_width)))


def pack_camera(cam, width, height):
    """scene_prep.cpp pack_camera in float32."""
    aspect = F(width) / F(height)
    fov = K_PI * (F(cam["fov_degrees"]) / F(180.0))
    ys = F(1.0) / F(_libm().tanf(fov / F(2.0)))
    return dict(pos=np.array(cam["position"], F), q=np.array(cam["orientation"], F), proj11=ys, proj00=ys / aspect,
                inv_xres=F(1.0) / F(width), inv_yres=F(1.0) / F(height), type=int(cam["type"]), film_w=F(cam["film_width"]),
                film_h=F(cam["film_width"]) / aspect)


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def quat_rotate(q, v, T=F):
    """Quaternion (w, x, y, z) times vector, kernels/temporal.h tp_quat_rotate."""
    qw, qv = q[0], (q[1], q[2], q[3])
    uv = _cross(qv, v)
    uuv = _cross(qv, uv)
    s = T(2.0) * qw
    uv = tuple(c * s for c in uv)
    uuv = tuple(c * T(2.0) for c in uuv)
    return tuple((v[k] + uv[k]) + uuv[k] for k in range(3))


def camera_ray(c, image_x, image_y, T=F):
    """tp_camera_ray: (o, d), three arrays each."""
    q, pos = [T(v) for v in c["q"]], [T(v) for v in c["pos"]]
    xndc = T(2.0) * image_x * T(c["inv_xres"]) - T(1.0)
    yndc = T(-2.0) * image_y * T(c["inv_yres"]) + T(1.0)
    zero, one = np.zeros_like(xndc), np.ones_like(xndc)
    if c["type"] == 1:
        xv = T(0.5) * T(c["film_w"]) * xndc
        yv = T(0.5) * T(c["film_h"]) * yndc
        r = quat_rotate(q, (xv, yv, zero), T)
        return tuple(pos[k] + r[k] for k in range(3)), quat_rotate(q, (zero, zero, one), T)
    xv = xndc / T(c["proj00"])
    yv = yndc / T(c["proj11"])
    inv = T(1.0) / np.sqrt(xv * xv + yv * yv + one * one)
    return tuple(np.full_like(xndc, pos[k]) for k in range(3)), quat_rotate(q, (xv * inv, yv * inv, one * inv), T)


def prepare(film, variance=None, normal=None, depth=None):
    """temporal_prepare_kernel, float32: dict(c (H, W, 3), l, n, z, valid, surf)."""
    film = np.asarray(film, F)
    H, W = film.shape[:2]
    one, zero = F(1.0), F(0.0)
    with np.errstate(all="ignore"):
        w = film[..., 3]
        c = (film[..., :3] * (one / w)[..., None]).astype(F)
        n = np.zeros((H, W, 3), F)
        if normal is not None:
            nacc = np.asarray(normal, F)
            nw = nacc[..., 3]
            n = np.where((nw != 0)[..., None], nacc[..., :3] * (one / nw)[..., None], zero).astype(F)
            length = np.sqrt((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]).astype(F)
            n = np.where((length > 0)[..., None], n / length[..., None], zero).astype(F)
        dacc = np.asarray(depth, F)
        z = np.where(dacc[..., 1] != 0, dacc[..., 0] / dacc[..., 1], zero).astype(F)
        coverage = np.where(dacc[..., 3] != 0, dacc[..., 1] / dacc[..., 3], zero).astype(F)
        surf = coverage > 0
        v = np.asarray(variance, F) if variance is not None else np.zeros((H, W), F)
        valid = (w > 0) & np.isfinite(c).all(-1) & np.isfinite(n).all(-1) & np.isfinite(z) & np.isfinite(v)
        l = lum(c[..., 0], c[..., 1], c[..., 2])
    return dict(c=c, l=l, n=n, z=z, v=v, valid=valid, surf=surf)


def accumulate(film, depth, cur_camera, variance=None, normal=None, history=None, prev_camera=None, dtype=np.float32, alpha_min=0.1,
               max_history=64.0, sigma_depth=0.05, cos_normal=0.9):
    """gbl_film_accumulate.  Returns dict(film (H, W, 4), variance (H, W), history (3, H, W, 4)) in ``dtype`` plus what the tests
    ask about a pixel: has_history, N, and per tap (4, H, W) inside / live / depth_ok / normal_ok / accepted."""
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
            cur, prv = pack_camera(cur_camera, W, H), pack_camera(prev_camera, W, H)
            ys, xs = np.mgrid[0:H, 0:W]
            o, d = camera_ray(cur, xs.astype(F).astype(T) + T(0.5), ys.astype(F).astype(T) + T(0.5), T)
            P = tuple(o[k] + d[k] * z for k in range(3))
            w = tuple(P[k] - T(prv["pos"][k]) for k in range(3))
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
                        normal_ok = (n[..., 0] * h[2, ..., 0] + n[..., 1] * h[2, ..., 1]) + n[..., 2] * h[2, ..., 2] >= cn
                    use = inside & live & depth_ok & normal_ok
                    t = 2 * j + i
                    taps["inside"][t], taps["live"][t], taps["depth_ok"][t] = inside, inside & live, inside & depth_ok
                    taps["normal_ok"][t], taps["accepted"][t] = inside & normal_ok, use
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


def bound(ref32, ref64):
    """The tolerance of a plane that is not restatable bit for bit (tests/denoise_reference.py bound)."""
    return 8.0 * float(np.abs(ref32.astype(np.float64) - ref64).max()) + 1e-6 * float(np.abs(ref64).max())


# ---- the fixture -------------------------------------------------------------------------------------------------------
NEAR_Z, FAR_Z, STEP_X = 5.0, 8.0, 0.3      # a half plane z = 5 over x < 0.3 in front of a wall z = 8, both facing the camera
SEQUENCE_PARAMS = dict(alpha_min=0.1, max_history=8.0, sigma_depth=0.05, cos_normal=0.9)


def _trace(cam, width, height):
    """Per pixel centre, in float64: distance along the camera ray to the first of the two planes, the world hit point."""
    c = pack_camera(cam, width, height)
    ys, xs = np.mgrid[0:height, 0:width]
    o, d = camera_ray(c, xs + 0.5, ys + 0.5, np.float64)
    t_near = (NEAR_Z - o[2]) / d[2]
    near = o[0] + t_near * d[0] < STEP_X
    t = np.where(near, t_near, (FAR_Z - o[2]) / d[2])
    return t, tuple(o[k] + t * d[k] for k in range(3)), near


def _colour(P):
    return np.stack([0.55 + 0.4 * np.sin(1.3 * P[0]), 0.5 + 0.4 * np.cos(0.9 * P[1] + 0.3 * P[0]), 0.3 + 0.05 * P[2]], -1)


@functools.lru_cache(maxsize=None)
def synthetic_sequence(width=37, height=23, seed=20261019):
    """Two analytic frames of the two planes: ``prev_camera`` at the origin looking down +z, ``cur_camera`` one unit to its right
    and yawed by 0.02 rad.  dict of the current frame's float32 accumulators film / normal / depth (H, W, 4) and variance (H, W),
    all with a non-uniform filter weight; ``history`` (3, H, W, 4), the previous frame's: its analytic colour, depth and normal,
    N in [1, max_history] with holes (N = 0), a block of N = 1, a patch whose normal has since turned and a patch without
    coverage; the two cameras and ``params``.  The current frame has a patch without coverage, one NaN colour and one pixel of
    weight 0 where they fit."""
    rng = np.random.default_rng(seed)
    H, W = height, width
    half = 0.01
    prev_camera = camera()
    cur_camera = camera(position=(1.0, 0.0, 0.0), orientation=(np.cos(half), 0.0, np.sin(half), 0.0))
    big = W >= 12 and H >= 16
    frames = {}
    for name, cam in (("prev", prev_camera), ("cur", cur_camera)):
        t, P, near = _trace(cam, W, H)
        frames[name] = dict(z=t.astype(F), colour=_colour(P).astype(F), near=near)
    nrm = np.broadcast_to(np.array([0.0, 0.0, -1.0], F), (H, W, 3))
    # the current frame
    w = rng.uniform(0.5, 4.0, (H, W)).astype(F)
    colour = (frames["cur"]["colour"] + rng.normal(0.0, 0.08, (H, W, 3))).astype(F)
    coverage = np.ones((H, W), F)
    if big:
        coverage[3:7, 20:25] = 0.0
    film = np.concatenate([colour * w[..., None], w[..., None]], -1).astype(F)
    normal = np.concatenate([nrm * (coverage * w)[..., None], w[..., None]], -1).astype(F)
    depth = np.stack([frames["cur"]["z"] * coverage * w, coverage * w, np.zeros((H, W), F), w], -1).astype(F)
    variance = rng.uniform(0.0, 0.1, (H, W)).astype(F)
    if W >= 4 and H >= 3:
        film[H // 2, W // 4] = 0.0                       # weight 0
        film[1, (3 * W) // 4, 1] = np.nan                # a NaN colour
    # the previous frame's history
    max_history = SEQUENCE_PARAMS["max_history"]
    N = rng.uniform(1.0, max_history, (H, W)).astype(F)
    N[rng.uniform(0.0, 1.0, (H, W)) < 0.06] = 0.0        # holes
    hn = nrm.copy()
    hsurf = np.ones((H, W), F)
    if big:
        N[15:21, 2:9] = 1.0                              # a young block: N stays below 4 after the blend
        hn[9:14, 26:31] = np.array([1.0, 0.0, 0.0], F)   # the surface's normal has turned since
        hsurf[16:20, 28:33] = 0.0                        # no coverage
    hc = (frames["prev"]["colour"] + rng.normal(0.0, 0.03, (H, W, 3))).astype(F)
    hl = lum(hc[..., 0], hc[..., 1], hc[..., 2])
    history = np.zeros((3, H, W, 4), F)
    history[0] = np.concatenate([hc, N[..., None]], -1)
    history[1] = np.stack([hl, hl * hl + rng.uniform(0.0, 0.02, (H, W)).astype(F), rng.uniform(0.0, 0.02, (H, W)).astype(F), frames["prev"]["z"]], -1)
    history[2] = np.concatenate([hn, hsurf[..., None]], -1)
    history[:, N == 0] = 0.0
    out = dict(film=film, normal=normal, depth=depth, variance=variance, history=history, cur_camera=cur_camera, prev_camera=prev_camera,
               params=dict(SEQUENCE_PARAMS))
    for arr in out.values():
        if isinstance(arr, np.ndarray):
            arr.setflags(write=False)
    return out
