"""TEST INFRASTRUCTURE: the contract of gbl_film_variance and gbl_film_denoise (include/goblin_hip.h) in numpy.

``variance`` restates the device's order of sums -- per pixel, one sum of the finite luminances over k = 0 .. S-1, then one sum
of the squared deviations over the same k -- in float32, operation by operation, so its plane is the device's bit for bit.

``denoise`` takes a ``dtype``.  ``prepare`` and with it every validity, threshold and coverage decision always runs in float32,
as on the device; only the arithmetic of the levels and the final multiplication run in ``dtype``.  With float32 every
operation is the kernel's in the kernel's order (numpy's exp in the place of gbl_expf); with float64 it is the same formula
without float32's rounding, and the distance between the two is what the GPU tests build their tolerance from.

``synthetic`` is the film the tests filter; computed once per shape and shared read-only.
"""
import functools

import numpy as np

F = np.float32
K5 = (0.375, 0.25, 0.0625)      # a-trous taps by |offset|
K3 = (0.5, 0.25)                # variance prefilter
DEFAULTS = dict(iterations=5, sigma_luminance=4.0, sigma_normal=0.5, sigma_albedo=0.1, sigma_depth=0.1, demodulate=True)


def lum(r, g, b, T=np.float32):
    return (T(F(0.2126)) * r + T(F(0.7152)) * g) + T(F(0.0722)) * b


def round_to_square(spp):
    return int(np.ceil(np.sqrt(np.float32(spp)))) ** 2


def variance(li, window, spp, xres, yres, out=None):
    """gbl_film_variance: li (n, 4) float32 in li_out order over ``window`` (x0, x1, y0, y1), S = round_to_square(spp) entries
    per pixel.  Returns the (yres, xres) float32 plane; pixels outside the window keep what ``out`` held (zeros if None)."""
    S = round_to_square(spp)
    x0, x1, y0, y1 = window
    ww, wh = x1 - x0, y1 - y0
    li = np.ascontiguousarray(li, F).reshape(wh, ww, S, 4)
    with np.errstate(all="ignore"):
        total = np.zeros((wh, ww), F)
        m = np.zeros((wh, ww), np.int32)
        for k in range(S):
            l = lum(li[:, :, k, 0], li[:, :, k, 1], li[:, :, k, 2])
            fin = np.isfinite(l)
            total = np.where(fin, total + l, total).astype(F)
            m += fin
        mf = m.astype(F)
        mean = total / mf
        ss = np.zeros((wh, ww), F)
        for k in range(S):
            l = lum(li[:, :, k, 0], li[:, :, k, 1], li[:, :, k, 2])
            d = l - mean
            ss = np.where(np.isfinite(l), ss + d * d, ss).astype(F)
        var = np.where(m >= 2, ss / (mf * (mf - F(1.0))), F(0.0)).astype(F)
    out = np.zeros((yres, xres), F) if out is None else out
    ys, xs = np.mgrid[y0:y1, x0:x1]
    inside = (xs >= 0) & (xs < xres) & (ys >= 0) & (ys < yres)
    out[ys[inside], xs[inside]] = var[inside]
    return out


def prepare(film, variance=None, albedo=None, normal=None, depth=None, demodulate=True):
    """The prepare pass, float32: dict(c (H, W, 3) = colour / d, v, n, z, a, d, valid, surf)."""
    film = np.asarray(film, F)
    H, W = film.shape[:2]
    one, zero = F(1.0), F(0.0)

    def resolved(accum):
        w = accum[..., 3]
        return np.where((w != 0)[..., None], accum[..., :3] * (one / w)[..., None], zero).astype(F)
    with np.errstate(all="ignore"):
        w = film[..., 3]
        c = (film[..., :3] * (one / w)[..., None]).astype(F)
        a = resolved(np.asarray(albedo, F)) if albedo is not None else np.zeros((H, W, 3), F)
        n = np.zeros((H, W, 3), F)
        if normal is not None:
            n = resolved(np.asarray(normal, F))
            length = np.sqrt((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]).astype(F)
            n = np.where((length > 0)[..., None], n / length[..., None], zero).astype(F)
        z, coverage = np.zeros((H, W), F), np.ones((H, W), F)     # no depth film: every pixel counts as covered
        if depth is not None:
            dacc = np.asarray(depth, F)
            z = np.where(dacc[..., 1] != 0, dacc[..., 0] / dacc[..., 1], zero).astype(F)
            coverage = np.where(dacc[..., 3] != 0, dacc[..., 1] / dacc[..., 3], zero).astype(F)
        surf = coverage > 0
        demod = bool(demodulate) and albedo is not None
        d = np.where(demod & surf[..., None] & (a >= F(1e-2)), a, one).astype(F)
        c = (c / d).astype(F)
        v = np.zeros((H, W), F)
        if variance is not None:
            ld = lum(d[..., 0], d[..., 1], d[..., 2])
            v = (np.asarray(variance, F) / (ld * ld)).astype(F)
        valid = (w > 0) & np.isfinite(c).all(-1) & np.isfinite(a).all(-1) & np.isfinite(n).all(-1) & np.isfinite(z) & np.isfinite(v)
    return dict(c=c, v=v, n=n, z=z, a=a, d=d, valid=valid, surf=surf)


def shift(arr, oy, ox):
    """out[y, x] = arr[y + oy, x + ox], zero (False) where that lies outside the image."""
    out = np.zeros_like(arr)
    H, W = arr.shape[:2]
    ya, yb, xa, xb = max(0, -oy), min(H, H - oy), max(0, -ox), min(W, W - ox)
    if ya < yb and xa < xb:
        out[ya:yb, xa:xb] = arr[ya + oy:yb + oy, xa + ox:xb + ox]
    return out


def sq_len(d):
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def denoise(film, variance=None, albedo=None, normal=None, depth=None, dtype=np.float32, iterations=5, sigma_luminance=4.0,
            sigma_normal=0.5, sigma_albedo=0.1, sigma_depth=0.1, demodulate=True):
    """gbl_film_denoise: the (H, W, 4) film_out, in ``dtype``."""
    T = dtype
    p = prepare(film, variance, albedo, normal, depth, demodulate)
    valid, surf = p["valid"], p["surf"]
    c, v, n, z, a = (p[k].astype(T) for k in ("c", "v", "n", "z", "a"))
    one, zero, eps = T(1.0), T(0.0), T(F(1e-6))
    sl = T(F(sigma_luminance))
    inv_sn2 = one / (T(F(sigma_normal)) * T(F(sigma_normal))) if normal is not None else zero
    inv_sa2 = one / (T(F(sigma_albedo)) * T(F(sigma_albedo))) if albedo is not None else zero
    with np.errstate(all="ignore"):
        for level in range(iterations):
            s = 1 << level
            sd = np.ones(valid.shape, T)
            if variance is not None:
                gs, gw = np.zeros(valid.shape, T), np.zeros(valid.shape, T)
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        ok = shift(valid, dy, dx)
                        kw = T(K3[abs(dx)]) * T(K3[abs(dy)])
                        gs = np.where(ok, gs + kw * shift(v, dy, dx), gs)
                        gw = np.where(ok, gw + kw, gw)
                sd = np.sqrt(gs / gw)
            inv_l = one / (sl * sd + eps)
            inv_z = one / ((T(F(sigma_depth)) * T(s)) * np.maximum(np.abs(z), eps)) if depth is not None else np.zeros(valid.shape, T)
            lum_p = lum(c[..., 0], c[..., 1], c[..., 2], T)
            total, ws, sv = np.zeros(c.shape, T), np.zeros(valid.shape, T), np.zeros(valid.shape, T)
            for dy in (-2, -1, 0, 1, 2):
                for dx in (-2, -1, 0, 1, 2):
                    oy, ox = s * dy, s * dx
                    use = shift(valid, oy, ox) & (shift(surf, oy, ox) == surf)
                    cq, vq = shift(c, oy, ox), shift(v, oy, ox)
                    h = T(K5[abs(dx)]) * T(K5[abs(dy)])
                    e = np.abs(lum(cq[..., 0], cq[..., 1], cq[..., 2], T) - lum_p) * inv_l
                    g2 = (sq_len(shift(n, oy, ox) - n) * inv_sn2 + np.abs(shift(z, oy, ox) - z) * inv_z) + sq_len(shift(a, oy, ox) - a) * inv_sa2
                    g2 = np.where(surf, g2, zero)
                    wt = (h * np.exp(-(e + g2))).astype(T)
                    total = np.where(use[..., None], total + wt[..., None] * cq, total)
                    ws = np.where(use, ws + wt, ws)
                    sv = np.where(use, sv + (wt * wt) * vq, sv)
            c = np.where(valid[..., None], total / ws[..., None], c).astype(T)
            v = np.where(valid, sv / (ws * ws), v).astype(T)
        out = np.zeros(c.shape[:2] + (4,), T)
        out[..., :3] = np.where(valid[..., None], c * p["d"].astype(T), zero)
        out[..., 3] = np.where(valid, one, zero)
    return out


def bound(ref32, ref64):
    """The GPU tests' tolerance: 8 max|ref32 - ref64| + 1e-6 max|ref64|."""
    return 8.0 * float(np.abs(ref32.astype(np.float64) - ref64).max()) + 1e-6 * float(np.abs(ref64).max())


def rel_mse(x, ref):
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float(np.mean((x - ref) ** 2 / (ref ** 2 + 0.01)))


@functools.lru_cache(maxsize=None)
def synthetic(width=37, height=23, holes=True, seed=20261018):
    """The film of the tests: weights in [0.5, 4]; colour in [0, 1] on the left half and [10, 11] on the right; normals +x left
    and +y right; albedo in [0.2, 0.9]; depth 5 + 0.05 x; variance in [0, 0.1]; with ``holes`` (where they fit) one pixel of
    weight 0, one NaN and a 4 x 7 patch of coverage 0 inside the left half.  dict of float32 accumulators film / albedo /
    normal / depth (H, W, 4), variance (H, W), plus left (H, W) bool."""
    rng = np.random.default_rng(seed)
    H, W = height, width
    w = rng.uniform(0.5, 4.0, (H, W)).astype(F)
    left = np.broadcast_to(np.arange(W)[None, :] < (W + 1) // 2, (H, W)).copy()
    colour = rng.uniform(0.0, 1.0, (H, W, 3)).astype(F) + np.where(left, F(0.0), F(10.0))[..., None].astype(F)
    alb = rng.uniform(0.2, 0.9, (H, W, 3)).astype(F)
    nrm = np.where(left[..., None], np.array([1, 0, 0], F), np.array([0, 1, 0], F)).astype(F)
    z = np.broadcast_to((5.0 + 0.05 * np.arange(W))[None, :], (H, W)).astype(F)
    var = rng.uniform(0.0, 0.1, (H, W)).astype(F)
    coverage = np.ones((H, W), F)
    if holes and W >= 12 and H >= 16:
        coverage[8:15, 5:9] = 0.0          # 4 wide, 7 high, inside the left half
    elif holes and W >= 2:
        coverage[0, 0] = 0.0
    hit = coverage[..., None]
    film = np.concatenate([colour * w[..., None], w[..., None]], -1).astype(F)
    albedo = np.concatenate([alb * hit * w[..., None], w[..., None]], -1).astype(F)
    normal = np.concatenate([nrm * hit * w[..., None], w[..., None]], -1).astype(F)
    depth = np.stack([z * coverage * w, coverage * w, np.zeros((H, W), F), w], -1).astype(F)
    if holes and W >= 4 and H >= 3:
        film[H // 2, W // 4] = 0.0                       # weight 0
        film[1, (3 * W) // 4, 1] = np.nan                # a NaN colour
    out = dict(film=film, albedo=albedo, normal=normal, depth=depth, variance=var, left=left)
    for arr in out.values():
        arr.setflags(write=False)
    return out
