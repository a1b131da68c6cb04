// gbl_film_accumulate: reprojected temporal accumulation of a film.  The frame just rendered is blended into a
// caller-owned history that is fetched from where each pixel's surface point lay under the previous camera.  Plain IEEE single
// arithmetic in the order written here (this unit is built with -ffp-contract=off): add, mul, div, sqrt, floor and compares, no
// transcendental function, so tests/temporal_reference.py restates every operation below in numpy, in the same order, bit for bit.
//
// Passes of one call, on one stream:
//   temporal_prepare_kernel      resolves the current frame once, by denoise_prepare_kernel's rules without albedo, into
//                                   cl = {c.rgb, l}    colour F.rgb * (1 / F.w) and its luminance
//                                   nz = {n.xyz, z}    unit normal (or 0) and depth
//                                   fl = flags         VALID | SURF << 1
//   temporal_accumulate_kernel   32 x 8 pixel tiles, one lane per pixel: reproject, gather the history (four taps of three
//                                16-byte loads from global memory: neighbouring lanes land on neighbouring history pixels),
//                                blend, estimate the variance, write film_out, variance_out and the three history planes.
//                                SPATIAL = true (no variance plane given) stages {l, z, flags} of the tile and its 2-pixel halo in
//                                LDS once, every staged pixel bounds-checked against the image and one outside it staged as
//                                invalid, and takes the 25 reads of the spatial estimate from there; SPATIAL = false stages nothing.
// History planes (xres * yres float4 each): H0 = {c.rgb, N}, H1 = {m1, m2, v, z}, H2 = {n.xyz, surf ? 1 : 0}.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "temporal_args.h"
#include "vecmath.h"

__device__ __forceinline__ float tp_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
__device__ __forceinline__ bool tp_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// Quaternion * Vector3, as render_kernels.h quat_rotate
__device__ __forceinline__ F3 tp_quat_rotate(float qw, float qx, float qy, float qz, F3 v) {
    const F3 qv = f3(qx, qy, qz);
    F3 uv = cross(qv, v);
    F3 uuv = cross(qv, uv);
    uv = uv * (2.0f * qw);
    uuv = uuv * 2.0f;
    return v + uv + uuv;
}

// render_kernels.h camera_ray without its lens: the pinhole (a thin lens counts as its pinhole) and the orthographic camera
__device__ __forceinline__ void tp_camera_ray(const DevCamera& c, float image_x, float image_y, F3* o, F3* d) {
    const float xndc = +2.0f * image_x * c.inv_xres - 1.0f;
    const float yndc = -2.0f * image_y * c.inv_yres + 1.0f;
    const F3 pos = f3(c.pos[0], c.pos[1], c.pos[2]);
    if (c.type == 1u) {
        const float xv = 0.5f * c.film_w * xndc;
        const float yv = 0.5f * c.film_h * yndc;
        *o = pos + tp_quat_rotate(c.q[0], c.q[1], c.q[2], c.q[3], f3(xv, yv, 0.0f));
        *d = tp_quat_rotate(c.q[0], c.q[1], c.q[2], c.q[3], f3(0.0f, 0.0f, 1.0f));
        return;
    }
    const float xv = xndc / c.proj00;
    const float yv = yndc / c.proj11;
    *o = pos;
    *d = tp_quat_rotate(c.q[0], c.q[1], c.q[2], c.q[3], normalize(f3(xv, yv, 1.0f)));
}

// The projection of a world point through a packed camera, as the reprojection of temporal_accumulate_kernel states it below
// (w, v, the `front` rule per camera type, xndc, yndc, z_exp, image_x, image_y).  Returns `front`; kernels/motion.h writes what
// this returns into its planes, so the two accumulate calls see the same numbers.
__device__ __forceinline__ bool tp_project(const DevCamera& prev, F3 P, int W, int H, float* image_x, float* image_y, float* z_exp_out) {
    const F3 w = P - f3(prev.pos[0], prev.pos[1], prev.pos[2]);
    const F3 v = tp_quat_rotate(prev.q[0], -prev.q[1], -prev.q[2], -prev.q[3], w);
    float xndc, yndc, z_exp;
    bool front;
    if (prev.type == 1u) {
        front = v.z >= 0.0f;
        xndc = v.x / (0.5f * prev.film_w);
        yndc = v.y / (0.5f * prev.film_h);
        z_exp = v.z;
    } else {
        front = v.z > 0.0f;
        xndc = (v.x / v.z) * prev.proj00;
        yndc = (v.y / v.z) * prev.proj11;
        z_exp = sqrtf((w.x * w.x + w.y * w.y) + w.z * w.z);
    }
    *image_x = ((xndc + 1.0f) * 0.5f) * static_cast<float>(W);
    *image_y = ((1.0f - yndc) * 0.5f) * static_cast<float>(H);
    *z_exp_out = z_exp;
    return front;
}

#ifndef GBL_TEMPORAL_NO_PREPARE   // (kernels_motion.hip includes this header for everything but the one kernel that is no template)
__global__ void temporal_prepare_kernel(const float4* __restrict__ film, const float* __restrict__ variance, const float4* __restrict__ normal,
                                        const float4* __restrict__ depth, float4* __restrict__ cl, float4* __restrict__ nz, uint32_t* __restrict__ fl,
                                        int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 F = film[i];
    const float inv = 1.0f / F.w;
    const float cr = F.x * inv, cg = F.y * inv, cb = F.z * inv;
    float nx = 0.0f, ny = 0.0f, nzz = 0.0f;
    if (normal) {
        const float4 N = normal[i];
        if (N.w != 0.0f) {
            const float in = 1.0f / N.w;
            nx = N.x * in;
            ny = N.y * in;
            nzz = N.z * in;
        }
        const float len = sqrtf((nx * nx + ny * ny) + nzz * nzz);
        if (len > 0.0f) {
            nx = nx / len;
            ny = ny / len;
            nzz = nzz / len;
        } else {
            nx = ny = nzz = 0.0f;
        }
    }
    const float4 D = depth[i];      // gbl_aov_resolve_depth's rule
    const float z = D.y != 0.0f ? D.x / D.y : 0.0f;
    const float coverage = D.w != 0.0f ? D.y / D.w : 0.0f;
    const bool surf = coverage > 0.0f;
    const float v = variance ? variance[i] : 0.0f;
    const bool valid = F.w > 0.0f && tp_finite(cr) && tp_finite(cg) && tp_finite(cb) && tp_finite(nx) && tp_finite(ny) && tp_finite(nzz) &&
                       tp_finite(z) && tp_finite(v);
    cl[i] = make_float4(cr, cg, cb, tp_lum(cr, cg, cb));
    nz[i] = make_float4(nx, ny, nzz, z);
    fl[i] = (valid ? GBL_TP_VALID : 0u) | (surf ? GBL_TP_SURF : 0u);
}
#endif

// Per valid pixel p = (x, y) with colour c, luminance l, normal n, depth z:
//   reproject  (covered p, history given)  (o, d) = the context camera's ray through (x + 0.5f, y + 0.5f); P = o + d * z;
//              w = P - pos_prev; v = w rotated by the conjugate of q_prev.
//              perspective:  v.z > 0;  xndc = (v.x / v.z) * proj00, yndc = (v.y / v.z) * proj11;  z_exp = sqrtf((w.x^2 + w.y^2) + w.z^2)
//              orthographic: v.z >= 0; xndc = v.x / (0.5f * film_w), yndc = v.y / (0.5f * film_h);  z_exp = v.z
//              image_x = ((xndc + 1) * 0.5f) * xres, image_y = ((1 - yndc) * 0.5f) * yres;  fx = image_x - 0.5f, x0 = floorf(fx),
//              tx = fx - x0, likewise y; a non-finite fx, fy or z_exp: no history
//   gather     taps (x0 + i, y0 + j), j = 0, 1 outer and i = 0, 1 inner, b = (i ? tx : 1 - tx) * (j ? ty : 1 - ty); accepted iff inside
//              the image, H0.N > 0, H2.w != 0, |H1.z - z_exp| <= sigma_depth * z_exp and, with a normal film,
//              (n.x n'.x + n.y n'.y) + n.z n'.z >= cos_normal.  ws = sum b; history iff ws > 0; previous value = (sum b * value) / ws
//   blend      no history: N = 1, alpha = 1, c_out = c, m1 = l, m2 = l * l.  Otherwise N = min(N_prev + 1, max_history),
//              alpha = max(1 / N, alpha_min), x_out = x_prev + alpha * (x - x_prev) for c, m1 (x = l) and m2 (x = l * l)
//   variance   with a plane: v_out = (alpha * alpha) * v_cur + ((1 - alpha) * (1 - alpha)) * v_prev, v_cur without history.
//              Without: v_out = s2 / N; s2 = max(0, m2 - m1 * m1) for N >= 4, else over the 5 x 5 neighbourhood (dy outer, dx inner)
//              of valid q with p's SURF and, on a covered p, |z_q - z_p| <= sigma_depth * z_p:  mean = (sum l) / m,
//              s2 = (sum (l - mean)^2) / (m - 1), 0 for m < 2
// An invalid pixel writes zeros to every output.
// MOTION (gbl_film_accumulate_motion): the reprojection is read from the planes of gbl_render_motion instead --
// (image_x, image_y, z_exp) = M0.xyz, no history where M0.w == 0 -- and, with a normal film, the taps are tested against M1.xyz, the
// current normal carried into the previous frame; H2 still stores n.  `motion` is not read otherwise.
template <bool SPATIAL, bool MOTION>
__device__ __forceinline__ void tp_accumulate(const float4* __restrict__ cl, const float4* __restrict__ nz, const uint32_t* __restrict__ fl,
                                              const float* __restrict__ variance, const float4* __restrict__ hist_in, float4* __restrict__ hist_out,
                                              float4* __restrict__ film_out, float* __restrict__ variance_out, const float4* __restrict__ motion,
                                              const TemporalArgs& a) {
    constexpr int SW = GBL_TP_TILE_W + 2 * GBL_TP_HALO, SH = GBL_TP_TILE_H + 2 * GBL_TP_HALO;
    __shared__ float s_l[SPATIAL ? SW * SH : 1];
    __shared__ float s_z[SPATIAL ? SW * SH : 1];
    __shared__ uint32_t s_f[SPATIAL ? SW * SH : 1];
    const int W = a.W, H = a.H, n = W * H;
    const int lx = threadIdx.x % GBL_TP_TILE_W, ly = threadIdx.x / GBL_TP_TILE_W;
    const int tx0 = blockIdx.x * GBL_TP_TILE_W, ty0 = blockIdx.y * GBL_TP_TILE_H;
    const int x = tx0 + lx, y = ty0 + ly;
    if (SPATIAL) {
        for (int i = threadIdx.x; i < SW * SH; i += GBL_TP_TILE_W * GBL_TP_TILE_H) {
            const int gx = tx0 - GBL_TP_HALO + i % SW, gy = ty0 - GBL_TP_HALO + i / SW;
            if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
                const int gi = gy * W + gx;
                s_l[i] = cl[gi].w;
                s_z[i] = nz[gi].w;
                s_f[i] = fl[gi];
            } else {
                s_l[i] = s_z[i] = 0.0f;
                s_f[i] = 0u;   // invalid: never counted
            }
        }
        __syncthreads();
    }
    if (x >= W || y >= H) return;
    const int pi = y * W + x;
    const uint32_t fp = fl[pi];
    const float4 zero4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (!(fp & GBL_TP_VALID)) {
        film_out[pi] = zero4;
        if (variance_out) variance_out[pi] = 0.0f;
        hist_out[pi] = hist_out[n + pi] = hist_out[2 * n + pi] = zero4;
        return;
    }
    const float4 cp = cl[pi], np = nz[pi];
    const bool surf = (fp & GBL_TP_SURF) != 0u;
    const float l = cp.w, z = np.w;

    // ---- reproject and gather
    float ws = 0.0f, pr = 0.0f, pg = 0.0f, pb = 0.0f, pN = 0.0f, pm1 = 0.0f, pm2 = 0.0f, pv = 0.0f;
    if (a.has_history && surf) {
        float image_x, image_y, z_exp;
        bool front;
        F3 nt = f3(np.x, np.y, np.z);   // the normal the taps are tested against
        if constexpr (MOTION) {
            const float4 m0 = motion[pi];
            image_x = m0.x;
            image_y = m0.y;
            z_exp = m0.z;
            front = m0.w != 0.0f;
            if (a.has_normal) {
                const float4 m1 = motion[n + pi];
                nt = f3(m1.x, m1.y, m1.z);
            }
        } else {
            F3 o, d;
            tp_camera_ray(a.cur, static_cast<float>(x) + 0.5f, static_cast<float>(y) + 0.5f, &o, &d);
            front = tp_project(a.prev, o + d * z, W, H, &image_x, &image_y, &z_exp);
        }
        const float fx = image_x - 0.5f, fy = image_y - 0.5f;
        const float x0f = floorf(fx), y0f = floorf(fy);
        // the float compares keep the conversion to int defined; taps of a footprint beyond them lie outside the image anyway
        if (front && tp_finite(fx) && tp_finite(fy) && tp_finite(z_exp) && x0f >= -1.0f && x0f < static_cast<float>(W) && y0f >= -1.0f &&
            y0f < static_cast<float>(H)) {
            const float tx = fx - x0f, ty = fy - y0f;
            const int x0 = static_cast<int>(x0f), y0 = static_cast<int>(y0f);
            const float ztol = a.sigma_depth * z_exp;
            for (int j = 0; j < 2; ++j)
                for (int i = 0; i < 2; ++i) {
                    const int qx = x0 + i, qy = y0 + j;
                    if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                    const int qi = qy * W + qx;
                    const float4 h0 = hist_in[qi];
                    if (!(h0.w > 0.0f)) continue;
                    const float4 h2 = hist_in[2 * n + qi];
                    if (!(h2.w != 0.0f)) continue;
                    const float4 h1 = hist_in[n + qi];
                    if (!(fabsf(h1.w - z_exp) <= ztol)) continue;
                    if (a.has_normal && !((nt.x * h2.x + nt.y * h2.y) + nt.z * h2.z >= a.cos_normal)) continue;
                    const float b = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty);
                    ws += b;
                    pr += b * h0.x;
                    pg += b * h0.y;
                    pb += b * h0.z;
                    pN += b * h0.w;
                    pm1 += b * h1.x;
                    pm2 += b * h1.y;
                    pv += b * h1.z;
                }
        }
    }

    // ---- blend
    float N = 1.0f, alpha = 1.0f, cr = cp.x, cg = cp.y, cb = cp.z, m1 = l, m2 = l * l, v_prev = 0.0f;
    const bool history = ws > 0.0f;
    if (history) {
        pr = pr / ws;
        pg = pg / ws;
        pb = pb / ws;
        pN = pN / ws;
        pm1 = pm1 / ws;
        pm2 = pm2 / ws;
        v_prev = pv / ws;
        N = fminf(pN + 1.0f, a.max_history);
        alpha = fmaxf(1.0f / N, a.alpha_min);
        cr = pr + alpha * (cp.x - pr);
        cg = pg + alpha * (cp.y - pg);
        cb = pb + alpha * (cp.z - pb);
        m1 = pm1 + alpha * (l - pm1);
        m2 = pm2 + alpha * (l * l - pm2);
    }

    // ---- variance of the accumulated pixel
    float v_out;
    if (!SPATIAL) {
        const float v_cur = variance[pi];
        const float ia = 1.0f - alpha;
        v_out = history ? (alpha * alpha) * v_cur + (ia * ia) * v_prev : v_cur;
    } else {
        float s2;
        if (N >= 4.0f) {
            s2 = fmaxf(0.0f, m2 - m1 * m1);
        } else {
            const float ztol = a.sigma_depth * z;
            const int base = (ly + GBL_TP_HALO) * SW + (lx + GBL_TP_HALO);
            auto counts = [&](int qi) {
                const uint32_t fq = s_f[qi];
                if (!(fq & GBL_TP_VALID) || ((fq ^ fp) & GBL_TP_SURF)) return false;
                return !surf || fabsf(s_z[qi] - z) <= ztol;
            };
            float sum = 0.0f;
            int m = 0;
            for (int dy = -GBL_TP_HALO; dy <= GBL_TP_HALO; ++dy)
                for (int dx = -GBL_TP_HALO; dx <= GBL_TP_HALO; ++dx) {
                    const int qi = base + dy * SW + dx;
                    if (!counts(qi)) continue;
                    sum += s_l[qi];
                    ++m;
                }
            s2 = 0.0f;
            if (m >= 2) {
                const float mf = static_cast<float>(m), mean = sum / mf;
                float ss = 0.0f;
                for (int dy = -GBL_TP_HALO; dy <= GBL_TP_HALO; ++dy)
                    for (int dx = -GBL_TP_HALO; dx <= GBL_TP_HALO; ++dx) {
                        const int qi = base + dy * SW + dx;
                        if (!counts(qi)) continue;
                        const float dl = s_l[qi] - mean;
                        ss += dl * dl;
                    }
                s2 = ss / (mf - 1.0f);
            }
        }
        v_out = s2 / N;
    }

    film_out[pi] = make_float4(cr, cg, cb, 1.0f);
    if (variance_out) variance_out[pi] = v_out;
    hist_out[pi] = make_float4(cr, cg, cb, N);
    hist_out[n + pi] = make_float4(m1, m2, v_out, z);
    hist_out[2 * n + pi] = make_float4(np.x, np.y, np.z, surf ? 1.0f : 0.0f);
}

template <bool SPATIAL>
__global__ __launch_bounds__(GBL_TP_TILE_W * GBL_TP_TILE_H) void temporal_accumulate_kernel(
    const float4* __restrict__ cl, const float4* __restrict__ nz, const uint32_t* __restrict__ fl, const float* __restrict__ variance,
    const float4* __restrict__ hist_in, float4* __restrict__ hist_out, float4* __restrict__ film_out, float* __restrict__ variance_out, TemporalArgs a) {
    tp_accumulate<SPATIAL, false>(cl, nz, fl, variance, hist_in, hist_out, film_out, variance_out, nullptr, a);
}
// ... and with the reprojection read from gbl_render_motion's planes (instantiated in kernels_motion.hip)
template <bool SPATIAL>
__global__ __launch_bounds__(GBL_TP_TILE_W * GBL_TP_TILE_H) void temporal_accumulate_motion_kernel(
    const float4* __restrict__ cl, const float4* __restrict__ nz, const uint32_t* __restrict__ fl, const float* __restrict__ variance,
    const float4* __restrict__ hist_in, float4* __restrict__ hist_out, float4* __restrict__ film_out, float* __restrict__ variance_out,
    const float4* __restrict__ motion, TemporalArgs a) {
    tp_accumulate<SPATIAL, true>(cl, nz, fl, variance, hist_in, hist_out, film_out, variance_out, motion, a);
}
