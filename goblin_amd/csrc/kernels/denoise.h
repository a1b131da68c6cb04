// gbl_film_variance and gbl_film_denoise: the variance of the pixel mean from per-sample radiance, and an
// edge-avoiding a-trous wavelet filter guided by it and by the first-hit films.  Plain IEEE single arithmetic in the order
// written here (this unit is built with -ffp-contract=off); the exponential is gbl_expf.  tests/denoise_reference.py restates
// every operation below in numpy, in the same order.
//
// Passes of one gbl_film_denoise call, all on one stream:
//   denoise_prepare_kernel   resolves the films once and packs, per pixel, three float4 planes
//                               cv = {c.rgb / d, v / lum(d)^2}     the filtered signal and its variance (ping-pong)
//                               nz = {n.xyz, z}                    unit normal (or 0) and depth
//                               af = {a.rgb, flags}                albedo; flags (integer bits) = VALID | SURF << 1
//                            so that a tap costs three 16-byte loads and no division, and no guide is resolved again
//   denoise_level_kernel     one a-trous level at stride s: 32 x 8 pixel tiles, one lane per pixel, the 3 x 3 variance
//                            prefilter fused.  Built two ways: LDS = true stages the tile and its halo of 2 s pixels of all
//                            three planes in LDS once (every staged pixel is bounds-checked against the image; a pixel outside it
//                            is staged as invalid) and taps with 16-byte LDS reads -- consecutive lanes read consecutive
//                            16-byte slots, which ds_read_b128 serves without bank conflicts; LDS = false takes every tap from
//                            global memory, bounds-checked.  Both run the same arithmetic in the same order.
//   denoise_finish_kernel    film_out = {c * d, 1} for a valid pixel, zeros for an invalid one
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "refmath.h"
#include "denoise_args.h"

__device__ __forceinline__ float dn_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
__device__ __forceinline__ bool dn_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// variance_out of one window pixel per lane: two sums over k = 0 .. S-1, in that order
__global__ void film_variance_kernel(const float4* __restrict__ li, float* __restrict__ variance, int wx0, int wy0, int ww, int wh, int S, int W, int H) {
    const long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= static_cast<long long>(ww) * wh) return;
    const int x = wx0 + static_cast<int>(i % ww), y = wy0 + static_cast<int>(i / ww);
    if (x < 0 || x >= W || y < 0 || y >= H) return;
    const float4* s = li + i * S;
    float sum = 0.0f;
    int m = 0;
    for (int k = 0; k < S; ++k) {
        const float4 L = s[k];
        const float l = dn_lum(L.x, L.y, L.z);
        if (dn_finite(l)) {
            sum += l;
            ++m;
        }
    }
    float var = 0.0f;
    if (m >= 2) {
        const float mf = static_cast<float>(m), mean = sum / mf;
        float ss = 0.0f;
        for (int k = 0; k < S; ++k) {
            const float4 L = s[k];
            const float l = dn_lum(L.x, L.y, L.z);
            if (dn_finite(l)) {
                const float d = l - mean;
                ss += d * d;
            }
        }
        var = ss / (mf * (mf - 1.0f));
    }
    variance[static_cast<long long>(y) * W + x] = var;
}

// d of a pixel: its albedo per channel where the pixel is covered and the channel is at least 1e-2, otherwise 1 (emitters
// with black albedo, the background); 1 with demodulation off
__device__ __forceinline__ float dn_demod(float a, bool surf, uint32_t demodulate) { return (demodulate && surf && a >= 1e-2f) ? a : 1.0f; }

__global__ void denoise_prepare_kernel(const float4* __restrict__ film, const float* __restrict__ variance, const float4* __restrict__ albedo,
                                       const float4* __restrict__ normal, const float4* __restrict__ depth, float4* __restrict__ cv,
                                       float4* __restrict__ nz, float4* __restrict__ af, int n, uint32_t demodulate) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 F = film[i];
    const float inv = 1.0f / F.w;
    float cr = F.x * inv, cg = F.y * inv, cb = F.z * inv;
    float ar = 0.0f, ag = 0.0f, ab = 0.0f;
    if (albedo) {
        const float4 A = albedo[i];
        if (A.w != 0.0f) {
            const float ia = 1.0f / A.w;
            ar = A.x * ia;
            ag = A.y * ia;
            ab = A.z * ia;
        }
    }
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
    float z = 0.0f, coverage = 1.0f;   // no depth film: every pixel counts as covered
    if (depth) {
        const float4 D = depth[i];
        z = D.y != 0.0f ? D.x / D.y : 0.0f;
        coverage = D.w != 0.0f ? D.y / D.w : 0.0f;
    }
    const bool surf = coverage > 0.0f;
    const float dr = dn_demod(ar, surf, demodulate), dg = dn_demod(ag, surf, demodulate), db = dn_demod(ab, surf, demodulate);
    cr = cr / dr;
    cg = cg / dg;
    cb = cb / db;
    float v = 0.0f;
    if (variance) {
        const float ld = dn_lum(dr, dg, db);
        v = variance[i] / (ld * ld);
    }
    const bool valid = F.w > 0.0f && dn_finite(cr) && dn_finite(cg) && dn_finite(cb) && dn_finite(ar) && dn_finite(ag) && dn_finite(ab) &&
                       dn_finite(nx) && dn_finite(ny) && dn_finite(nzz) && dn_finite(z) && dn_finite(v);
    const uint32_t flags = (valid ? GBL_DN_VALID : 0u) | (surf ? GBL_DN_SURF : 0u);
    cv[i] = make_float4(cr, cg, cb, v);
    nz[i] = make_float4(nx, ny, nzz, z);
    af[i] = make_float4(ar, ag, ab, __uint_as_float(flags));
}

// One level.  Per valid pixel p:
//   g      3 x 3 Gaussian (1/4 1/2 1/4 in each direction) of v over the valid neighbours inside the image, dy outer and dx inner,
//          divided by the sum of the weights used;  sd = sqrtf(g), 1 without a variance plane;  inv_l = 1 / (sigma_l * sd + 1e-6f)
//   taps   dy = -2 .. 2 (outer), dx = -2 .. 2 (inner), q = p + s (dx, dy); skipped outside the image, at an invalid q, and where
//          q and p differ in SURF.  h = k[|dx|] * k[|dy|], k = {3/8, 1/4, 1/16};  e = |lum(c_q) - lum(c_p)| * inv_l;  on a
//          covered p  g2 = (|n_q - n_p|^2 * inv_sn2 + |z_q - z_p| * inv_z) + |a_q - a_p|^2 * inv_sa2  with
//          inv_z = 1 / (sz * max(|z_p|, 1e-6f)) (0 without a depth film) and squared lengths (x^2 + y^2) + z^2, else g2 = 0;
//          wt = h * gbl_expf(-(e + g2));  sum += wt * c_q, ws += wt, sv += (wt * wt) * v_q
//   out    c_p = sum / ws, v_p = sv / (ws * ws)       (the centre tap keeps ws > 0)
// An invalid pixel is copied through.
template <bool LDS>
__global__ __launch_bounds__(GBL_DN_TILE_W * GBL_DN_TILE_H) void denoise_level_kernel(const float4* __restrict__ cv_in, const float4* __restrict__ nz,
                                                                                     const float4* __restrict__ af, float4* __restrict__ cv_out,
                                                                                     DenoiseArgs a) {
    extern __shared__ __align__(16) unsigned char dn_smem[];
    const int W = a.W, H = a.H, s = a.stride;
    const int lx = threadIdx.x % GBL_DN_TILE_W, ly = threadIdx.x / GBL_DN_TILE_W;
    const int tx0 = blockIdx.x * GBL_DN_TILE_W, ty0 = blockIdx.y * GBL_DN_TILE_H;
    const int x = tx0 + lx, y = ty0 + ly;
    const int halo = 2 * s, SW = GBL_DN_TILE_W + 2 * halo, SH = GBL_DN_TILE_H + 2 * halo;
    float4* const s_cv = reinterpret_cast<float4*>(dn_smem);
    float4* const s_nz = s_cv + (LDS ? SW * SH : 0);
    float4* const s_af = s_nz + (LDS ? SW * SH : 0);
    if (LDS) {
        for (int i = threadIdx.x; i < SW * SH; i += GBL_DN_TILE_W * GBL_DN_TILE_H) {
            const int gx = tx0 - halo + i % SW, gy = ty0 - halo + i / SW;
            if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
                const int gi = gy * W + gx;
                s_cv[i] = cv_in[gi];
                s_nz[i] = nz[gi];
                s_af[i] = af[gi];
            } else {
                s_cv[i] = s_nz[i] = s_af[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);   // flags 0: invalid, never tapped
            }
        }
        __syncthreads();
    }
    if (x >= W || y >= H) return;
    // a pixel at offset (ox, oy) from p: `in` says whether it lies inside the image (the staged copy carries that in its flags)
    auto index = [&](int ox, int oy, bool& in) -> int {
        if (LDS) {
            in = true;
            return (ly + halo + oy) * SW + (lx + halo + ox);
        }
        const int qx = x + ox, qy = y + oy;
        in = qx >= 0 && qx < W && qy >= 0 && qy < H;
        return qy * W + qx;
    };
    const float4* const p_cv = LDS ? s_cv : cv_in;
    const float4* const p_nz = LDS ? s_nz : nz;
    const float4* const p_af = LDS ? s_af : af;
    bool in;
    const int pi = index(0, 0, in);
    const float4 cp = p_cv[pi], ap = p_af[pi];
    const uint32_t fp = __float_as_uint(ap.w);
    const int out = y * W + x;
    if (!(fp & GBL_DN_VALID)) {
        cv_out[out] = cp;
        return;
    }
    const float4 np = p_nz[pi];
    float sd = 1.0f;
    if (a.has_var) {
        float gs = 0.0f, gw = 0.0f;
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const int qi = index(dx, dy, in);
                if (!in) continue;
                if (!(__float_as_uint(p_af[qi].w) & GBL_DN_VALID)) continue;
                const float kw = (dx == 0 ? 0.5f : 0.25f) * (dy == 0 ? 0.5f : 0.25f);
                gs += kw * p_cv[qi].w;
                gw += kw;
            }
        sd = sqrtf(gs / gw);
    }
    const float inv_l = 1.0f / (a.sigma_l * sd + 1e-6f);
    const bool surf_p = (fp & GBL_DN_SURF) != 0u;
    const float inv_z = a.sz > 0.0f ? 1.0f / (a.sz * fmaxf(fabsf(np.w), 1e-6f)) : 0.0f;
    const float lum_p = dn_lum(cp.x, cp.y, cp.z);
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, ws = 0.0f, sv = 0.0f;
    for (int dy = -2; dy <= 2; ++dy) {
        const float ky = dy == 0 ? 0.375f : ((dy == 1 || dy == -1) ? 0.25f : 0.0625f);
        for (int dx = -2; dx <= 2; ++dx) {
            const int qi = index(s * dx, s * dy, in);
            if (!in) continue;
            const float4 aq = p_af[qi];
            const uint32_t fq = __float_as_uint(aq.w);
            if (!(fq & GBL_DN_VALID) || ((fq ^ fp) & GBL_DN_SURF)) continue;
            const float4 cq = p_cv[qi];
            const float kx = dx == 0 ? 0.375f : ((dx == 1 || dx == -1) ? 0.25f : 0.0625f);
            const float h = kx * ky;
            const float e = fabsf(dn_lum(cq.x, cq.y, cq.z) - lum_p) * inv_l;
            float g2 = 0.0f;
            if (surf_p) {
                const float4 nq = p_nz[qi];
                const float dnx = nq.x - np.x, dny = nq.y - np.y, dnz = nq.z - np.z;
                const float dax = aq.x - ap.x, day = aq.y - ap.y, daz = aq.z - ap.z;
                g2 = (((dnx * dnx + dny * dny) + dnz * dnz) * a.inv_sn2 + fabsf(nq.w - np.w) * inv_z) + ((dax * dax + day * day) + daz * daz) * a.inv_sa2;
            }
            const float wt = h * gbl_expf(-(e + g2));
            sr += wt * cq.x;
            sg += wt * cq.y;
            sb += wt * cq.z;
            ws += wt;
            sv += (wt * wt) * cq.w;
        }
    }
    cv_out[out] = make_float4(sr / ws, sg / ws, sb / ws, sv / (ws * ws));
}

__global__ void denoise_finish_kernel(const float4* __restrict__ cv, const float4* __restrict__ af, float4* __restrict__ film_out, int n, uint32_t demodulate) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 a = af[i];
    const uint32_t f = __float_as_uint(a.w);
    if (!(f & GBL_DN_VALID)) {
        film_out[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const float4 c = cv[i];
    const bool surf = (f & GBL_DN_SURF) != 0u;
    film_out[i] = make_float4(c.x * dn_demod(a.x, surf, demodulate), c.y * dn_demod(a.y, surf, demodulate), c.z * dn_demod(a.z, surf, demodulate), 1.0f);
}
