// An image based light's tables made again on the device after its image changed (gbl_update_environment*, api_environment.hip):
// what scene_prep.cpp's pack_ibl_distribution, attach_ibl_texels and pack_light_distribution pack on the host at gbl_create,
// behind the pyramid launches (kernels/pyramid.h) on the same stream.
//
// The tables must equal the host's bit for bit, so every sum keeps the host's order and operations (the unit is built with
// -ffp-contract=off, and a float divide is the correctly rounded one):
//   func      luminance(rgb) * sin_theta[r], luminance = 0.212671f * r + 0.715160f * g + 0.072169f * b from the left; the sine
//             table is the host's (scene_prep.h ibl_sin_theta), made with the loader's sinf
//   cdf1d     cdf[0] = 0, cdf[k] = cdf[k - 1] + f[k - 1] * dx with dx = 1.0f / n, integral = cdf[n], then cdf[k] /= integral for
//             k >= 1.  The recurrence is serial by definition -- float adds do not reassociate -- so one lane owns one row and
//             walks it; the divides have no order and run over all lanes
//   average   the bilinear lookup of the 1 x 1 level at (-0.5, -0.5) under repeat: four taps of the one texel, each weighted
//             0.5f * 0.5f, added from the left
//   power     luminance of avg * pi * (4 pi r^2), each channel multiplied in that order; then cdf1d over the lights' powers and
//             pick_pdf[i] = (power[i] / integral) * dx
//
// The distribution is at most 256 x 256 (the level is chosen so), the lights are few: three small launches, whose cost is the
// serial walks' latency, not bandwidth.  A 4-channel pyramid may start at a float offset that is no multiple of four
// (device_scene.h), so texels are read float by float.
#pragma once
#include "../device_scene.h"
#include "vecmath.h"
#include "environment_args.h"

#define GBL_ENV_ROWS 64    // rows of the distribution per workgroup of environment_rows: one lane of its first wave per row
#define GBL_ENV_TAIL 256   // threads of environment_tail: one per row of the largest distribution

__device__ __forceinline__ float environment_luminance(float r, float g, float b) { return 0.212671f * r + 0.715160f * g + 0.072169f * b; }

// The rows' blocks start behind the marginal block; each is func[dw], cdf[dw + 1], integral
__device__ __forceinline__ float* environment_row(const EnvironmentArgs& a, uint32_t r) {
    return a.dist + (2u * a.dh + 2u) + static_cast<size_t>(r) * (2u * a.dw + 2u);
}

// func of every row: one thread per texel of the distribution's level
__global__ __launch_bounds__(GBL_BLOCK) void environment_func(EnvironmentArgs a) {
    const uint32_t k = blockIdx.x * GBL_BLOCK + threadIdx.x;
    if (k >= a.dw * a.dh) return;
    const uint32_t r = k / a.dw, c = k - r * a.dw;
    const float* p = a.level + static_cast<size_t>(k) * 4;
    environment_row(a, r)[c] = environment_luminance(p[0], p[1], p[2]) * a.sin_theta[r];
}

// cdf and integral of every row.  A workgroup takes GBL_ENV_ROWS rows and stages them through LDS in tiles of 64 columns: its
// four waves load the tile row by row, consecutive lanes on consecutive columns, so the global loads cover whole lines; then lane
// r of the first wave walks row r of the tile (rows 65 floats apart: the lanes of a half wave fall on 32 different banks) and
// leaves the running sum in place of each value; the four waves store the tile as they loaded it.  The divides follow, again row
// by row with the lanes over the columns.
__global__ __launch_bounds__(GBL_BLOCK) void environment_rows(EnvironmentArgs a) {
    __shared__ float tile[GBL_ENV_ROWS][GBL_ENV_ROWS + 1];
    __shared__ float integral[GBL_ENV_ROWS];
    const uint32_t lane = threadIdx.x % GBL_ENV_ROWS, wave = threadIdx.x / GBL_ENV_ROWS, waves = GBL_BLOCK / GBL_ENV_ROWS;
    const uint32_t row0 = blockIdx.x * GBL_ENV_ROWS, n = a.dw;
    const uint32_t rows = min(static_cast<uint32_t>(GBL_ENV_ROWS), a.dh - row0);
    const bool walks = wave == 0 && lane < rows;
    const size_t stride = 2u * n + 2u;
    float* const base = environment_row(a, row0);
    const float dx = 1.0f / static_cast<float>(n);
    float cdf = 0.0f;
    for (uint32_t c0 = 0; c0 < n; c0 += GBL_ENV_ROWS) {
        const uint32_t cols = min(static_cast<uint32_t>(GBL_ENV_ROWS), n - c0);
        if (lane < cols)
            for (uint32_t i = wave; i < rows; i += waves) tile[i][lane] = base[i * stride + c0 + lane];
        __syncthreads();
        if (walks)
            for (uint32_t k = 0; k < cols; ++k) {
                cdf = cdf + tile[lane][k] * dx;
                tile[lane][k] = cdf;
            }
        __syncthreads();
        if (lane < cols)
            for (uint32_t i = wave; i < rows; i += waves) base[i * stride + n + 1u + c0 + lane] = tile[i][lane];
        __syncthreads();
    }
    if (walks) {
        integral[lane] = cdf;
        base[lane * stride + n] = 0.0f;          // cdf[0]
        base[lane * stride + 2u * n + 1u] = cdf;
    }
    __syncthreads();   // ... which also orders the tiles' stores before the loads below, within the workgroup
    for (uint32_t i = wave; i < rows; i += waves) {
        const float total = integral[i];
        for (uint32_t k = lane; k < n; k += GBL_ENV_ROWS) {
            float* const p = base + i * stride + n + 1u + k;
            *p = *p / total;
        }
    }
}

// The rest, one workgroup: the marginal block over the row integrals, the average radiance and the power, then the lights' pick
// distribution over the powers with this light's replaced.  Thread 0 walks the two serial sums; the divides take all threads.
__global__ __launch_bounds__(GBL_ENV_TAIL) void environment_tail(EnvironmentArgs a) {
    __shared__ float f[GBL_ENV_TAIL], cdf[GBL_ENV_TAIL + 1], total[2];
    const uint32_t t = threadIdx.x, n = a.dh, lights = a.num_lights;
    if (t < n) {
        f[t] = environment_row(a, t)[2u * a.dw + 1u];
        a.dist[t] = f[t];
    }
    __syncthreads();
    const float dxl = 1.0f / static_cast<float>(lights);
    if (t == 0) {
        const float dx = 1.0f / static_cast<float>(n);
        float c = 0.0f;
        cdf[0] = 0.0f;
        for (uint32_t k = 0; k < n; ++k) {
            c = c + f[k] * dx;
            cdf[k + 1] = c;
        }
        total[0] = c;
        a.dist[n] = 0.0f;
        a.dist[2u * n + 1u] = c;
        // attach_ibl_texels: ds = dt = 0.5f, every tap is the one texel
        const float w = 0.5f * 0.5f;
        float p[3];
        for (int ch = 0; ch < 3; ++ch) {
            const float texel = a.top[ch];
            const float avg = w * texel + w * texel + w * texel + w * texel;
            p[ch] = avg * GBL_PI * a.sphere_area;
        }
        a.power[a.light] = environment_luminance(p[0], p[1], p[2]);
        // pack_light_distribution
        c = 0.0f;
        a.light_cdf[0] = 0.0f;
        for (uint32_t k = 0; k < lights; ++k) {
            c = c + a.power[k] * dxl;
            a.light_cdf[k + 1] = c;
        }
        total[1] = c;
    }
    __syncthreads();   // (thread 0's global stores are the workgroup's own: the loads below see them)
    if (t < n) a.dist[n + 1u + t] = cdf[t + 1] / total[0];
    for (uint32_t k = t; k < lights; k += GBL_ENV_TAIL) {
        a.light_cdf[k + 1] = a.light_cdf[k + 1] / total[1];
        a.light_pick_pdf[k] = (a.power[k] / total[1]) * dxl;
    }
}
