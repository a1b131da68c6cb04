// Film::writeImage's tail on the device (gbl_film_develop): Goblin::bloom (GoblinImageIO.cpp:169-218), Goblin::toneMapping
// (:220-236) and writeImagePPM's 8-bit quantisation (:101-127), in the reference's operation order so that the pixels are
// the reference's bit for bit.  Plain IEEE single arithmetic; this unit is built with -ffp-contract=off, and the one
// explicit fused multiply-add below multiplies by exactly 0 or 1, so it rounds like the add alone.
//
// What decides the bits is the order of two sums, and only that:
//   bloom     every output pixel adds w * r, w * g, w * b and w over py ascending (outer) and px ascending (inner).  One
//             pixel's four accumulators live in one lane's registers and that lane walks the window in exactly this order;
//             which lane owns which pixel, the tiling and the staging are free.
//   tone map  the reference adds logf(1e4 + luminance) of all W * H pixels into ONE float, in index order.  The sum is far
//             from associative at image sizes (past 2^24 every addend is rounded to a multiple of 2 or 4), so it is kept
//             serial: one lane adds, the rest of its workgroup only feeds it (tone_sum_kernel).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "refmath.h"

// ---- bloom ---------------------------------------------------------------------------------------------------------
// A workgroup owns GBL_BLOOM_ROWS output rows x GBL_BLOOM_TILE_W output columns: one wave per row, GBL_BLOOM_PX
// horizontally adjacent pixels per lane.  It walks the input rows py in ascending order; each row is cut into chunks of
// GBL_BLOOM_CHUNK window steps so that the LDS it needs is a constant, whatever the filter width:
//   seg    the input pixels {r, g, b, inside-the-image ? 1 : 0} the chunk's steps read, staged once for all rows of the tile
//   frow   per wave: the filter row filter[|py - y|][|k|] over the tap offsets k the chunk reads, 0 where |k| >= fw and
//          at the centre tap (k == 0 in the row py == y), which the reference skips
// At step d a lane reads ONE staged pixel, x + d, and adds it to each of its PX outputs j with the weight of offset d - j:
// every LDS read is used PX times, and for each output the steps come in ascending px.  A tap outside the window or the
// image adds w * 0 or 0 * c = +0 to the colour sums and 0 to the weight sum: for finite pixels that is exactly the
// reference's skipping it (the sums start at +0 and never become -0).  A non-finite pixel spreads NaN over the reference's
// window too (its corner weights are 0); here it also reaches itself and up to PX - 1 more pixels on either side.
#define GBL_BLOOM_PX 4
#define GBL_BLOOM_ROWS 4
#define GBL_BLOOM_TILE_W (64 * GBL_BLOOM_PX)
#define GBL_BLOOM_CHUNK 64   // a multiple of GBL_BLOOM_PX: the weight registers rotate back to their places every PX steps
#define GBL_BLOOM_SEG (GBL_BLOOM_TILE_W - GBL_BLOOM_PX + GBL_BLOOM_CHUNK)   // staged pixels per chunk: lane 63's last step
#define GBL_BLOOM_FROW (GBL_BLOOM_CHUNK + GBL_BLOOM_PX - 1)
// One pixel more after every 16: a lane's step-d pixel is q = PX * lane + d, and ds_read_b128 serves 16 lanes at a time,
// whose 16-byte slots must differ mod 16 (kernels read q + q / 16)
#define GBL_BLOOM_SLOT(q) ((q) + ((q) >> 4))
#define GBL_BLOOM_SEG_SLOTS (GBL_BLOOM_SEG + GBL_BLOOM_SEG / 16 + 1)

// rgb1[i] = {accum.rgb * (1 / accum.w), 1}: the un-bloomed image the blend and every window read (as film_resolve_kernel)
__global__ void develop_resolve_kernel(const float4* accum, float4* rgb1, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 a = accum[i];
    const float inv = 1.0f / a.w;
    rgb1[i] = make_float4(a.x * inv, a.y * inv, a.z * inv, 1.0f);
}

// filter[fy * fwx + fx] = powf(max(0, 1 - sqrtf(fx^2 + fy^2) / fw), 4) for fx < fwx = min(fw, W), fy < fwy = min(fw, H):
// no tap further away lies inside the image
__global__ void bloom_filter_kernel(float* filter, int fw, int fwx, int fwy) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= fwx * fwy) return;
    const int fx = i % fwx, fy = i / fwx;
    const float d = sqrtf(static_cast<float>(fx * fx + fy * fy)) / static_cast<float>(fw);
    filter[i] = gbl_powf(fmaxf(0.0f, 1.0f - d), 4.0f);
}

__global__ __launch_bounds__(64 * GBL_BLOOM_ROWS) void bloom_kernel(const float4* __restrict__ rgb1, const float* __restrict__ filter, float* __restrict__ out,
                                                                     int W, int H, int fw, int fwx, float weight) {
    __shared__ float4 seg[GBL_BLOOM_SEG_SLOTS];
    __shared__ float frow[GBL_BLOOM_ROWS][GBL_BLOOM_FROW + 1];
    const int lane = threadIdx.x & 63, row = threadIdx.x >> 6;
    const int tx0 = blockIdx.x * GBL_BLOOM_TILE_W, ty0 = blockIdx.y * GBL_BLOOM_ROWS;
    const int y = ty0 + row, x = tx0 + lane * GBL_BLOOM_PX;
    float acc[GBL_BLOOM_PX][3], wsum[GBL_BLOOM_PX];
#pragma unroll
    for (int j = 0; j < GBL_BLOOM_PX; ++j) acc[j][0] = acc[j][1] = acc[j][2] = wsum[j] = 0.0f;
    const int py0 = max(0, ty0 - fw + 1), py1 = min(H - 1, ty0 + GBL_BLOOM_ROWS - 1 + fw - 1);
    // the steps of a lane: d = -(fw - 1) .. (PX - 1) + (fw - 1), cut where even lane 0 has left the image on the right
    const int d_lo = -(fw - 1), d_hi = min(GBL_BLOOM_PX - 1 + fw - 1, W - 1 - tx0);
    for (int py = py0; py <= py1; ++py) {
        const int fy = abs(py - y);
        const bool mine = y < H && fy < fw;   // wave-uniform
        for (int dc = d_lo; dc <= d_hi; dc += GBL_BLOOM_CHUNK) {
            // stage: seg[q] = the pixel at column tx0 + dc + q of row py
            for (int q = threadIdx.x; q < GBL_BLOOM_SEG; q += 64 * GBL_BLOOM_ROWS) {
                const int px = tx0 + dc + q;
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (px >= 0 && px < W) v = rgb1[static_cast<size_t>(py) * W + px];
                seg[GBL_BLOOM_SLOT(q)] = v;
            }
            // frow[row][i] = the weight of tap offset k = dc - (PX - 1) + i in this wave's filter row
            if (mine) {
                for (int i = lane; i < GBL_BLOOM_FROW; i += 64) {
                    const int k = dc - (GBL_BLOOM_PX - 1) + i, a = abs(k);
                    float w = 0.0f;
                    if (a < fwx && !(a == 0 && fy == 0)) w = filter[fy * fwx + a];
                    frow[row][i] = w;
                }
            }
            __syncthreads();
            if (mine) {
                const int steps = min(GBL_BLOOM_CHUNK, d_hi - dc + 1);
                // w[j] = weight of offset d - j; entering step d = dc it holds offsets dc - 1 - j for j < PX - 1
                float w[GBL_BLOOM_PX];
#pragma unroll
                for (int j = 0; j < GBL_BLOOM_PX - 1; ++j) w[j] = frow[row][GBL_BLOOM_PX - 2 - j];
                const int q0 = lane * GBL_BLOOM_PX;
                auto step = [&](int s) {   // d = dc + s
#pragma unroll
                    for (int j = GBL_BLOOM_PX - 1; j > 0; --j) w[j] = w[j - 1];
                    w[0] = frow[row][s + GBL_BLOOM_PX - 1];
                    const float4 c = seg[GBL_BLOOM_SLOT(q0 + s)];
#pragma unroll
                    for (int j = 0; j < GBL_BLOOM_PX; ++j) {
                        acc[j][0] += w[j] * c.x;
                        acc[j][1] += w[j] * c.y;
                        acc[j][2] += w[j] * c.z;
                        wsum[j] = __builtin_fmaf(w[j], c.w, wsum[j]);   // c.w is 0 or 1: the product is exact
                    }
                };
                int s = 0;
                for (; s + GBL_BLOOM_PX <= steps; s += GBL_BLOOM_PX) {   // PX steps at a time: the weights are back in their registers
#pragma unroll
                    for (int u = 0; u < GBL_BLOOM_PX; ++u) step(s + u);
                }
                for (; s < steps; ++s) step(s);
            }
            __syncthreads();
        }
    }
    if (y >= H) return;
    const float keep = 1.0f - weight;
#pragma unroll
    for (int j = 0; j < GBL_BLOOM_PX; ++j) {
        if (x + j >= W) break;
        const size_t i = static_cast<size_t>(y) * W + x + j;
        const float4 c = rgb1[i];
        const float inv = 1.0f / wsum[j];   // Color::operator/= multiplies by the reciprocal
        out[3 * i + 0] = keep * c.x + weight * (acc[j][0] * inv);
        out[3 * i + 1] = keep * c.y + weight * (acc[j][1] * inv);
        out[3 * i + 2] = keep * c.z + weight * (acc[j][2] * inv);
    }
}

// ---- tone map ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float develop_luminance(float r, float g, float b) { return 0.212671f * r + 0.715160f * g + 0.072169f * b; }   // GoblinColor.h

__global__ void tone_log_kernel(const float* rgb, float* logs, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    logs[i] = gbl_logf(1e4f + develop_luminance(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]));
}

// The serial sum.  One workgroup: all of it copies chunk k + 1 from memory into registers, lane 0 adds chunk k out of LDS
// in index order, then the registers go to the other LDS buffer.  What it costs is the latency of one dependent add per pixel.  inv_out[0] = 1 / (Ywa * Ywa), Ywa = expf(sum / (W * H)).
#define GBL_TONE_THREADS 256
#define GBL_TONE_CHUNK (GBL_TONE_THREADS * 16)
__global__ __launch_bounds__(GBL_TONE_THREADS) void tone_sum_kernel(const float* __restrict__ logs, int n, float* inv_out) {
    __shared__ float4 buf[2][GBL_TONE_CHUNK / 4];
    const int t = threadIdx.x;
    float4 v[4];
    auto fetch = [&](int base) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = base + 4 * (t + k * GBL_TONE_THREADS);
            float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (i + 3 < n) {
                c = make_float4(logs[i], logs[i + 1], logs[i + 2], logs[i + 3]);
            } else {
                if (i < n) c.x = logs[i];
                if (i + 1 < n) c.y = logs[i + 1];
                if (i + 2 < n) c.z = logs[i + 2];
            }
            v[k] = c;
        }
    };
    auto put = [&](int b) {
#pragma unroll
        for (int k = 0; k < 4; ++k) buf[b][t + k * GBL_TONE_THREADS] = v[k];
    };
    fetch(0);
    put(0);
    __syncthreads();
    float sum = 0.0f;
    int cur = 0;
    for (int base = 0; base < n; base += GBL_TONE_CHUNK) {
        const bool more = base + GBL_TONE_CHUNK < n;
        if (more) fetch(base + GBL_TONE_CHUNK);
        if (t == 0) {
            // 32 values per block, two register sets: the LDS reads of one block are in flight while the other is added, so
            // the chain of dependent adds is all the lane waits for (16 reads outstanding at most: the wait counter's reach)
            const int count = min(GBL_TONE_CHUNK, n - base), blocks = count >> 5;
            const float4* src = buf[cur];
            float4 a[8], b[8];
            auto load = [&](float4 (&r)[8], int blk) {
#pragma unroll
                for (int k = 0; k < 8; ++k) r[k] = src[blk * 8 + k];
                __builtin_amdgcn_sched_barrier(0);   // the reads are issued here, ahead of the other set's adds
            };
            auto add = [&](const float4 (&r)[8]) {
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    sum += r[k].x;
                    sum += r[k].y;
                    sum += r[k].z;
                    sum += r[k].w;
                }
            };
            int blk = 0;
            if (blocks > 0) load(a, 0);
            for (; blk + 2 <= blocks; blk += 2) {
                load(b, blk + 1);
                add(a);
                load(a, min(blk + 2, blocks - 1));   // (past the last block: read again, not added)
                add(b);
            }
            if (blk < blocks) add(a);
            const float* tail = reinterpret_cast<const float*>(src);
            for (int i = blocks << 5; i < count; ++i) sum += tail[i];
        }
        if (more) put(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }
    if (t == 0) {
        const float ywa = gbl_expf(sum / static_cast<float>(n));
        inv_out[0] = 1.0f / (ywa * ywa);
    }
}

__global__ void tone_scale_kernel(float* rgb, const float* inv_in, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float invy2 = inv_in[0];
    const float r = rgb[3 * i], g = rgb[3 * i + 1], b = rgb[3 * i + 2];
    const float y = develop_luminance(r, g, b);
    const float s = (1.0f + y * invy2) / (1.0f + y);
    rgb[3 * i] = r * s;
    rgb[3 * i + 1] = g * s;
    rgb[3 * i + 2] = b * s;
}

// ---- 8 bit ---------------------------------------------------------------------------------------------------------
// writeImagePPM: int(clamp(powf(c, 1 / 2.2f), 0, 1) * 255) per channel; n = W * H * 3
__global__ void quantize_kernel(const float* rgb, uint8_t* rgb8, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float inv_gamma = 1.0f / 2.2f;
    float g = gbl_powf(rgb[i], inv_gamma);
    g = g < 0.0f ? 0.0f : (g > 1.0f ? 1.0f : g);
    rgb8[i] = static_cast<uint8_t>(static_cast<int>(g * 255.0f));
}
