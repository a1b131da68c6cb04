// gbl_render_motion: per image pixel, where the surface point under the pixel's centre lay in the previous frame
// -- under the previous camera and, for an instance that moved, under the instance's previous transform -- and the current
// normal carried back there.  What gbl_film_accumulate_motion (temporal.h, MOTION) reads in place of its own reprojection.
//
// One wave per 8 x 8 pixel tile, one lane per pixel; the lanes of a tile at the image's edge that lie outside it carry no ray
// and store nothing.  The ray is tp_camera_ray's through (x + 0.5f, y + 0.5f) and the query gbl_render_aov's for a camera ray
// without exact_ties: unfiltered closest hit from the camera's mint.
//   motion_packet_kernel   lean scenes with stack_entries <= GBL_PACKET_STACK: the tile's 64 rays as one packet (packet.h), a ray
//                          whose answer depends on the visiting order traced again on its own, as aov_packet_kernel<false> does
//   motion_kernel<EXT>     one ray per lane with the LDS stack: the EXT scenes (shapes, masks, thin-lens or orthographic context
//                          camera) and, EXT = false, lean scenes whose tree is too deep for the packet's stack
// Planes (W * H float4 each): M0 = {image_x, image_y, z_exp, ok}, all zero unless ok; M1 = {n_b.xyz, instance + 1 or 0}.
// Plain IEEE single arithmetic in the order written (-ffp-contract=off), the projection being temporal.h's tp_project itself.
#pragma once
#include "motion_args.h"
#include "packet.h"
#include "temporal.h"

// Pixel (x, y) of the image, which the caller has checked to lie inside it: the two texels of the pixel.
__device__ __forceinline__ void mo_write(const DevScene& sc, const MotionArgs& a, int x, int y, bool got, const Hit& hit, F3 o, F3 d) {
    const int n = a.W * a.H, pi = y * a.W + x;
    F3 nn = f3(0.0f, 0.0f, 0.0f);
    if (a.normal) {   // temporal_prepare_kernel's rule
        const float4 N = a.normal[pi];
        if (N.w != 0.0f) {
            const float in = 1.0f / N.w;
            nn = f3(N.x * in, N.y * in, N.z * in);
        }
        const float len = sqrtf((nn.x * nn.x + nn.y * nn.y) + nn.z * nn.z);
        nn = len > 0.0f ? f3(nn.x / len, nn.y / len, nn.z / len) : f3(0.0f, 0.0f, 0.0f);
    }
    float4 m0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    F3 nb = nn;
    float id = 0.0f;
    if (got) {
        const int i = hit.inst;
        F3 P = o + d * hit.t;
        if (a.moved != nullptr && a.moved[i] != 0u) {
            const DevInstance* ip = sc.instances + i;
            const float* pm = a.prev_xf + static_cast<size_t>(GBL_MOTION_XF_FLOATS) * static_cast<size_t>(i);
            P = xf_point(pm, xf_point(ip->inv, P));
            if (a.normal) {   // the inverse transpose, as Fragment::transform carries a normal: to object space by M_cur, on by Minv_prev
                const F3 u = xf_normal(pm + 12, xf_normal(ip->m, nn));
                const float len = sqrtf((u.x * u.x + u.y * u.y) + u.z * u.z);
                nb = len > 0.0f ? f3(u.x / len, u.y / len, u.z / len) : f3(0.0f, 0.0f, 0.0f);
            }
        }
        float image_x, image_y, z_exp;
        const bool front = tp_project(a.prev, P, a.W, a.H, &image_x, &image_y, &z_exp);
        if (front && tp_finite(image_x) && tp_finite(image_y) && tp_finite(z_exp)) m0 = make_float4(image_x, image_y, z_exp, 1.0f);
        id = static_cast<float>(i + 1);
    }
    a.out[pi] = m0;
    a.out[n + pi] = make_float4(nb.x, nb.y, nb.z, id);
}

// The tile and pixel of this lane; false for a wave past the last tile
__device__ __forceinline__ bool mo_pixel(const MotionArgs& a, int* x, int* y) {
    const int tiles_x = (a.W + GBL_TILE - 1) / GBL_TILE, tiles_y = (a.H + GBL_TILE - 1) / GBL_TILE;
    const int tile = static_cast<int>(blockIdx.x) * (GBL_BLOCK / 64) + static_cast<int>(threadIdx.x >> 6);
    if (tile >= tiles_x * tiles_y) return false;
    const int lane = static_cast<int>(threadIdx.x & 63u);
    *x = (tile % tiles_x) * GBL_TILE + (lane & (GBL_TILE - 1));
    *y = (tile / tiles_x) * GBL_TILE + lane / GBL_TILE;
    return true;
}
__device__ __forceinline__ float mo_mint(const DevCamera& c) { return c.type == 1u ? 0.0f : 1e-3f; }   // render_kernels.h camera_ray

// LDS: the waves' shared stacks (static) and the lanes' own for the retraces (dynamic, stack_lds_bytes), as aov_packet_kernel
__global__ __launch_bounds__(GBL_BLOCK) void motion_packet_kernel(DevScene sc, MotionArgs a) {
    __shared__ uint32_t pk_stack[(GBL_BLOCK / 64) * GBL_PACKET_STACK_WORDS];
    extern __shared__ __align__(16) unsigned char smem[];
    gbl_lds_u32* const wstack = gbl_as_lds(pk_stack + (threadIdx.x >> 6) * GBL_PACKET_STACK_WORDS);
    const LdsStack stk = {gbl_as_lds(reinterpret_cast<uint32_t*>(smem) + threadIdx.x)};
    int x, y;
    if (!mo_pixel(a, &x, &y)) return;   // (wave-uniform)
    const bool live = x < a.W && y < a.H;
    F3 o, d;
    tp_camera_ray(sc.camera, static_cast<float>(x) + 0.5f, static_cast<float>(y) + 0.5f, &o, &d);
    const float mint = mo_mint(sc.camera);
    Hit hit;
    bool tied;
    bool got = packet_closest(sc, live, o, d, mint, wstack, hit, tied);
    if (live && tied) {
        LaneCounters scratch = {};
        got = trace<false, false, false, false>(sc, o, d, mint, INFINITY, stk, hit, scratch);
    }
    if (live) mo_write(sc, a, x, y, got, hit, o, d);
}

template <bool EXT>
__global__ __launch_bounds__(GBL_BLOCK, EXT ? 2 : 4) void motion_kernel(DevScene sc, MotionArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const LdsStack stk = {gbl_as_lds(reinterpret_cast<uint32_t*>(smem) + threadIdx.x)};
    int x, y;
    if (!mo_pixel(a, &x, &y)) return;
    if (x >= a.W || y >= a.H) return;
    F3 o, d;
    tp_camera_ray(sc.camera, static_cast<float>(x) + 0.5f, static_cast<float>(y) + 0.5f, &o, &d);
    Hit hit;
    LaneCounters cnt = {};
    const bool got = trace<false, false, EXT, false>(sc, o, d, mo_mint(sc.camera), INFINITY, stk, hit, cnt);
    mo_write(sc, a, x, y, got, hit, o, d);
}
