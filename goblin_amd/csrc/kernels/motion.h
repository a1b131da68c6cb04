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
//   motion_packet_deform_kernel, motion_deform_kernel<EXT>   the same three for gbl_render_motion_deform when some mesh is
//                          deformed (mo_write<true>): a hit of such a mesh is followed through the triangle's previous pose
// Planes (W * H float4 each): M0 = {image_x, image_y, z_exp, ok}, all zero unless ok; M1 = {n_b.xyz, instance + 1 or 0}.
// Plain IEEE single arithmetic in the order written (-ffp-contract=off), the projection being temporal.h's tp_project itself.
#pragma once
#include "motion_args.h"
#include "packet.h"
#include "temporal.h"

// gbl_render_motion_deform's hit of instance `ip` of a deformed triangle mesh (`off`: the mesh's entry of MotionArgs::mesh_prev):
// the hit's barycentrics on the triangle's previous pose, taken to the previous frame's world by `m` -- the instance's previous
// toWorld rows if it moved, else its current ones -- and, with a normal film, the normal carried by the inverse transpose of the
// triangle's own deformation between `u = xf_normal(ip->m, nn)` and `inv`, the inverse rows that go with `m`.  False, and nothing
// written, for a vertex outside the packed positions (the host's tables never hold one).
__device__ __forceinline__ bool mo_deformed(const DevScene& sc, const MotionArgs& a, const Hit& hit, const DevInstance* ip, int32_t off, const float* m,
                                            const float* inv, F3 nn, F3* P, F3* nb) {
    const DevTri* T = sc.tris + hit.tri;
    const DevTriShade s = sc.tri_shade[T->shade];
    F3 v[3];
    for (int k = 0; k < 3; ++k) {
        const int64_t at = static_cast<int64_t>(s.v[k]) + off;
        if (at < 0 || at >= static_cast<int64_t>(a.prev_count)) return false;
        const float* p = a.prev_pos + 3 * static_cast<size_t>(at);
        v[k] = f3(p[0], p[1], p[2]);
    }
    const F3 e1p = v[1] - v[0], e2p = v[2] - v[0];
    *P = xf_point(m, (v[0] + e1p * hit.b1) + e2p * hit.b2);
    if (a.normal) {
        const F3 u = xf_normal(ip->m, nn);
        const F3 e1 = f3(T->e1[0], T->e1[1], T->e1[2]), e2 = f3(T->e2[0], T->e2[1], T->e2[2]);
        const F3 g = cross(e1, e2), gp = cross(e1p, e2p);
        const float L = sqrtf((g.x * g.x + g.y * g.y) + g.z * g.z), Lp = sqrtf((gp.x * gp.x + gp.y * gp.y) + gp.z * gp.z);
        F3 xx = u;   // a triangle without area in either pose: the instance alone carries the normal
        if (L > 0.0f && Lp > 0.0f) {
            const F3 gh = f3(g.x / L, g.y / L, g.z / L), ghp = f3(gp.x / Lp, gp.y / Lp, gp.z / Lp);
            const float c1 = dot(e1, u), c2 = dot(e2, u), c3 = dot(gh, u);
            xx = (cross(e2p, ghp) * (c1 / Lp) + cross(ghp, e1p) * (c2 / Lp)) + ghp * c3;   // e1'.x = c1, e2'.x = c2, g^'.x = c3
        }
        const F3 w = xf_normal(inv, xx);
        const float len = sqrtf((w.x * w.x + w.y * w.y) + w.z * w.z);
        *nb = len > 0.0f ? f3(w.x / len, w.y / len, w.z / len) : f3(0.0f, 0.0f, 0.0f);
    }
    return true;
}

// Pixel (x, y) of the image, which the caller has checked to lie inside it: the two texels of the pixel.  DEFORM: a hit of a
// triangle mesh whose previous pose the call was given goes through mo_deformed; every other hit takes the path below it.
template <bool DEFORM>
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
        bool deformed = false;
        if constexpr (DEFORM) {
            const DevInstance* ip = sc.instances + i;
            const uint32_t mesh = static_cast<uint32_t>(ip->mesh);
            const int32_t off = ip->shape == 0u && mesh < a.num_meshes ? a.mesh_prev[mesh] : GBL_MOTION_STATIC;
            if (off != GBL_MOTION_STATIC) {
                const float* m = ip->m;
                const float* inv = ip->inv;
                if (a.moved != nullptr && a.moved[i] != 0u) {
                    m = a.prev_xf + static_cast<size_t>(GBL_MOTION_XF_FLOATS) * static_cast<size_t>(i);
                    inv = m + 12;
                }
                deformed = mo_deformed(sc, a, hit, ip, off, m, inv, nn, &P, &nb);
            }
        }
        if (!deformed && a.moved != nullptr && a.moved[i] != 0u) {
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
template <bool DEFORM>
__device__ __forceinline__ void motion_packet(const DevScene& sc, const MotionArgs& a) {
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
    if (live) mo_write<DEFORM>(sc, a, x, y, got, hit, o, d);
}

template <bool EXT, bool DEFORM>
__device__ __forceinline__ void motion_lane(const DevScene& sc, const MotionArgs& a) {
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
    mo_write<DEFORM>(sc, a, x, y, got, hit, o, d);
}
template <bool EXT>
__global__ __launch_bounds__(GBL_BLOCK, EXT ? 2 : 4) void motion_kernel(DevScene sc, MotionArgs a) { motion_lane<EXT, false>(sc, a); }
template <bool EXT>
__global__ __launch_bounds__(GBL_BLOCK, EXT ? 2 : 4) void motion_deform_kernel(DevScene sc, MotionArgs a) { motion_lane<EXT, true>(sc, a); }
__global__ __launch_bounds__(GBL_BLOCK) void motion_packet_kernel(DevScene sc, MotionArgs a) { motion_packet<false>(sc, a); }
__global__ __launch_bounds__(GBL_BLOCK) void motion_packet_deform_kernel(DevScene sc, MotionArgs a) { motion_packet<true>(sc, a); }
