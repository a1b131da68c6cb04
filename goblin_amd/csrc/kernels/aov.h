// aov_kernel: the first-hit features of every camera sample of a call -- albedo, shading normal, depth, position, instance
// (gbl_render_aov).  A first-hit pass over the call's camera samples like sss_kernel (subsurface.h): the camera
// sample is gbl_render's (camera_sample), the query is Scene::intersect as PathTracer::Li issues it for the camera ray
// (GoblinPathtracer.cpp:58-60: unfiltered closest hit, Material::perturb on the fragment, GoblinScene.cpp:75-83), and the
// albedo is the material's first colour slot looked up as the bounce-0 BSDF looks it up, after computeUVDifferential (:77).
// The medium, the lights and max_ray_depth do not enter.
#pragma once
#include "aov_args.h"
#include "packet.h"
#include "render_kernels.h"

// The material's first colour slot: Lambert Kd, Blinn Kg, transparent / mirror Kr (color / tex_color), subsurface Kr (color3 /
// tex_color3); a mask answers with the material it wraps (MaskMaterial forwards its lookups, GoblinMaterial.cpp:747-811).
template <bool EXT>
__device__ __forceinline__ F3 aov_albedo(const DevScene& sc, int material, const Frag& fr, const TexFrag& tf) {
    const DevMaterial* m = sc.materials + material;
    if (EXT && m->type == GBL_MAT_MASK) m = sc.materials + m->masked;
    if (EXT && m->type == GBL_MAT_SUBSURFACE)
        return m->tex_color3 >= 0 ? tex_eval<GBL_TEX_MAX_DEPTH>(sc, m->tex_color3, fr, tf) : f3(m->color3[0], m->color3[1], m->color3[2]);
    if (EXT && m->tex_color >= 0) return tex_eval<GBL_TEX_MAX_DEPTH>(sc, m->tex_color, fr, tf);
    return f3(m->color[0], m->color[1], m->color[2]);
}

// The features of a hit, written to whichever outputs the call asked for.  !got: the camera ray left the scene.
template <bool EXT, bool REPLAY>
__device__ __forceinline__ void aov_write(const DevScene& sc, const AovArgs& aa, const SampleSource& src, bool got, const Hit& hit, F3 o, F3 d, float image_x,
                                          float image_y, size_t plane_index, size_t out_index) {
    F3 albedo = f3(0.0f, 0.0f, 0.0f), n = albedo, p = albedo;
    float t = -1.0f;
    int inst = -1;
    if (got) {
        Frag fr;
        TexFrag tf;
        make_fragment<EXT>(sc, hit, o, d, fr, &tf);
        const int material = sc.instances[hit.inst].material;
        if (EXT && sc.materials[material].has_tex != 0u) hit_differentials<REPLAY>(sc, src, true, image_x, image_y, fr, tf);
        albedo = aov_albedo<EXT>(sc, material, fr, tf);
        n = fr.n;
        p = fr.p;
        t = hit.t;
        inst = hit.inst;
    }
    const float h = got ? 1.0f : 0.0f;
    if (aa.albedo) aa.albedo[plane_index] = make_float4(albedo.x, albedo.y, albedo.z, 0.0f);
    if (aa.normal) aa.normal[plane_index] = make_float4(n.x, n.y, n.z, 0.0f);
    if (aa.depth) aa.depth[plane_index] = make_float4(got ? t : 0.0f, h, 0.0f, 0.0f);
    if (aa.samples) {
        float4* q = reinterpret_cast<float4*>(aa.samples + out_index);   // (48-byte records in a hipMalloc'd array: 16-byte aligned)
        q[0] = make_float4(albedo.x, albedo.y, albedo.z, t);
        q[1] = make_float4(n.x, n.y, n.z, __int_as_float(inst));
        q[2] = make_float4(p.x, p.y, p.z, __uint_as_float(got ? 1u : 0u));
    }
}

// One lane per camera sample of the chunk (ids enumerate owned tile, pixel in tile, sample of the chunk: consecutive lanes are
// samples of one pixel, so the rays of a wave are coherent).  EXT / TIES as in the path kernels: the lean build serves the scenes
// of the headline feature set (triangles, constant colours, pinhole camera), TIES keeps the reference's exact-t tie rule.
#ifndef GBL_AOV_WAVES
#define GBL_AOV_WAVES 2   // 256 registers for the EXT builds (texture graphs and image lookups), as sss_kernel
#endif
template <bool REPLAY, bool STATS, bool EXT, bool TIES>
__global__ __launch_bounds__(GBL_BLOCK, EXT ? GBL_AOV_WAVES : 4) void aov_kernel(DevScene sc, RenderArgs ra, AovArgs aa) {
    extern __shared__ __align__(16) unsigned char smem[];
    const LdsStack stk = {gbl_as_lds(reinterpret_cast<uint32_t*>(smem) + threadIdx.x)};
    LaneCounters cnt = {};
    uint32_t paths = 0;
    const uint64_t per_tile = 64ull * static_cast<uint64_t>(aa.pass_spp);
    const uint64_t total = static_cast<uint64_t>(ra.local_tiles) * per_tile;
    for (uint64_t id = static_cast<uint64_t>(blockIdx.x) * GBL_BLOCK + threadIdx.x; id < total; id += static_cast<uint64_t>(gridDim.x) * GBL_BLOCK) {
        const uint32_t lt = static_cast<uint32_t>(id / per_tile), r = static_cast<uint32_t>(id % per_tile);
        const uint32_t pix = r / static_cast<uint32_t>(aa.pass_spp), kk = r % static_cast<uint32_t>(aa.pass_spp);
        const uint32_t k = static_cast<uint32_t>(aa.pass_k0) + kk;
        int px, py;
        tile_pixel(ra, lt, pix, &px, &py);
        if (px >= ra.window[1] || py >= ra.window[3]) continue;
        const uint32_t wp = window_pixel(ra, px, py);
        const size_t out_index = static_cast<size_t>(wp) * ra.spp + k;
        float image_x, image_y;
        F3 o, d;
        float mint;
        const SampleSource src = camera_sample<EXT, REPLAY>(sc, ra, px, py, k, REPLAY ? ra.replay + out_index * ra.dims : nullptr, &image_x, &image_y,
                                                            &o, &d, &mint);
        Hit hit;
        const bool got = trace<false, STATS, EXT, TIES>(sc, o, d, mint, INFINITY, stk, hit, cnt);
        if (STATS) {
            cnt.ext += 1;
            paths += 1;
        }
        aov_write<EXT, REPLAY>(sc, aa, src, got, hit, o, d, image_x, image_y, static_cast<size_t>(wp) * aa.pass_spp + kk, out_index);
    }
    if (STATS) accumulate_stats(ra, cnt, paths);
}

// The same records from packet queries (kernels/packet.h): one wave per (pixel, 64 samples of the chunk), the 64 camera rays
// walking the tree together as in the primary pass of the path tracer (kernels_quad.hip primary_kernel).  Lean scenes under the
// native sampler with stack_entries <= GBL_PACKET_STACK.  A ray whose answer depends on the visiting order -- an exact tie; under
// EXACT also a hit the reference's box tests might pass by (trace.h trace_needs_redo) -- is traced again on its own, right here, so
// every record is what aov_kernel<false, false, false, EXACT> writes.  LDS: the waves' shared stacks (static) and the lanes' own
// for those retraces (dynamic, stack_lds_bytes).
template <bool EXACT>
__global__ __launch_bounds__(GBL_BLOCK) void aov_packet_kernel(DevScene sc, RenderArgs ra, AovArgs aa) {
    __shared__ uint32_t pk_stack[(GBL_BLOCK / 64) * GBL_PACKET_STACK_WORDS];
    extern __shared__ __align__(16) unsigned char smem[];
    gbl_lds_u32* const wstack = gbl_as_lds(pk_stack + (threadIdx.x >> 6) * GBL_PACKET_STACK_WORDS);
    const LdsStack stk = {gbl_as_lds(reinterpret_cast<uint32_t*>(smem) + threadIdx.x)};
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t chunks = (static_cast<uint32_t>(aa.pass_spp) + 63u) / 64u;
    const uint64_t n_tasks = static_cast<uint64_t>(ra.local_tiles) * 64u * chunks;   // (owned tile, pixel of the tile, 64-sample chunk)
    const uint64_t waves = static_cast<uint64_t>(gridDim.x) * (GBL_BLOCK / 64);
    for (uint64_t task = static_cast<uint64_t>(blockIdx.x) * (GBL_BLOCK / 64) + (threadIdx.x >> 6); task < n_tasks; task += waves) {
        const uint32_t c = static_cast<uint32_t>(task % chunks);
        const uint64_t pt = task / chunks;
        const uint32_t pix = static_cast<uint32_t>(pt % 64u), lt = static_cast<uint32_t>(pt / 64u);
        int px, py;
        tile_pixel(ra, lt, pix, &px, &py);
        if (px >= ra.window[1] || py >= ra.window[3]) continue;   // (wave-uniform: an edge tile's clipped pixels)
        const uint32_t kk = c * 64u + lane;
        const bool live = kk < static_cast<uint32_t>(aa.pass_spp);
        const uint32_t k = static_cast<uint32_t>(aa.pass_k0) + (live ? kk : 0u);
        float image_x, image_y;
        F3 o, d;
        float mint;
        const SampleSource src = camera_sample<false, false>(sc, ra, px, py, k, nullptr, &image_x, &image_y, &o, &d, &mint);
        Hit hit;
        bool tied;
        bool got = packet_closest(sc, live, o, d, mint, wstack, hit, tied);
        if (EXACT && live) tied = trace_needs_redo(sc, false, got, hit, tied, o, d, mint, INFINITY);
        if (live && tied) {
            LaneCounters scratch = {};
            got = trace<false, false, false, EXACT>(sc, o, d, mint, INFINITY, stk, hit, scratch);
        }
        if (live) {
            const uint32_t wp = window_pixel(ra, px, py);
            aov_write<false, false>(sc, aa, src, got, hit, o, d, image_x, image_y, static_cast<size_t>(wp) * aa.pass_spp + kk,
                                    static_cast<size_t>(wp) * ra.spp + k);
        }
    }
}
