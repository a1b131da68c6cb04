// sss_kernel: Renderer::Lsubsurface of every camera sample as a pass ahead of the path kernels (see bssrdf.h).
#pragma once
#include "bssrdf.h"
#include "render_kernels.h"

// One lane per camera sample of the launch's tiles (ids enumerate owned tile, pixel in tile, sample: consecutive lanes
// are samples of one pixel, so the primary rays of a wave are coherent).  out[pixel * spp + k], pixel-major over the
// render window like li_out.
#ifndef GBL_SSS_WAVES
#define GBL_SSS_WAVES 2   // 256 registers (left alone: 301 with 45 accumulation registers, one wave per SIMD)
#endif
template <bool REPLAY, bool STATS>
__global__ __launch_bounds__(GBL_BLOCK, GBL_SSS_WAVES) void sss_kernel(DevScene sc, RenderArgs ra, float4* out) {
    extern __shared__ __align__(16) unsigned char smem[];
    const LdsStack stk = {gbl_as_lds(reinterpret_cast<uint32_t*>(smem) + threadIdx.x)};
    LaneCounters cnt = {};
    const uint64_t per_tile = 64ull * static_cast<uint64_t>(ra.spp);
    const uint64_t total = static_cast<uint64_t>(ra.local_tiles) * per_tile;
    for (uint64_t id = static_cast<uint64_t>(blockIdx.x) * GBL_BLOCK + threadIdx.x; id < total; id += static_cast<uint64_t>(gridDim.x) * GBL_BLOCK) {
        const uint32_t lt = static_cast<uint32_t>(id / per_tile), r = static_cast<uint32_t>(id % per_tile);
        const uint32_t pix = r / static_cast<uint32_t>(ra.spp), k = r % static_cast<uint32_t>(ra.spp);
        int px, py;
        tile_pixel(ra, lt, pix, &px, &py);
        if (px >= ra.window[1] || py >= ra.window[3]) continue;
        const uint32_t out_index = window_pixel(ra, px, py) * ra.spp + k;
        float image_x, image_y;
        F3 o, d;
        float mint;
        const SampleSource src = camera_sample<true, REPLAY>(sc, ra, px, py, k, REPLAY ? ra.replay + static_cast<size_t>(out_index) * ra.dims : nullptr,
                                                             &image_x, &image_y, &o, &d, &mint);
        F3 L = f3(0, 0, 0);
        Hit hit;
        LaneCounters scratch = {};   // the camera ray is the path kernel's query; it is not counted twice
        if (sc.num_lights > 0 && trace<false, false, true>(sc, o, d, mint, INFINITY, stk, hit, scratch)) {
            const int material = sc.instances[hit.inst].material;
            if (sc.materials[material].type == GBL_MAT_SUBSURFACE) {
                Frag fr;
                TexFrag tf;
                make_fragment<true>(sc, hit, o, d, fr, &tf);
                DevMaterial mo;
                sss_resolve(sc, material, fr, tf, mo);   // Lsubsurface runs before computeUVDifferential (GoblinPathtracer.cpp:69, :77)
                const F3 wo = -d;
                const F3 single = l_bssrdf_single<REPLAY, STATS>(sc, ra, src, fr, mo, material, wo, stk, cnt);
                const F3 multi = l_bssrdf_diffusion<REPLAY, STATS>(sc, ra, src, fr, tf, mo, material, wo, stk, cnt);
                L = single + multi;
            }
        }
        out[out_index] = make_float4(L.x, L.y, L.z, 0.0f);
    }
    if (STATS) accumulate_stats(ra, cnt, 0);
}
