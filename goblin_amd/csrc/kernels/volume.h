// vol_kernel: the participating medium's {tr, Lv} of every camera sample as a pass of its own (see medium.h).
#pragma once
#include "medium.h"
#include "render_kernels.h"

// One lane per camera sample: the medium's {tr, Lv} into ra.vol[2 * out_index ..] (native / replay samplers).
template <bool REPLAY, bool STATS>
__global__ __launch_bounds__(GBL_BLOCK) void vol_kernel(DevScene sc, RenderArgs ra) {
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
        camera_sample<true, REPLAY>(sc, ra, px, py, k, REPLAY ? ra.replay + static_cast<size_t>(out_index) * ra.dims : nullptr, &image_x, &image_y, &o, &d,
                                    &mint);
        // the camera ray as Li leaves it: clipped at the first surface -- unless Li returned before its first query
        // (PathTracer::Li without lights, GoblinPathtracer.cpp:53-56)
        float maxt = INFINITY;
        if (!(ra.integrator == 0 && sc.num_lights == 0)) {
            Hit hit;
            LaneCounters scratch = {};   // the integrator's own query: not counted twice
            if (trace<false, false, true>(sc, o, d, mint, INFINITY, stk, hit, scratch)) maxt = hit.t;
        }
        VolRand rnd = vol_rand_hashed(image_x, image_y);
        const F3 tr = vol_transmittance(sc, o, d, mint, maxt, rnd);   // (Renderer::transmittance comes first: the heterogeneous region's jitter is the sample's first draw)
        const F3 Lv = volume_lv<STATS>(sc, o, d, mint, maxt, rnd, stk, cnt);
        float4* q = reinterpret_cast<float4*>(ra.vol) + 2 * static_cast<size_t>(out_index);
        q[0] = make_float4(tr.x, tr.y, tr.z, 0.0f);
        q[1] = make_float4(Lv.x, Lv.y, Lv.z, 0.0f);
    }
    if (STATS) accumulate_stats(ra, cnt, 0);
}
