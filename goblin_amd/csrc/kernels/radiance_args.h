// Arguments of gbl_radiance_rays' kernels (kernels/radiance.h) beyond the scene: the caller's rays and output, the integrator's
// settings, where a path's draws come from, and the launch's stack and hot-prefix layout.  DevScene, RenderArgs and QueryArgs stay
// what they are; nothing of the call lives in them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct RadianceArgs {
    const float4* rays;             // gbl_ray: {o.xyz, mint}, {d.xyz, maxt} -- two 16-byte loads per ray
    float4* out;                    // {Li.r, Li.g, Li.b, 1} per ray; {0, 0, 0, 0} for an invalid one
    const float* records;           // replay builds: record i is ray i's, `dims` floats
    uint32_t* stack_spill;          // global backing of the stacks beyond GBL_WF_STACK_LDS levels, one column per thread of the grid
    uint32_t n;                     // rays
    uint32_t hot_count, hot_word;   // nodes[0 .. hot_count) also live in LDS, at word hot_word of the workgroup's block (HotSplitStack)
    int32_t max_depth;              // PathTracer's max_ray_depth: the loop runs max_depth - 1 times
    int32_t dims, off2_base;        // replay: floats per record, float offset of the first 2D pattern (api_render.hip sample_layout)
    int32_t spp, root;              // native: samples per group and their square root
    uint32_t first_group;           // native: the group of ray 0
    uint32_t seed_key;              // native: as RenderArgs::seed_key
    uint32_t russian_roulette;      // native: the build-side extension of gbl_render_params.russian_roulette
};
