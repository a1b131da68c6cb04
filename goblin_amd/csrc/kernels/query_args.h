// Arguments of gbl_trace_rays' kernels (kernels/query.h) beyond the scene: the caller's rays and output, the per-mesh triangle
// offsets that turn a hit's triangle record into the scene description's numbering, and the launch's stack and hot-prefix layout.
// DevScene stays what every kernel takes by value; nothing of the query lives in it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct QueryArgs {
    const float4* rays;             // gbl_ray: {o.xyz, mint}, {d.xyz, maxt} -- two 16-byte loads per ray
    float4* hits;                   // closest-hit queries: gbl_ray_hit, two 16-byte stores per ray
    uint8_t* occluded;              // any-hit queries: one byte per ray
    const uint32_t* mesh_tri_offset;   // per mesh of the scene description: gbl_mesh::tri_offset (DevTri::shade minus this = primitive)
    uint32_t* stack_spill;          // global backing of the stacks beyond GBL_WF_STACK_LDS levels, one column per thread of the grid
    uint32_t n;                     // rays
    uint32_t hot_count, hot_word;   // nodes[0 .. hot_count) also live in LDS, at word hot_word of the workgroup's block (HotSplitStack)
};
