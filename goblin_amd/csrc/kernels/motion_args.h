// What the host side of gbl_render_motion (api_motion.hip) and its kernels (kernels/motion.h) share: the arguments of the call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../device_scene.h"

#define GBL_MOTION_XF_FLOATS 24   // per instance in MotionArgs::prev_xf: the previous toWorld rows 0..2 (3x4), then its inverse's

struct MotionArgs {
    int W, H;
    DevCamera prev;            // params->prev_camera, packed by pack_camera with the context's film
    const float* prev_xf;      // GBL_MOTION_XF_FLOATS per instance; an entry is read only where `moved` says so
    const uint32_t* moved;     // per instance: its previous transform differs from the current one; null: no instance moved
    const float4* normal;      // the current frame's normal film, or null
    float4* out;               // M0 then M1, W * H float4 each
    // gbl_render_motion_deform (read by the DEFORM kernels only, and only on a hit of a triangle mesh)
    const float* prev_pos;     // 3 per vertex: the previous positions of the deformed meshes, packed (motion_stage.h)
    const int32_t* mesh_prev;  // per mesh: packed_first_vertex - vertex_offset, or GBL_MOTION_STATIC: the mesh is not deformed
    uint32_t num_meshes;       // entries of mesh_prev ...
    uint32_t prev_count;       // ... and vertices of prev_pos: an index beyond either is never followed
};
#define GBL_MOTION_STATIC INT32_MIN   // (motion_stage.h GBL_MOTION_NOT_DEFORMED)
