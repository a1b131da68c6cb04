// What the host side of the device-pointer vertex entries (api_geometry.hip, api_motion.hip) and their kernels
// (kernels/vertices.h) share: plain data.
#pragma once
#include <stdint.h>

// One listed mesh of gbl_render_motion_deform_device: its previous positions (the caller's device memory) and its slice of the
// context's positions
struct PoseList {
    const float* prev;
    uint32_t first_float;   // 3 * vertex_offset
    uint32_t num_floats;    // 3 * vertex_count
};

// gbl_ctx::vertex_words: the words a call's launches meet in, set to all ones by one fill before them, and the bound behind
#define GBL_VW_KEYS 0      // six 64-bit keys (mesh_bound_kernel)
#define GBL_VW_CHECK 48    // the check word (vertices_check_kernel), padded to 64
#define GBL_VW_FILL 64     // bytes the fill covers
#define GBL_VW_BOUND 64    // six floats: lo, hi (mesh_bound_finish)
#define GBL_VW_BYTES 96
