// What the material and texture edits (api_materials.hip, host only) and their compose kernels (kernels/materials.h) share:
// plain data.
#pragma once
#include <stdint.h>

#include "../device_scene.h"

// A raw row of gbl_update_materials_device: {color[3], color2[3], color3[3], index, k, exponent}
#define GBL_MAT_ROW_FLOATS 12
// ... and of gbl_update_textures_device: {value[3], uv_scale[2], uv_offset[2]}
#define GBL_TEX_ROW_FLOATS 7

// Records [first, first + count) of the live table take the editable fields of rows[0 .. count); every other field stays
struct MatComposeArgs {
    DevMaterial* materials;
    const float* rows;   // count * GBL_MAT_ROW_FLOATS, 4-byte aligned
    uint32_t first, count;
};
struct TexComposeArgs {
    DevTexture* textures;
    const float* rows;   // count * GBL_TEX_ROW_FLOATS, 4-byte aligned
    uint32_t first, count;
};
