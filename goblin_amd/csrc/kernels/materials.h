// Material and texture edits (gbl_update_materials*, gbl_update_textures*): the editable fields of a DevMaterial
// and of a DevTexture written from a raw row, stated once.
//
//   mat_compose / tex_compose   host + device inline: scene_prep.cpp's pack_materials / pack_textures call them for every
//                               record they pack, the kernels below for every record they edit, so the two cannot drift apart
//   mat_compose_kernel          one lane per edited material: the live record in, its editable fields from the row, the record out
//   tex_compose_kernel          the same for a texture
//
// The first half needs no HIP: tests/test_materials_cpu.py compiles it with g++ beside scene_prep.cpp and compares bits.  The
// kernels use no LDS and no atomics, and every index is bounded by a count the host passes in.
#pragma once
#include <stdint.h>

#include "../../../include/goblin_hip.h"
#include "materials_args.h"

#ifdef __HIPCC__
#define GBL_MAT_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define GBL_MAT_HD inline
#endif

// a / b rounded as IEEE division rounds it, on either side
GBL_MAT_HD float mat_div(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}

// BSSRDF ctor (GoblinMaterial.cpp:32-38): A = (1 + Fdr) / (1 - Fdr) from the diffuse Fresnel reflectance polynomial
// (GoblinMaterial.h:94-105)
GBL_MAT_HD float mat_bssrdf_a(float eta) {
    const float fdr = eta < 1.0f ? -0.4399f + mat_div(0.7099f, eta) - mat_div(0.3319f, eta * eta) + mat_div(0.0636f, eta * eta * eta)
                                 : mat_div(-1.4399f, eta * eta) + mat_div(0.7099f, eta) + 0.6681f + 0.0636f * eta;
    return mat_div(1.0f + fdr, 1.0f - fdr);
}

// The editable fields of a record whose type is in place: row = {color[3], color2[3], color3[3], index, k, exponent}.  color3
// belongs to a subsurface material only and stays as it is (zero) elsewhere; a subsurface material's exponent holds A and the
// row's is ignored.
GBL_MAT_HD void mat_compose(DevMaterial* dm, const float row[GBL_MAT_ROW_FLOATS]) {
    for (int k = 0; k < 3; ++k) dm->color[k] = row[k], dm->color2[k] = row[3 + k];
    dm->index = row[9];
    dm->k = row[10];
    if (dm->type == GBL_MAT_SUBSURFACE) {
        for (int k = 0; k < 3; ++k) dm->color3[k] = row[6 + k];
        dm->exponent = mat_bssrdf_a(row[9]);
    } else {
        dm->exponent = row[11];
    }
}

// ... of a texture whose is_float is in place: row = {value[3], uv_scale[2], uv_offset[2]}.  A float texture's value[0] is
// broadcast.
GBL_MAT_HD void tex_compose(DevTexture* t, const float row[GBL_TEX_ROW_FLOATS]) {
    for (int k = 0; k < 3; ++k) t->value[k] = t->is_float ? row[0] : row[k];
    for (int k = 0; k < 2; ++k) t->uv_scale[k] = row[3 + k], t->uv_offset[k] = row[5 + k];
}

// The raw rows of a description's records: what the compose functions read
GBL_MAT_HD void mat_row_of(const gbl_material& m, float row[GBL_MAT_ROW_FLOATS]) {
    for (int k = 0; k < 3; ++k) row[k] = m.color[k], row[3 + k] = m.color2[k], row[6 + k] = m.color3[k];
    row[9] = m.index;
    row[10] = m.k;
    row[11] = m.exponent;
}
GBL_MAT_HD void tex_row_of(const gbl_texture& g, float row[GBL_TEX_ROW_FLOATS]) {
    for (int k = 0; k < 3; ++k) row[k] = g.value[k];
    for (int k = 0; k < 2; ++k) row[3 + k] = g.uv_scale[k], row[5 + k] = g.uv_offset[k];
}

// (hipcc compiles scene_prep.cpp and api_materials.hip as HIP too: the kernels are for the one unit that asks for them)
#if defined(__HIPCC__) && defined(GBL_MATERIALS_KERNELS)
__global__ void __launch_bounds__(GBL_BLOCK) mat_compose_kernel(const MatComposeArgs a) {
    const uint32_t i = blockIdx.x * GBL_BLOCK + threadIdx.x;
    if (i >= a.count) return;
    float row[GBL_MAT_ROW_FLOATS];
    for (int k = 0; k < GBL_MAT_ROW_FLOATS; ++k) row[k] = a.rows[static_cast<size_t>(i) * GBL_MAT_ROW_FLOATS + k];
    DevMaterial dm = a.materials[a.first + i];
    mat_compose(&dm, row);
    a.materials[a.first + i] = dm;
}

__global__ void __launch_bounds__(GBL_BLOCK) tex_compose_kernel(const TexComposeArgs a) {
    const uint32_t i = blockIdx.x * GBL_BLOCK + threadIdx.x;
    if (i >= a.count) return;
    float row[GBL_TEX_ROW_FLOATS];
    for (int k = 0; k < GBL_TEX_ROW_FLOATS; ++k) row[k] = a.rows[static_cast<size_t>(i) * GBL_TEX_ROW_FLOATS + k];
    DevTexture t = a.textures[a.first + i];
    tex_compose(&t, row);
    a.textures[a.first + i] = t;
}
#endif
