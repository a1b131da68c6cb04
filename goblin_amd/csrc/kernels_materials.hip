// libgoblin_hip.so, kernel unit: the compose passes of gbl_update_materials_device / gbl_update_textures_device (kernels/materials.h).
#include "gbl_internal.h"
#define GBL_MATERIALS_KERNELS
#include "kernels/materials.h"

void gbl_launch_mat_compose(const MatComposeArgs& a, hipStream_t stream) {
    if (a.count == 0) return;
    hipLaunchKernelGGL(mat_compose_kernel, dim3((a.count + GBL_BLOCK - 1) / GBL_BLOCK), dim3(GBL_BLOCK), 0, stream, a);
}

void gbl_launch_tex_compose(const TexComposeArgs& a, hipStream_t stream) {
    if (a.count == 0) return;
    hipLaunchKernelGGL(tex_compose_kernel, dim3((a.count + GBL_BLOCK - 1) / GBL_BLOCK), dim3(GBL_BLOCK), 0, stream, a);
}
