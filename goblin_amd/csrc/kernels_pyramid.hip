// libgoblin_hip.so, kernel unit: the pass of gbl_update_image* (kernels/pyramid.h).
#include "gbl_internal.h"
#include "kernels/pyramid.h"

void gbl_launch_pyramid_level(const PyramidArgs& a, hipStream_t stream) {
    const uint32_t texels = static_cast<uint32_t>(a.dw) * static_cast<uint32_t>(a.dh);
    if (texels == 0) return;
    hipLaunchKernelGGL(pyramid_level, dim3((texels + GBL_BLOCK - 1) / GBL_BLOCK), dim3(GBL_BLOCK), 0, stream, a);
}
