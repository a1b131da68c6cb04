// libgoblin_hip.so, kernel unit: the passes of gbl_update_environment* (kernels/environment.h).
#include "gbl_internal.h"
#include "kernels/environment.h"

void gbl_launch_environment(const EnvironmentArgs& a, unsigned parts, hipStream_t stream) {
    const uint32_t texels = a.dw * a.dh;
    if (texels == 0) return;
    if (parts & 2u) {
        hipLaunchKernelGGL(environment_func, dim3((texels + GBL_BLOCK - 1) / GBL_BLOCK), dim3(GBL_BLOCK), 0, stream, a);
        hipLaunchKernelGGL(environment_rows, dim3((a.dh + GBL_ENV_ROWS - 1) / GBL_ENV_ROWS), dim3(GBL_BLOCK), 0, stream, a);
    }
    if (parts & 4u) hipLaunchKernelGGL(environment_tail, dim3(1), dim3(GBL_ENV_TAIL), 0, stream, a);
}
