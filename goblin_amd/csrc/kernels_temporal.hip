// libgoblin_hip.so, kernel unit: the passes of gbl_film_accumulate (kernels/temporal.h).
#include "gbl_internal.h"
#include "kernels/temporal.h"

void gbl_launch_temporal_prepare(const float* film, const float* variance, const float* normal, const float* depth, float4* cl, float4* nz, uint32_t* fl,
                                 int n, hipStream_t stream) {
    hipLaunchKernelGGL(temporal_prepare_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, reinterpret_cast<const float4*>(film), variance,
                       reinterpret_cast<const float4*>(normal), reinterpret_cast<const float4*>(depth), cl, nz, fl, n);
}

// spatial: the kernel that estimates the variance itself (no variance plane: `variance` is not read)
void gbl_launch_temporal_accumulate(bool spatial, const float4* cl, const float4* nz, const uint32_t* fl, const float* variance, const float* history_in,
                                    float* history_out, float* film_out, float* variance_out, const TemporalArgs& a, hipStream_t stream) {
    const dim3 grid((a.W + GBL_TP_TILE_W - 1) / GBL_TP_TILE_W, (a.H + GBL_TP_TILE_H - 1) / GBL_TP_TILE_H), block(GBL_TP_TILE_W * GBL_TP_TILE_H);
    const float4* hin = reinterpret_cast<const float4*>(history_in);
    float4* hout = reinterpret_cast<float4*>(history_out);
    float4* fout = reinterpret_cast<float4*>(film_out);
    if (spatial)
        hipLaunchKernelGGL(temporal_accumulate_kernel<true>, grid, block, 0, stream, cl, nz, fl, variance, hin, hout, fout, variance_out, a);
    else
        hipLaunchKernelGGL(temporal_accumulate_kernel<false>, grid, block, 0, stream, cl, nz, fl, variance, hin, hout, fout, variance_out, a);
}
