// libgoblin_hip.so, kernel unit: gbl_render_motion (kernels/motion.h) and the accumulate kernels of gbl_film_accumulate_motion
// (kernels/temporal.h, its MOTION flavour).
#include "gbl_internal.h"
#define GBL_TEMPORAL_NO_PREPARE   // temporal_prepare_kernel is kernels_temporal.hip's
#include "kernels/motion.h"

gbl_motion_kernel gbl_kernel_motion(bool packet, bool ext, bool deform) {
    if (deform) {
        if (packet) return motion_packet_deform_kernel;
        return ext ? motion_deform_kernel<true> : motion_deform_kernel<false>;
    }
    if (packet) return motion_packet_kernel;
    return ext ? motion_kernel<true> : motion_kernel<false>;
}

// as gbl_launch_temporal_accumulate, the reprojection read from `motion`
void gbl_launch_temporal_accumulate_motion(bool spatial, const float4* cl, const float4* nz, const uint32_t* fl, const float* variance,
                                           const float* history_in, float* history_out, float* film_out, float* variance_out, const float* motion,
                                           const TemporalArgs& a, hipStream_t stream) {
    const dim3 grid((a.W + GBL_TP_TILE_W - 1) / GBL_TP_TILE_W, (a.H + GBL_TP_TILE_H - 1) / GBL_TP_TILE_H), block(GBL_TP_TILE_W * GBL_TP_TILE_H);
    const float4* hin = reinterpret_cast<const float4*>(history_in);
    float4* hout = reinterpret_cast<float4*>(history_out);
    float4* fout = reinterpret_cast<float4*>(film_out);
    const float4* mo = reinterpret_cast<const float4*>(motion);
    if (spatial)
        hipLaunchKernelGGL(temporal_accumulate_motion_kernel<true>, grid, block, 0, stream, cl, nz, fl, variance, hin, hout, fout, variance_out, mo, a);
    else
        hipLaunchKernelGGL(temporal_accumulate_motion_kernel<false>, grid, block, 0, stream, cl, nz, fl, variance, hin, hout, fout, variance_out, mo, a);
}
