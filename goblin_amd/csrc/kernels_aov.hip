// libgoblin_hip.so, kernel unit: the first-hit feature pass of gbl_render_aov (kernels/aov.h) and the depth film's resolve.
#include "gbl_internal.h"
#include "kernels/aov.h"

// Built: the lean kernel of the native sampler with and without the tie rule, and the EXT build (always with it, like every EXT
// path kernel) for the feature scenes, the replay sampler and instrumented calls.
gbl_aov_kernel gbl_kernel_aov(bool replay, bool stats, bool ext, bool exact_ties) {
    if (stats) return replay ? aov_kernel<true, true, true, true> : aov_kernel<false, true, true, true>;
    if (replay) return aov_kernel<true, false, true, true>;
    if (ext) return aov_kernel<false, false, true, true>;
    return exact_ties ? aov_kernel<false, false, false, true> : aov_kernel<false, false, false, false>;
}
gbl_aov_kernel gbl_kernel_aov_packet(bool exact_ties) { return exact_ties ? aov_packet_kernel<true> : aov_packet_kernel<false>; }

// depth = sum w t hit / sum w hit, coverage = sum w hit / sum w; 0 where the denominator is 0
__global__ void aov_resolve_depth_kernel(const float4* accum, float* depth, float* coverage, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 a = accum[i];
    depth[i] = a.y != 0.0f ? a.x / a.y : 0.0f;
    if (coverage) coverage[i] = a.w != 0.0f ? a.y / a.w : 0.0f;
}
void gbl_launch_aov_resolve_depth(const float* accum, float* depth, float* coverage, int n, hipStream_t stream) {
    hipLaunchKernelGGL(aov_resolve_depth_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, reinterpret_cast<const float4*>(accum), depth, coverage, n);
}
