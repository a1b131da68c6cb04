// libgoblin_hip.so, kernel unit: gbl_film_variance and the passes of gbl_film_denoise (kernels/denoise.h).
#include "gbl_internal.h"
#include "kernels/denoise.h"

void gbl_launch_film_variance(const float* li, float* variance, const int32_t window[4], int spp, int width, int height, hipStream_t stream) {
    const int ww = window[1] - window[0], wh = window[3] - window[2];
    const long long n = static_cast<long long>(ww) * wh;
    if (n == 0) return;
    hipLaunchKernelGGL(film_variance_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, stream, reinterpret_cast<const float4*>(li),
                       variance, window[0], window[2], ww, wh, spp, width, height);
}

void gbl_launch_denoise_prepare(const float* film, const float* variance, const float* albedo, const float* normal, const float* depth, float4* cv,
                                float4* nz, float4* af, int n, uint32_t demodulate, hipStream_t stream) {
    hipLaunchKernelGGL(denoise_prepare_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, reinterpret_cast<const float4*>(film), variance,
                       reinterpret_cast<const float4*>(albedo), reinterpret_cast<const float4*>(normal), reinterpret_cast<const float4*>(depth), cv, nz,
                       af, n, demodulate);
}

// LDS of the staging level kernel at a stride: tile and halo of the three planes; 0 where that is more than a workgroup may have
// (a CU's 160 KB, the limit the traversal stacks are held to as well: api_aov.hip, api_render.hip)
static const size_t kDenoiseLdsLimit = 160 * 1024;
size_t gbl_denoise_lds_bytes(int stride) {
    const size_t sw = GBL_DN_TILE_W + 4 * static_cast<size_t>(stride), sh = GBL_DN_TILE_H + 4 * static_cast<size_t>(stride);
    const size_t bytes = sw * sh * 3 * sizeof(float4);
    return bytes <= kDenoiseLdsLimit ? bytes : 0;
}

// *lds_allowed: the context's note that the staging kernel has been allowed its largest tile on the context's device (a launch
// with more than 64 KB of dynamic LDS needs that once, not per call)
hipError_t gbl_launch_denoise_level(bool lds, const float4* cv_in, const float4* nz, const float4* af, float4* cv_out, const DenoiseArgs& a, hipStream_t stream,
                                    bool* lds_allowed) {
    const dim3 grid((a.W + GBL_DN_TILE_W - 1) / GBL_DN_TILE_W, (a.H + GBL_DN_TILE_H - 1) / GBL_DN_TILE_H), block(GBL_DN_TILE_W * GBL_DN_TILE_H);
    if (!lds) {
        hipLaunchKernelGGL(denoise_level_kernel<false>, grid, block, 0, stream, cv_in, nz, af, cv_out, a);
        return hipGetLastError();
    }
    const size_t bytes = gbl_denoise_lds_bytes(a.stride);
    if (bytes == 0) return hipErrorInvalidValue;
    if (bytes > 64 * 1024 && !*lds_allowed) {
        size_t largest = bytes;   // the staged tile of the largest stride that fits
        for (int s = a.stride; gbl_denoise_lds_bytes(s) != 0; s *= 2) largest = gbl_denoise_lds_bytes(s);
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(denoise_level_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 static_cast<int>(largest));
        if (e != hipSuccess) return e;
        *lds_allowed = true;
    }
    hipLaunchKernelGGL(denoise_level_kernel<true>, grid, block, bytes, stream, cv_in, nz, af, cv_out, a);
    return hipGetLastError();
}

void gbl_launch_denoise_finish(const float4* cv, const float4* af, float* film_out, int n, uint32_t demodulate, hipStream_t stream) {
    hipLaunchKernelGGL(denoise_finish_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, cv, af, reinterpret_cast<float4*>(film_out), n, demodulate);
}
