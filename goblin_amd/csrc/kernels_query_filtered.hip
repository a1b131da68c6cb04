// libgoblin_hip.so, kernel unit: gbl_trace_rays_filtered's kernels (kernels/query_filtered.h).  EXT builds only: a scene with a mask
// material is `extended`, and a scene without one is answered through gbl_trace_rays' kernels and the two fills below.
#include "gbl_internal.h"
#include "kernels/query_filtered.h"

gbl_query_filtered_kernel gbl_kernel_query_filtered(uint32_t kind, bool ties, bool normal) {
    if (kind == GBL_QUERY_TRANSMITTANCE) {
        if (normal) return nullptr;
        return ties ? query_filtered_trace<GBL_QK_TRANSMITTANCE, true, false> : query_filtered_trace<GBL_QK_TRANSMITTANCE, false, false>;
    }
    if (kind == GBL_QUERY_ANY) {
        if (normal) return nullptr;
        return ties ? query_filtered_trace<GBL_QK_ANY, true, false> : query_filtered_trace<GBL_QK_ANY, false, false>;
    }
    if (normal) return ties ? query_filtered_trace<GBL_QK_CLOSEST, true, true> : query_filtered_trace<GBL_QK_CLOSEST, false, true>;
    return ties ? query_filtered_trace<GBL_QK_CLOSEST, true, false> : query_filtered_trace<GBL_QK_CLOSEST, false, false>;
}

static unsigned fill_grid(uint32_t n) { return static_cast<unsigned>(std::min<uint64_t>((static_cast<uint64_t>(n) + GBL_BLOCK - 1) / GBL_BLOCK, 4096)); }

void gbl_launch_query_fill_miss(float4* hits, uint32_t n, hipStream_t stream) {
    hipLaunchKernelGGL(query_fill_miss, dim3(fill_grid(n)), dim3(GBL_BLOCK), 0, stream, hits, n);
}

void gbl_launch_query_any_to_transmittance(const uint8_t* occluded, float4* out, uint32_t n, hipStream_t stream) {
    hipLaunchKernelGGL(query_any_to_transmittance, dim3(fill_grid(n)), dim3(GBL_BLOCK), 0, stream, occluded, out, n);
}
