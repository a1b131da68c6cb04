// libgoblin_hip.so, kernel unit: the passes of gbl_update_vertices (kernels/refit.h) and of gbl_mesh_tree_stats (kernels/treestats.h).
#include "gbl_internal.h"
#include "kernels/refit.h"
#include "kernels/treestats.h"

void gbl_launch_refit_tris(DevTri* tris, DevTriBound* bounds, const DevTriShade* tri_shade, const float* pos, uint32_t num_vertices, uint32_t first,
                           uint32_t count, hipStream_t stream) {
    if (count == 0) return;
    hipLaunchKernelGGL(refit_tris, dim3((count + GBL_BLOCK - 1) / GBL_BLOCK), dim3(GBL_BLOCK), 0, stream, tris, bounds, tri_shade, pos, num_vertices, first, count);
}

void gbl_launch_refit_level(DevNode* nodes, const DevTriBound* bounds, const RefitRecord* plan, RefitBox* node_box, uint32_t begin, uint32_t end,
                            hipStream_t stream) {
    if (end <= begin) return;
    hipLaunchKernelGGL(refit_level, dim3((end - begin + GBL_BLOCK - 1) / GBL_BLOCK), dim3(GBL_BLOCK), 0, stream, nodes, bounds, plan, node_box, begin, end);
}

void gbl_launch_tree_stats(const DevNode* nodes, uint64_t num_nodes, const RefitRecord* plan, uint32_t num_records, double* sums, double* partial,
                           hipStream_t stream) {
    if (num_records == 0) return;
    const uint32_t blocks = (num_records + GBL_BLOCK - 1) / GBL_BLOCK;
    hipLaunchKernelGGL(treestats_partial, dim3(blocks), dim3(GBL_BLOCK), 0, stream, nodes, num_nodes, plan, num_records, sums, partial);
    hipLaunchKernelGGL(treestats_sum, dim3(1), dim3(64), 0, stream, partial, blocks, sums);
}
