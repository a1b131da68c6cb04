// libgoblin_hip.so, kernel unit: the passes of the device-pointer vertex entries (kernels/vertices.h).
#include "gbl_internal.h"
#include "kernels/vertices.h"

// Grid-stride launches: enough workgroups for one element per thread, at most `cap`
static unsigned vertices_blocks(uint64_t n, unsigned cap) {
    const uint64_t want = (n + GBL_VERTICES_BLOCK - 1) / GBL_VERTICES_BLOCK;
    return static_cast<unsigned>(want < 1 ? 1 : want > cap ? cap : want);
}

void gbl_launch_vertices_check(const float* positions, const float* normals, uint32_t n, uint32_t* first_bad, hipStream_t stream) {
    if (n == 0) return;
    hipLaunchKernelGGL(vertices_check_kernel, dim3(vertices_blocks(n, 1024)), dim3(GBL_VERTICES_BLOCK), 0, stream, positions, normals, n, first_bad);
}

void gbl_launch_mesh_bound(const float* positions, uint32_t vertex_count, unsigned long long* keys, float* bound, hipStream_t stream) {
    if (vertex_count > 0)
        hipLaunchKernelGGL(mesh_bound_kernel, dim3(vertices_blocks(vertex_count, 64)), dim3(GBL_VERTICES_BLOCK), 0, stream, positions, vertex_count, keys);
    hipLaunchKernelGGL(mesh_bound_finish, dim3(1), dim3(64), 0, stream, positions, vertex_count, keys, bound);
}

void gbl_launch_pose_differs(const PoseList* list, uint32_t num_listed, uint32_t max_floats, const float* positions, uint32_t num_floats_total, uint32_t* differs,
                             hipStream_t stream) {
    for (uint32_t m0 = 0; m0 < num_listed; m0 += 65535u) {   // (a grid's y extent)
        const uint32_t m = num_listed - m0 < 65535u ? num_listed - m0 : 65535u;
        hipLaunchKernelGGL(pose_differs_kernel, dim3(vertices_blocks(max_floats, 256), m), dim3(GBL_VERTICES_BLOCK), 0, stream, list + m0, m, positions,
                           num_floats_total, differs + m0);
    }
}
