// libgoblin_hip.so, kernel unit: the passes of the device-pointer instance entries (kernels/instances.h) and the TLAS build on
// the device over instance boxes (kernels/lbvh.h's hierarchy and fit, instances.h's keys and collapse).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "gbl_host.h"
#include <hipcub/hipcub.hpp>

namespace {   // lbvh.h's kernels once more, with internal linkage: kernels_aux.hip holds the BLAS path's under the same names
#include "kernels/lbvh.h"
}
#include "kernels/instances.h"

static_assert(sizeof(LbvhBox) == sizeof(DevInstanceBound), "an instance bound is read as the builder's box");
static_assert(sizeof(DevInstance) == 128 && sizeof(DevInstanceBound) == 24 && sizeof(gbl_trs) == 40, "the records gbl_selftest_instances documents");

void gbl_launch_inst_compose(const gbl_trs* d_trs, uint32_t first, uint32_t count, const DevInstance* live, const float* mesh_bounds, uint32_t num_meshes,
                             bool refuse_box, DevInstance* out_inst, DevInstanceBound* out_bound, unsigned long long* refusal, hipStream_t stream) {
    if (count == 0) return;
    hipLaunchKernelGGL(inst_compose_kernel, dim3((count + GBL_INSTANCES_BLOCK - 1) / GBL_INSTANCES_BLOCK), dim3(GBL_INSTANCES_BLOCK), 0, stream,
                       reinterpret_cast<const float*>(d_trs), first, count, live, mesh_bounds, num_meshes, refuse_box ? 1u : 0u, out_inst, out_bound, refusal);
}

// The TLAS over d_bounds[0 .. n), n >= 2, built into the context's builder scratch: *d_nodes_out points at its records there
// (node k refers to its children as tlas_base + their number; record 0 is the root), valid until the scratch's next user.
// Nothing of the scene is written.  One 8-byte read-back per level; the device is idle on return.
gbl_status gbl_build_tlas_device(gbl_ctx* ctx, const DevInstanceBound* d_bounds, uint32_t n, int32_t tlas_base, uint32_t capacity, const DevNode** d_nodes_out,
                                 uint32_t* nodes_out, int* depth_out) {
    if (n < 2 || capacity == 0) return fail(ctx, GBL_ERR_INTERNAL, "gbl_update_instances_device: a device TLAS needs two instances and room for a node");
    const size_t ni = n - 1;
    size_t temp_bytes = 0;
    HIP_TRY(ctx, hipcub::DeviceRadixSort::SortKeys(nullptr, temp_bytes, static_cast<unsigned long long*>(nullptr), static_cast<unsigned long long*>(nullptr),
                                                   static_cast<int>(n), 0, 62));
    size_t scratch_bytes = 0;
    const auto take = [&](size_t count, size_t size) {
        const size_t at = scratch_bytes;
        scratch_bytes += (std::max<size_t>(1, count) * size + 255) & ~static_cast<size_t>(255);
        return at;
    };
    const size_t o_keys = take(n, sizeof(unsigned long long)), o_sorted = take(n, sizeof(unsigned long long));
    const size_t o_left = take(ni, sizeof(int32_t)), o_right = take(ni, sizeof(int32_t)), o_parent = take(2 * static_cast<size_t>(n), sizeof(int32_t));
    const size_t o_first = take(ni, sizeof(uint32_t)), o_last = take(ni, sizeof(uint32_t)), o_box = take(ni, sizeof(LbvhBox)), o_leaf_box = take(n, sizeof(LbvhBox));
    const size_t o_visits = take(ni, sizeof(uint32_t)), o_fa = take(ni, sizeof(LbvhFrontier)), o_fb = take(ni, sizeof(LbvhFrontier));
    const size_t o_counters = take(2, sizeof(uint32_t)), o_bound = take(6, sizeof(uint32_t)), o_nodes = take(capacity, sizeof(DevNode)), o_temp = take(temp_bytes, 1);
    const gbl_status grown = grow(ctx, ctx->lbvh_scratch, scratch_bytes, "device BVH build scratch");
    if (grown != GBL_OK) return grown;
    unsigned char* const base = static_cast<unsigned char*>(ctx->lbvh_scratch.p);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(base + o_keys);
    unsigned long long* keys_sorted = reinterpret_cast<unsigned long long*>(base + o_sorted);
    LbvhTree t;
    memset(&t, 0, sizeof(t));
    t.left = reinterpret_cast<int32_t*>(base + o_left);
    t.right = reinterpret_cast<int32_t*>(base + o_right);
    t.parent = reinterpret_cast<int32_t*>(base + o_parent);
    t.first = reinterpret_cast<uint32_t*>(base + o_first);
    t.last = reinterpret_cast<uint32_t*>(base + o_last);
    t.box = reinterpret_cast<LbvhBox*>(base + o_box);
    t.leaf_box = reinterpret_cast<LbvhBox*>(base + o_leaf_box);
    t.visits = reinterpret_cast<uint32_t*>(base + o_visits);
    LbvhFrontier* fa = reinterpret_cast<LbvhFrontier*>(base + o_fa);
    LbvhFrontier* fb = reinterpret_cast<LbvhFrontier*>(base + o_fb);
    uint32_t* counters = reinterpret_cast<uint32_t*>(base + o_counters);   // [0] next frontier size, [1] nodes emitted
    uint32_t* bound_keys = reinterpret_cast<uint32_t*>(base + o_bound);
    DevNode* d_nodes = reinterpret_cast<DevNode*>(base + o_nodes);
    unsigned char* temp = base + o_temp;

    const dim3 block(GBL_INSTANCES_BLOCK), grid((n + GBL_INSTANCES_BLOCK - 1) / GBL_INSTANCES_BLOCK);
    HIP_TRY(ctx, hipMemsetAsync(bound_keys, 0xFF, 3 * sizeof(uint32_t), 0));
    HIP_TRY(ctx, hipMemsetAsync(bound_keys + 3, 0, 3 * sizeof(uint32_t), 0));
    hipLaunchKernelGGL(inst_scene_bound_kernel, dim3(std::min<unsigned>(grid.x, 256u)), block, 0, 0, d_bounds, n, bound_keys);
    hipLaunchKernelGGL(inst_keys_kernel, grid, block, 0, 0, d_bounds, n, bound_keys, keys);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipcub::DeviceRadixSort::SortKeys(temp, temp_bytes, keys, keys_sorted, static_cast<int>(n), 0, 62));
    hipLaunchKernelGGL(lbvh_gather_boxes, grid, block, 0, 0, keys_sorted, reinterpret_cast<const LbvhBox*>(d_bounds), n, t.leaf_box);
    hipLaunchKernelGGL(lbvh_hierarchy, grid, block, 0, 0, keys_sorted, static_cast<int>(n), t);
    HIP_TRY(ctx, hipMemsetAsync(t.visits, 0, ni * sizeof(uint32_t), 0));
    hipLaunchKernelGGL(lbvh_fit, grid, block, 0, 0, static_cast<int>(n), t);
    HIP_TRY(ctx, hipGetLastError());
    // collapse, one 4-wide level per launch
    const LbvhFrontier rootf = {0, 0};
    const uint32_t init[2] = {0u, 1u};
    HIP_TRY(ctx, hipMemcpy(fa, &rootf, sizeof(rootf), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(counters, init, sizeof(init), hipMemcpyHostToDevice));
    uint32_t n_in = 1, used = 1;
    int depth = 0;
    while (n_in > 0) {
        ++depth;
        hipLaunchKernelGGL(inst_collapse_kernel, dim3((n_in + GBL_INSTANCES_BLOCK - 1) / GBL_INSTANCES_BLOCK), block, 0, 0, t, keys_sorted, n, fa, n_in, fb, counters,
                           counters + 1, d_nodes, capacity, tlas_base);
        HIP_TRY(ctx, hipGetLastError());
        uint32_t h[2];
        HIP_TRY(ctx, hipMemcpy(h, counters, sizeof(h), hipMemcpyDeviceToHost));
        n_in = h[0];
        used = h[1];
        if (used > capacity || n_in > ni) return fail(ctx, GBL_ERR_INTERNAL, "gbl_update_instances_device: the device TLAS outgrew its reserved nodes");
        HIP_TRY(ctx, hipMemsetAsync(counters, 0, sizeof(uint32_t), 0));
        std::swap(fa, fb);
        if (depth > 128) return fail(ctx, GBL_ERR_DEVICE, "gbl_update_instances_device: the device TLAS build did not terminate");
    }
    HIP_TRY(ctx, hipDeviceSynchronize());
    *d_nodes_out = d_nodes;
    *nodes_out = used;
    *depth_out = depth;
    return GBL_OK;
}
