// Tree cost (gbl_mesh_tree_stats): the surface areas of the QUANTISED child boxes of one mesh's BLAS -- the boxes
// traversal tests -- summed over the plan of scene_refit.h.  A ray that enters the root's box meets a child box with a
// probability close to the ratio of their areas, so node_area / root_area is the expected number of interior children it
// visits and tri_area / root_area the expected number of triangles it tests (the surface area heuristic's two sums).
//
//   treestats_partial   one lane per plan record, all levels in one launch: the node's used slots, corners o + float(q) * scale
//                       in float32, areas in double; shuffles and LDS leave two sums per workgroup.  Record 0 is the root:
//                       its lane also writes the area of the union of the root's used slots.
//   treestats_sum       one wave adds the workgroups' sums in index order
//
// The kernels only read `nodes`, use no atomics and no workgroup waits for another: two calls return the same bits.  Every
// index is bounded by a count the host passes.
#pragma once
#include <hip/hip_runtime.h>

#include "../device_scene.h"
#include "refit_args.h"

// dx * dy + dy * dz + dz * dx in double, the differences of the float32 corners formed in double
__device__ __forceinline__ double treestats_area(const float* lo, const float* hi) {
    const double dx = static_cast<double>(hi[0]) - static_cast<double>(lo[0]);
    const double dy = static_cast<double>(hi[1]) - static_cast<double>(lo[1]);
    const double dz = static_cast<double>(hi[2]) - static_cast<double>(lo[2]);
    return dx * dy + dy * dz + dz * dx;
}

__device__ __forceinline__ double treestats_wave_sum(double v) {
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
    return v;   // (lane 0 holds the wave's sum)
}

__global__ __launch_bounds__(GBL_BLOCK) void treestats_partial(const DevNode* nodes, uint64_t num_nodes, const RefitRecord* plan, uint32_t num_records,
                                                                double* sums, double* partial) {
    __shared__ double wave_sums[2 * (GBL_BLOCK / 64)];
    const uint32_t r = blockIdx.x * GBL_BLOCK + threadIdx.x;
    double node_area = 0.0, tri_area = 0.0;
    if (r < num_records) {
        const int32_t at = plan[r].node;
        if (at >= 0 && static_cast<uint64_t>(at) < num_nodes) {
            const DevNode nd = nodes[at];
            float ulo[3] = {INFINITY, INFINITY, INFINITY}, uhi[3] = {-INFINITY, -INFINITY, -INFINITY};
            bool any = false;
            for (int c = 0; c < 4; ++c) {
                const int32_t ref = nd.child[c];
                if (ref == static_cast<int32_t>(GBL_REF_NONE)) continue;
                float lo[3], hi[3];
                for (int a = 0; a < 3; ++a) {
                    lo[a] = nd.o[a] + static_cast<float>((nd.qlo[a] >> (8 * c)) & 0xffu) * nd.scale[a];
                    hi[a] = nd.o[a] + static_cast<float>((nd.qhi[a] >> (8 * c)) & 0xffu) * nd.scale[a];
                    ulo[a] = fminf(ulo[a], lo[a]);
                    uhi[a] = fmaxf(uhi[a], hi[a]);
                }
                any = true;
                const double area = treestats_area(lo, hi);
                if (ref < 0)
                    tri_area += static_cast<double>((~static_cast<uint32_t>(ref) & 3u) + 1u) * area;
                else
                    node_area += area;
            }
            if (r == 0) sums[0] = any ? treestats_area(ulo, uhi) : 0.0;
        }
    }
    node_area = treestats_wave_sum(node_area);
    tri_area = treestats_wave_sum(tri_area);
    const uint32_t wave = threadIdx.x / 64;
    if ((threadIdx.x & 63u) == 0) {
        wave_sums[2 * wave] = node_area;
        wave_sums[2 * wave + 1] = tri_area;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double n = 0.0, t = 0.0;
        for (int w = 0; w < GBL_BLOCK / 64; ++w) {
            n += wave_sums[2 * w];
            t += wave_sums[2 * w + 1];
        }
        partial[2 * static_cast<size_t>(blockIdx.x)] = n;
        partial[2 * static_cast<size_t>(blockIdx.x) + 1] = t;
    }
}

// One wave: lane l adds partials l, l + 64, ... in index order, the lanes' sums are added by shuffles
__global__ __launch_bounds__(64) void treestats_sum(const double* partial, uint32_t num_partials, double* sums) {
    double n = 0.0, t = 0.0;
    for (uint32_t i = threadIdx.x; i < num_partials; i += 64) {
        n += partial[2 * static_cast<size_t>(i)];
        t += partial[2 * static_cast<size_t>(i) + 1];
    }
    n = treestats_wave_sum(n);
    t = treestats_wave_sum(t);
    if (threadIdx.x == 0) {
        sums[1] = n;
        sums[2] = t;
    }
}
