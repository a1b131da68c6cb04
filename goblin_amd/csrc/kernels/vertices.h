// Device-pointer vertex edits (gbl_update_vertices_device, gbl_render_motion_deform_device): what the host
// entries do to the caller's floats with loops on the host, done where the floats are.
//
//   vertices_check_kernel   the lowest index of a float that is not finite, over positions and (when given) normals
//   mesh_bound_kernel       a mesh's object bound with the bits mesh_object_bound gives: (value, vertex) keys, reduced by 64-bit
//                           atomic minima; mesh_bound_finish turns the six winning vertices back into floats
//   pose_differs_kernel     per listed mesh: do its previous positions differ bitwise from the context's
//
// Every index is bounded by a count the host passes in; nothing is indexed from data another kernel or the caller wrote, but for
// mesh_bound_finish's vertex numbers, which it checks against the count.  The words the kernels meet in -- the check word, the
// six keys, the flags -- are set by the host before every launch (all ones, or zero for the flags), and are read by the host or
// by the next launch in the stream: no workgroup waits for another.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vertices_args.h"

#define GBL_VERTICES_BLOCK 256

// Not finite by the bits (the exponent field is all ones), whatever the compiler assumes about floats
__device__ __forceinline__ bool vertices_not_finite(float v) { return (__float_as_uint(v) & 0x7F800000u) == 0x7F800000u; }

// *first_bad (0xFFFFFFFF before the launch) = the lowest i < n with positions[i] or normals[i] not finite.  normals may be NULL.
// One atomic per wave that found one.
__global__ void vertices_check_kernel(const float* positions, const float* normals, uint32_t n, uint32_t* first_bad) {
    const uint32_t stride = gridDim.x * blockDim.x;
    uint32_t bad = 0xFFFFFFFFu;
    // (i + stride may wrap for n near 2^32: the loop ends on the wrap as well)
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        if (vertices_not_finite(positions[i]) || (normals != nullptr && vertices_not_finite(normals[i]))) {
            bad = i;   // a lane's indices rise: its first is its lowest
            break;
        }
        if (i + stride < i) break;
    }
    for (int off = 32; off > 0; off >>= 1) bad = min(bad, static_cast<uint32_t>(__shfl_xor(static_cast<int>(bad), off)));
    if ((threadIdx.x & 63u) == 0u && bad != 0xFFFFFFFFu) atomicMin(first_bad, bad);
}

// A float as an unsigned key that orders like the float compares: -0 and +0 share a key, as they compare equal
__device__ __forceinline__ uint32_t vertices_order_key(float v) {
    uint32_t b = __float_as_uint(v);
    if (b == 0x80000000u) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// keys[0..2]: per axis the lowest (order key of the coordinate, vertex) -- the lowest value, and among equal values the lowest
// vertex, which is the one std::min folded in vertex order keeps; keys[3..5]: the same over the complemented order key, the
// highest value and among equal ones the lowest vertex, as std::max keeps.  All ones before the launch.  One thread per vertex
// and turn, a wave's six minima by shuffles, a workgroup's through LDS, six atomics per workgroup.
__global__ void mesh_bound_kernel(const float* positions, uint32_t vertex_count, unsigned long long* keys) {
    __shared__ unsigned long long wave_keys[GBL_VERTICES_BLOCK / 64][6];
    unsigned long long k[6];
    for (int s = 0; s < 6; ++s) k[s] = ~0ull;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < vertex_count; v += stride) {
        const float* p = positions + 3 * static_cast<size_t>(v);
        for (int a = 0; a < 3; ++a) {
            const uint32_t o = vertices_order_key(p[a]);
            const unsigned long long lo = (static_cast<unsigned long long>(o) << 32) | v, hi = (static_cast<unsigned long long>(~o) << 32) | v;
            k[a] = lo < k[a] ? lo : k[a];
            k[3 + a] = hi < k[3 + a] ? hi : k[3 + a];
        }
        if (v + stride < v) break;
    }
    for (int s = 0; s < 6; ++s)
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long other = __shfl_xor(k[s], off);
            k[s] = other < k[s] ? other : k[s];
        }
    const uint32_t wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    if ((threadIdx.x & 63u) == 0u)
        for (int s = 0; s < 6; ++s) wave_keys[wave][s] = k[s];
    __syncthreads();
    if (threadIdx.x < 6u) {
        unsigned long long m = ~0ull;
        for (uint32_t w = 0; w < waves && w < GBL_VERTICES_BLOCK / 64; ++w) m = wave_keys[w][threadIdx.x] < m ? wave_keys[w][threadIdx.x] : m;
        if (m != ~0ull) atomicMin(keys + threadIdx.x, m);
    }
}

// The launch after mesh_bound_kernel: bound[0..2] = lo, bound[3..5] = hi, each the winning vertex's own float (its bits tell +0
// from -0, which the key does not).  A mesh without vertices leaves the keys all ones: +infinity / -infinity, mesh_object_bound's
// empty box.
__global__ void mesh_bound_finish(const float* positions, uint32_t vertex_count, const unsigned long long* keys, float* bound) {
    const uint32_t s = threadIdx.x;
    if (s >= 6u) return;
    const unsigned long long key = keys[s];
    const uint32_t v = static_cast<uint32_t>(key);
    float out = s < 3u ? INFINITY : -INFINITY;
    if (key != ~0ull && v < vertex_count) out = positions[3 * static_cast<size_t>(v) + s % 3u];
    bound[s] = out;
}

// differs[m] (0 before the launch) = 1 iff mesh m's previous positions differ bitwise from the context's.  blockIdx.y is the
// listed mesh; one atomic per wave that saw a difference.
__global__ void pose_differs_kernel(const PoseList* list, uint32_t num_listed, const float* positions, uint32_t num_floats_total, uint32_t* differs) {
    const uint32_t m = blockIdx.y;
    if (m >= num_listed) return;
    const PoseList pl = list[m];
    if (static_cast<uint64_t>(pl.first_float) + pl.num_floats > num_floats_total) return;   // (the host checked; not from device data)
    const uint32_t stride = gridDim.x * blockDim.x;
    bool diff = false;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < pl.num_floats; i += stride) {
        if (__float_as_uint(pl.prev[i]) != __float_as_uint(positions[pl.first_float + i])) {
            diff = true;
            break;
        }
        if (i + stride < i) break;
    }
    if (__any(diff) && (threadIdx.x & 63u) == 0u) atomicOr(differs + m, 1u);
}
