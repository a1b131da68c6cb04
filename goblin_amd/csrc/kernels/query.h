// gbl_trace_rays' kernels: Scene::intersect / Scene::occluded for a flat array of caller rays in device memory.
//
//   query_trace   wf_trace's loop (kernels/wavefront.h) without the path pool: persistent workgroups, the hot top of the tree in
//                 LDS, HotSplitStack, and per wave an in-wave refill -- wave w owns the 64-ray regions w, w + n_waves, ... of the
//                 array and hands their rays to its idle lanes by ballot + prefix popcount while the busy lanes keep traversing.
//                 The cursor is the wave's own: no atomics.  Steps are phased by majority state (trace.h GBL_TRAV_TH).
//   query_plain   one ray per lane, grid-stride, trace<>() over a plain LdsStack, as the self-test hook calls it.  Built only
//                 under -DGBL_QUERY_PLAIN, for the measurement of DESIGN.md 4.11.
//
// ANY: Scene::occluded, one byte per ray; else Scene::intersect, one gbl_ray_hit per ray.  EXT: the scene holds analytic shapes
// (DevScene::extended).  TIES: the reference's exact-t tie rule and reachability test, inline at every accepted triangle
// (GBL_TIE_EXACT, as wf_trace: the redo form spills there); without it the bare loop (GBL_TIE_NONE), which never reads tri_order.
// NORMAL: the hit's world-space shading normal, make_fragment's Frag::n, not flipped.
// Queries are unfiltered (GBL_FILTER_NONE): the surface of a mask material is a surface.
#pragma once
#include "../device_scene.h"
#include "query_args.h"
#include "shade.h"
#include "trace.h"
#include "vecmath.h"

#ifndef GBL_QUERY_REFILL
#define GBL_QUERY_REFILL 16   // refill as soon as this many lanes of the wave are idle (wavefront.h WF_REFILL)
#endif
#ifndef GBL_QUERY_WAVES
#define GBL_QUERY_WAVES 5     // waves per SIMD the kernels are compiled for (wavefront.h GBL_WF_TRACE_WAVES)
#endif

// A ray that may enter traversal: no NaN among its eight floats, finite origin and direction, a direction that is not all
// zeros, mint <= maxt (maxt = +inf and mint = -inf are fine).  Anything else is answered as a miss without a node fetched.
__device__ __forceinline__ bool query_ray_valid(float4 a, float4 b) {
    const bool finite = fabsf(a.x) < INFINITY && fabsf(a.y) < INFINITY && fabsf(a.z) < INFINITY && fabsf(b.x) < INFINITY &&
                        fabsf(b.y) < INFINITY && fabsf(b.z) < INFINITY;   // (false for a NaN too)
    const bool moves = b.x != 0.0f || b.y != 0.0f || b.z != 0.0f;
    return finite && moves && a.w <= b.w;   // (false when mint or maxt is a NaN)
}

// gbl_ray_hit of a finished closest-hit query: {t, b1, b2, instance}, {primitive, n.xyz}; a miss is {-1, 0, 0, -1}, {0, 0, 0, 0}
template <bool EXT, bool NORMAL>
__device__ __forceinline__ void query_store_hit(const DevScene& sc, const QueryArgs& qa, uint32_t idx, const Hit& h, F3 o, F3 d) {
    float4 r0 = make_float4(-1.0f, 0.0f, 0.0f, __int_as_float(-1)), r1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (h.inst >= 0) {
        const DevInstance* ip = sc.instances + h.inst;
        uint32_t prim = 0u;   // a sphere or a disk
        if (!(EXT && ip->shape != 0u)) prim = sc.tris[h.tri].shade - qa.mesh_tri_offset[ip->mesh];
        r0 = make_float4(h.t, h.b1, h.b2, __int_as_float(h.inst));
        r1.x = __uint_as_float(prim);
        if (NORMAL) {
            Frag fr;
            make_fragment<EXT>(sc, h, o, d, fr);
            r1.y = fr.n.x;
            r1.z = fr.n.y;
            r1.w = fr.n.z;
        }
    }
    qa.hits[2 * static_cast<size_t>(idx)] = r0;
    qa.hits[2 * static_cast<size_t>(idx) + 1] = r1;
}

// (EXT with NORMAL: make_fragment's analytic shapes and bump shaders at 96 registers spill 220 - 270 of them; compiled for 3
//  waves per SIMD, as wf_trace's MASKS builds are)
template <bool ANY, bool EXT, bool TIES, bool NORMAL>
__global__ __launch_bounds__(GBL_BLOCK, (EXT && NORMAL) ? 3 : GBL_QUERY_WAVES) void query_trace(DevScene sc, QueryArgs qa) {
    extern __shared__ __align__(16) unsigned char smem[];
    HotSplitStack stk;
    stk.p = gbl_as_lds(reinterpret_cast<uint32_t*>(smem) + threadIdx.x);
    stk.g = gbl_as_global(qa.stack_spill + blockIdx.x * GBL_BLOCK + threadIdx.x);
    stk.gstride = gridDim.x * GBL_BLOCK;
    {   // the top of the tree, once per (persistent) workgroup: trace.h HotLdsStack
        uint4* hot = reinterpret_cast<uint4*>(reinterpret_cast<uint32_t*>(smem) + qa.hot_word);
        for (uint32_t i = threadIdx.x; i < 4u * qa.hot_count; i += GBL_BLOCK) hot[i] = reinterpret_cast<const uint4*>(sc.nodes)[i];
        stk.hot = (const gbl_lds_u4*)hot;
        stk.hot_count = qa.hot_count;
        if (qa.hot_count) __syncthreads();
    }
    LaneCounters cnt = {};
    const int lane = threadIdx.x & 63;
    const uint32_t n_regions = (qa.n >> 6) + ((qa.n & 63u) != 0u ? 1u : 0u);   // (n + 63 may not fit 32 bits)
    const uint32_t n_waves = gridDim.x * (GBL_BLOCK / 64);
    // this wave's regions: w, w + n_waves, w + 2 n_waves, ...; the last region of the array may be short
    uint32_t region = blockIdx.x * (GBL_BLOCK / 64) + (threadIdx.x >> 6);
    auto region_count = [&](uint32_t r) { return r < n_regions ? min(64u, qa.n - r * 64u) : 0u; };
    uint32_t r_off = 0, r_cnt = region_count(region);

    bool busy = false;
    TravState st;
    st.sp = 0;
    st.cur = GBL_STACK_EXIT;
    st.inst = -1;
    st.mint = st.maxt = 0.0f;
    uint32_t idx = 0;

    for (;;) {
        // ---- refill idle lanes from this wave's regions (all scalar bookkeeping)
        const unsigned long long idle = __ballot(!busy);
        const int n_idle = __popcll(idle);
        if (region < n_regions && n_idle >= GBL_QUERY_REFILL) {
            const int my_rank = __popcll(idle & ((1ull << lane) - 1ull));
            int assigned = 0;
            uint32_t my_entry = 0xffffffffu;   // (no ray has this number: n < 2^32)
            while (assigned < n_idle && region < n_regions) {
                const int avail = static_cast<int>(r_cnt - r_off);
                const int take = min(avail, n_idle - assigned);
                if (!busy && my_rank >= assigned && my_rank < assigned + take) my_entry = region * 64u + r_off + static_cast<uint32_t>(my_rank - assigned);
                assigned += take;
                r_off += take;
                if (r_off >= r_cnt) {
                    region += n_waves;
                    r_off = 0;
                    r_cnt = region_count(region);
                }
            }
            if (my_entry != 0xffffffffu) {
                const float4 a = qa.rays[2 * static_cast<size_t>(my_entry)], b = qa.rays[2 * static_cast<size_t>(my_entry) + 1];
                if (query_ray_valid(a, b)) {
                    idx = my_entry;
                    trav_begin(sc, st, f3(a.x, a.y, a.z), f3(b.x, b.y, b.z), a.w, b.w, stk);
                    busy = true;
                } else if (ANY) {   // an invalid ray: unoccluded / a miss, and the lane stays idle
                    qa.occluded[my_entry] = 0;
                } else {
                    Hit miss;
                    miss.inst = -1;
                    query_store_hit<EXT, false>(sc, qa, my_entry, miss, f3(0, 0, 0), f3(0, 0, 0));
                }
            }
        }
        const bool drained = region >= n_regions;
        if (__ballot(busy) == 0ull) {
            if (drained) break;
            continue;
        }
        // ---- traverse while enough lanes are busy (or nothing is left to fetch)
        const int keep = drained ? 1 : (64 - GBL_QUERY_REFILL + 1);
        while (__popcll(__ballot(busy)) >= keep) {
            const bool at_int = busy && trav_at_interior(st);
            const bool at_oth = busy && !at_int;
            const unsigned long long mi = __ballot(at_int), mo = __ballot(at_oth);
            if (mo == 0ull || __popcll(mi) >= GBL_TRAV_TH) {
                if (at_int) trav_interior<false, !ANY>(sc, st, stk, cnt);
            } else if (at_oth) {
                bool occluded = false;
                if (trav_other<ANY, false, EXT, HotSplitStack, TIES ? GBL_TIE_EXACT : GBL_TIE_NONE, GBL_FUSE_TAIL>(sc, st, stk, cnt, &occluded, GBL_FILTER_NONE)) {
                    if (ANY) qa.occluded[idx] = occluded ? 1 : 0;
                    else query_store_hit<EXT, NORMAL>(sc, qa, idx, st.hit, st.world.o, st.world.d);
                    busy = false;
                }
            }
        }
    }
}

#ifdef GBL_QUERY_PLAIN
template <bool ANY, bool EXT, bool TIES, bool NORMAL>
__global__ __launch_bounds__(GBL_BLOCK) void query_plain(DevScene sc, QueryArgs qa) {
    extern __shared__ __align__(16) unsigned char smem[];
    const LdsStack stk = {gbl_as_lds(reinterpret_cast<uint32_t*>(smem) + threadIdx.x)};
    LaneCounters cnt = {};
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * GBL_BLOCK;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * GBL_BLOCK + threadIdx.x; i < qa.n; i += stride) {
        const float4 a = qa.rays[2 * i], b = qa.rays[2 * i + 1];
        const F3 o = f3(a.x, a.y, a.z), d = f3(b.x, b.y, b.z);
        Hit hit;
        hit.inst = -1;
        const bool valid = query_ray_valid(a, b);
        if (ANY) {
            qa.occluded[i] = valid && trace<true, false, EXT, TIES>(sc, o, d, a.w, b.w, stk, hit, cnt) ? 1 : 0;
        } else {
            if (!(valid && trace<false, false, EXT, TIES>(sc, o, d, a.w, b.w, stk, hit, cnt))) hit.inst = -1;
            query_store_hit<EXT, NORMAL>(sc, qa, static_cast<uint32_t>(i), hit, o, d);
        }
    }
}
#endif
