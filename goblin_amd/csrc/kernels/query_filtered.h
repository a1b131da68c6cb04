// gbl_trace_rays_filtered's kernels: Scene::intersect / Scene::occluded under the reference's isOpaque / notOpaque IntersectFilter, and
// the transmittance of a shadow segment as PathTracer::Li takes it, for a flat array of caller rays in device memory.
//
//   query_filtered_trace   query_trace's loop (kernels/query.h: persistent workgroups, the hot top of the tree in LDS, HotSplitStack,
//                          refill by ballot + prefix popcount, steps phased by majority state) with the filter a RUN-TIME value of the
//                          launch, handed to trav_other, whose trav_enter skips an instance on the wrong side whole at its TLAS leaf.
//   query_fill_miss, query_any_to_transmittance   the two answers of a scene without masks that need no traversal of their own.
//
// KIND: GBL_QUERY_CLOSEST, GBL_QUERY_ANY, or GBL_QUERY_TRANSMITTANCE -- an isOpaque any-hit query whose unoccluded lanes go on, inline
// and at once, to the attenuation walk over the mask surfaces of their segment (as wf_trace's MASKS builds do: the other lanes of the
// wave wait for them).  EXT always: a mask material makes the scene `extended`.  TIES, NORMAL: as query_trace.
#pragma once
#include "query.h"
#include "query_filtered_args.h"
#include "render_kernels.h"   // eval_attenuation, which query_attenuation restates with a count

#define GBL_QK_CLOSEST 0
#define GBL_QK_ANY 1
#define GBL_QK_TRANSMITTANCE 2
#define GBL_TR_OCCLUDED 0x80000000u   // gbl_ray_transmittance::crossed of a segment an opaque surface blocks

// eval_attenuation (render_kernels.h) with the number of factors multiplied in: the same queries, the same lookups, the same products
// in the same order -- PathTracer::evalAttenuation (GoblinPathtracer.cpp:21-48).  A subsurface wrap answers Black before its factor
// is formed and is not counted; a factor that takes the product to Black is.
template <class STK>
__device__ __forceinline__ F3 query_attenuation(const DevScene& sc, F3 o, F3 d, float mint, float maxt, const STK& stk, LaneCounters& cnt, uint32_t* crossed) {
    F3 thr = f3(1.0f, 1.0f, 1.0f);
    uint32_t n = 0u;
    for (int guard = 0; guard < 1024; ++guard) {   // every step moves mint past a hit; the cap only bounds a degenerate scene
        Hit h;
        if (!trace<false, false, true>(sc, o, d, mint, maxt, stk, h, cnt, GBL_FILTER_MASK)) break;
        Frag fr;
        TexFrag tf;
        make_fragment<true>(sc, h, o, d, fr, &tf);
        uv_differential(fr, tf, false, o, o, o, o);
        const DevMaterial& m = sc.materials[sc.instances[h.inst].material];
        if (m.type == GBL_MAT_SUBSURFACE) {
            thr = f3(0.0f, 0.0f, 0.0f);
            break;
        }
        float alpha = m.tex_exponent >= 0 ? tex_eval<GBL_TEX_MAX_DEPTH>(sc, m.tex_exponent, fr, tf).x : m.exponent;
        F3 tcolor = m.tex_color >= 0 ? tex_eval<GBL_TEX_MAX_DEPTH>(sc, m.tex_color, fr, tf) : f3(m.color[0], m.color[1], m.color[2]);
        thr = thr * ((1.0f - alpha) * tcolor);
        ++n;
        if (is_black(thr)) break;
        mint = h.t + fr.eps;   // currentRay.mint = currentRay.maxt + epsilon
    }
    *crossed = n;
    return thr;
}

__device__ __forceinline__ void query_store_transmittance(const FilteredQueryArgs& fa, uint32_t idx, F3 tr, uint32_t crossed) {
    fa.transmittance[idx] = make_float4(tr.x, tr.y, tr.z, __uint_as_float(crossed));
}

// (NORMAL and TRANSMITTANCE: make_fragment plus, for the walk, tex_eval -- compiled for 3 waves per SIMD as query_trace<.., EXT, .., NORMAL>)
template <int KIND, bool TIES, bool NORMAL>
__global__ __launch_bounds__(GBL_BLOCK, (NORMAL || KIND == GBL_QK_TRANSMITTANCE) ? 3 : GBL_QUERY_WAVES) void query_filtered_trace(DevScene sc, FilteredQueryArgs fa) {
    constexpr bool ANY = KIND != GBL_QK_CLOSEST, TRANSMIT = KIND == GBL_QK_TRANSMITTANCE;
    const QueryArgs& qa = fa.q;
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
    const int filter = TRANSMIT ? GBL_FILTER_OPAQUE : fa.filter;   // Scene::occluded(ray, isOpaque) ahead of the walk
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
                } else if (TRANSMIT) {   // an invalid ray: nothing between its ends, and the lane stays idle
                    query_store_transmittance(fa, my_entry, f3(1.0f, 1.0f, 1.0f), 0u);
                } else if (ANY) {
                    qa.occluded[my_entry] = 0;
                } else {
                    Hit miss;
                    miss.inst = -1;
                    query_store_hit<true, false>(sc, qa, my_entry, miss, f3(0, 0, 0), f3(0, 0, 0));
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
                if (trav_other<ANY, false, true, HotSplitStack, TIES ? GBL_TIE_EXACT : GBL_TIE_NONE, GBL_FUSE_TAIL>(sc, st, stk, cnt, &occluded, filter)) {
                    if constexpr (TRANSMIT) {
                        F3 tr = f3(0.0f, 0.0f, 0.0f);
                        uint32_t crossed = GBL_TR_OCCLUDED;
                        // the lane's stack is free again: the walk's queries run on it
                        if (!occluded) tr = query_attenuation(sc, st.world.o, st.world.d, st.mint, st.maxt, stk, cnt, &crossed);
                        query_store_transmittance(fa, idx, tr, crossed);
                    } else if constexpr (ANY) {
                        qa.occluded[idx] = occluded ? 1 : 0;
                    } else {
                        query_store_hit<true, NORMAL>(sc, qa, idx, st.hit, st.world.o, st.world.d);
                    }
                    busy = false;
                }
            }
        }
    }
}

// A scene without masks under GBL_QUERY_FILTER_MASK: every closest-hit record is gbl_trace_rays' miss.
__global__ __launch_bounds__(GBL_BLOCK) void query_fill_miss(float4* hits, uint32_t n) {
    const uint32_t stride = gridDim.x * GBL_BLOCK;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * GBL_BLOCK + threadIdx.x; i < n; i += stride) {
        hits[2 * i] = make_float4(-1.0f, 0.0f, 0.0f, __int_as_float(-1));
        hits[2 * i + 1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}

// A scene without masks under GBL_QUERY_TRANSMITTANCE: the unfiltered any-hit answer in gbl_ray_transmittance's two forms.
__global__ __launch_bounds__(GBL_BLOCK) void query_any_to_transmittance(const uint8_t* occluded, float4* out, uint32_t n) {
    const uint32_t stride = gridDim.x * GBL_BLOCK;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * GBL_BLOCK + threadIdx.x; i < n; i += stride) {
        const float v = occluded[i] ? 0.0f : 1.0f;
        out[i] = make_float4(v, v, v, __uint_as_float(occluded[i] ? GBL_TR_OCCLUDED : 0u));
    }
}
