// libgoblin_hip.so -- C ABI of the device integrator (include/goblin_hip.h): gbl_trace_rays, batched scene queries on rays in
// device memory (kernels/query.h), gbl_trace_rays_filtered, the same under the reference's isOpaque / notOpaque
// filters and the transmittance of a shadow segment (kernels/query_filtered.h), and the two self-test hooks, the same calls with
// their persistent grid capped.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "gbl_host.h"
#include "kernels/trace.h"   // GBL_WF_STACK_LDS

namespace {

// gbl_mesh::tri_offset per mesh on the device, made once: DevTri::shade numbers a triangle within the scene description, a
// hit reports it within its mesh.  No edit changes the offsets (vertex edits and rebuilds keep the topology).
gbl_status ensure_mesh_offsets(gbl_ctx* ctx) {
    if (ctx->d_mesh_tri_offset) return GBL_OK;
    std::vector<uint32_t> off(std::max<size_t>(1, ctx->h_meshes.size()), 0u);
    for (size_t m = 0; m < ctx->h_meshes.size(); ++m) off[m] = ctx->h_meshes[m].tri_offset;
    void* p = nullptr;
    const gbl_status st = device_alloc(ctx, off.size() * sizeof(uint32_t), "mesh triangle offsets", &p);
    if (st != GBL_OK) return st;
    HIP_TRY(ctx, hipMemcpy(p, off.data(), off.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    ctx->d_mesh_tri_offset = static_cast<uint32_t*>(p);
    return GBL_OK;
}

// Stack levels of the query kernels beyond the LDS part: one column per thread of the largest persistent grid (8 workgroups
// per CU), as wf_ensure_spill sizes the wavefront trace kernels'.  A buffer of its own: a query may be in flight on another
// stream than a wavefront render.  Re-made when an edit deepens the tree: grow() then frees and allocates, which waits for the device.
gbl_status ensure_query_spill(gbl_ctx* ctx) {
    const int deep = ctx->scene.stack_entries > GBL_WF_STACK_LDS ? ctx->scene.stack_entries - GBL_WF_STACK_LDS : 1;
    const uint64_t level_bytes = static_cast<uint64_t>(ctx->num_cus) * 8 * GBL_BLOCK * sizeof(uint32_t);
    return grow(ctx, ctx->query_spill, static_cast<uint64_t>(deep) * level_bytes, "query stack backing");
}

}   // namespace

// (gbl_host.h: gbl_radiance_rays checks its buffers and lays its launch out the same way)
// A call's buffers, as the entry points refuse them (n > 0): null pointers, 2^32 rays or more, memory that is not the device's or
// ends early, an output that overlaps the rays.  Sets the device.
gbl_status check_query_buffers(gbl_ctx* ctx, const std::string& who, const gbl_ray* d_rays, uint64_t n, void* d_out, uint64_t out_stride) {
    if (!d_rays || !d_out) return fail(ctx, GBL_ERR_INVALID, who + ": null pointer with n > 0");
    if (n >= (1ull << 32)) return fail(ctx, GBL_ERR_UNSUPPORTED, who + ": 2^32 rays or more in one call (the kernel keeps 32-bit ray indices)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint64_t ray_bytes = n * sizeof(gbl_ray), out_bytes = n * out_stride;
    gbl_status st = check_device_pointer(ctx, d_rays, ray_bytes, who, "d_rays");
    if (st != GBL_OK) return st;
    if ((st = check_device_pointer(ctx, d_out, out_bytes, who, "d_out")) != GBL_OK) return st;
    if (overlaps(d_rays, ray_bytes, d_out, out_bytes)) return fail(ctx, GBL_ERR_INVALID, who + ": d_out overlaps d_rays");
    return GBL_OK;
}

// The persistent kernels' launch: the stack backing and the LDS layout into qa, the grid into *wgs, the LDS bytes into *lds.
// max_workgroups: 0 for the grid the device holds
gbl_status persistent_layout(gbl_ctx* ctx, const void* kernel, uint64_t n, uint32_t max_workgroups, QueryArgs& qa, size_t* lds_out, uint64_t* wgs_out) {
    const DevScene& sc = ctx->scene;
    gbl_status st = ensure_query_spill(ctx);
    if (st != GBL_OK) return st;
    qa.stack_spill = static_cast<uint32_t*>(ctx->query_spill.p);
    // the stacks' LDS levels, then the top of the tree (trace.h HotSplitStack), as the wavefront trace launcher lays them out
    size_t lds = static_cast<size_t>(std::min<int>(sc.stack_entries, GBL_WF_STACK_LDS)) * GBL_BLOCK * sizeof(uint32_t);
    qa.hot_word = static_cast<uint32_t>(lds / sizeof(uint32_t));
    qa.hot_count = std::min<uint32_t>(GBL_WF_HOT_NODES, sc.hot_nodes);
    lds += qa.hot_count * sizeof(DevNode);
    // a persistent grid: exactly the resident workgroups (regions are assigned statically), never more waves than regions
    // (asked of the runtime once per kernel and LDS size of the context: a frame makes this call many times)
    const auto key = std::make_pair(kernel, lds);
    auto found = ctx->query_occupancy.find(key);
    if (found == ctx->query_occupancy.end()) {
        int asked = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&asked, key.first, GBL_BLOCK, lds) != hipSuccess || asked < 1) asked = 1;
        found = ctx->query_occupancy.emplace(key, asked).first;
    }
    const int occ = std::min(found->second, 8);   // query_spill is sized for 8 workgroups per CU
    const uint64_t regions = (n + 63) / 64;
    uint64_t wgs = std::min<uint64_t>(static_cast<uint64_t>(ctx->num_cus) * occ, (regions + GBL_BLOCK / 64 - 1) / (GBL_BLOCK / 64));
    if (max_workgroups > 0) wgs = std::min<uint64_t>(wgs, max_workgroups);
    *wgs_out = std::max<uint64_t>(1, wgs);
    *lds_out = lds;
    return GBL_OK;
}

namespace {

// gbl_trace_rays behind its refusals: n > 0 rays through the unfiltered kernels
gbl_status launch_unfiltered(gbl_ctx* ctx, const std::string& who, bool any, bool ties, bool normal, const gbl_ray* d_rays, uint64_t n, void* d_out,
                             uint32_t max_workgroups, hipStream_t stream) {
    const DevScene& sc = ctx->scene;
    // Which build: the EXT one for a scene beyond the headline feature set, with the tie rule only where the caller asks for
    // it.  Only the two exact_ties builds read tri_order (GBL_TIE_EXACT: tie_goes_to); the lean build and the EXT build without
    // the flag run GBL_TIE_NONE and leave a deferred vertex edit's tie order pending.
    const bool ext = sc.extended != 0;
    gbl_status st = make_orders_if(ctx, ties);
    if (st != GBL_OK) return st;
    gbl_query_kernel kernel = gbl_kernel_query(any, ext, ties, normal);
    if (!kernel) return fail(ctx, GBL_ERR_UNSUPPORTED, who + ": query kernel variant not built");
    if ((st = ensure_mesh_offsets(ctx)) != GBL_OK) return st;

    QueryArgs qa;
    memset(&qa, 0, sizeof(qa));
    qa.rays = reinterpret_cast<const float4*>(d_rays);
    qa.hits = any ? nullptr : static_cast<float4*>(d_out);
    qa.occluded = any ? static_cast<uint8_t*>(d_out) : nullptr;
    qa.mesh_tri_offset = ctx->d_mesh_tri_offset;
    qa.n = static_cast<uint32_t>(n);
    size_t lds = 0;
    uint64_t wgs = 0;
    if (gbl_query_plain()) {   // the measurement form: the whole stack in LDS, grid-stride.  Never taken in the shipped library: only a
                               // kernels_query.hip compiled with -DGBL_QUERY_PLAIN (tools/query_bench.py's variant) answers true
        lds = stack_lds_bytes(sc);
        if (lds > 160 * 1024) return fail(ctx, GBL_ERR_UNSUPPORTED, who + ": scene's BVH is too deep for the LDS traversal stacks");
        wgs = std::min<uint64_t>((n + GBL_BLOCK - 1) / GBL_BLOCK, static_cast<uint64_t>(ctx->num_cus) * 8);
        if (max_workgroups > 0) wgs = std::min<uint64_t>(wgs, max_workgroups);
        wgs = std::max<uint64_t>(1, wgs);
    } else if ((st = persistent_layout(ctx, reinterpret_cast<const void*>(kernel), n, max_workgroups, qa, &lds, &wgs)) != GBL_OK) {
        return st;
    }
    if ((st = allow_lds(ctx, kernel, lds)) != GBL_OK) return st;
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(wgs)), dim3(GBL_BLOCK), lds, stream, sc, qa);
    HIP_TRY(ctx, hipGetLastError());
    return GBL_OK;
}

// sync: the self-test hook's synchronise behind the launch
gbl_status trace_rays_impl(gbl_ctx* ctx, const char* who_c, uint32_t kind, const gbl_ray* d_rays, uint64_t n, void* d_out, uint32_t flags, uint32_t max_workgroups,
                           hipStream_t stream, bool sync) {
    if (!ctx) return GBL_ERR_INVALID;
    const std::string who = who_c;
    if (kind != GBL_QUERY_CLOSEST && kind != GBL_QUERY_ANY) return fail(ctx, GBL_ERR_INVALID, who + ": unknown kind " + std::to_string(kind));
    if ((flags & ~(GBL_QUERY_EXACT_TIES | GBL_QUERY_SHADING_NORMAL)) != 0u) return fail(ctx, GBL_ERR_INVALID, who + ": unknown bits in flags");
    const bool any = kind == GBL_QUERY_ANY, ties = (flags & GBL_QUERY_EXACT_TIES) != 0u, normal = (flags & GBL_QUERY_SHADING_NORMAL) != 0u;
    if (any && normal) return fail(ctx, GBL_ERR_INVALID, who + ": GBL_QUERY_SHADING_NORMAL needs GBL_QUERY_CLOSEST: an any-hit query has no hit to shade");
    if (n == 0) return GBL_OK;
    gbl_status st = check_query_buffers(ctx, who, d_rays, n, d_out, any ? 1 : sizeof(gbl_ray_hit));
    if (st != GBL_OK) return st;
    if ((st = launch_unfiltered(ctx, who, any, ties, normal, d_rays, n, d_out, max_workgroups, stream)) != GBL_OK) return st;
    if (sync) HIP_TRY(ctx, hipDeviceSynchronize());
    return GBL_OK;
}

// gbl_trace_rays_filtered.  What runs: the unfiltered kernels for GBL_QUERY_FILTER_NONE and for every query of a scene without
// masks (OPAQUE is NONE there, MASK a fill, TRANSMITTANCE the any-hit answer rewritten); else query_filtered_trace.
gbl_status trace_rays_filtered_impl(gbl_ctx* ctx, const char* who_c, uint32_t kind, uint32_t filter, const gbl_ray* d_rays, uint64_t n, void* d_out, uint32_t flags,
                                    uint32_t max_workgroups, hipStream_t stream, bool sync) {
    if (!ctx) return GBL_ERR_INVALID;
    const std::string who = who_c;
    if (kind != GBL_QUERY_CLOSEST && kind != GBL_QUERY_ANY && kind != GBL_QUERY_TRANSMITTANCE)
        return fail(ctx, GBL_ERR_INVALID, who + ": unknown kind " + std::to_string(kind));
    if (filter != GBL_QUERY_FILTER_NONE && filter != GBL_QUERY_FILTER_OPAQUE && filter != GBL_QUERY_FILTER_MASK)
        return fail(ctx, GBL_ERR_INVALID, who + ": unknown filter " + std::to_string(filter));
    if ((flags & ~(GBL_QUERY_EXACT_TIES | GBL_QUERY_SHADING_NORMAL)) != 0u) return fail(ctx, GBL_ERR_INVALID, who + ": unknown bits in flags");
    const bool any = kind == GBL_QUERY_ANY, transmit = kind == GBL_QUERY_TRANSMITTANCE;
    const bool ties = (flags & GBL_QUERY_EXACT_TIES) != 0u, normal = (flags & GBL_QUERY_SHADING_NORMAL) != 0u;
    if (any && normal) return fail(ctx, GBL_ERR_INVALID, who + ": GBL_QUERY_SHADING_NORMAL needs GBL_QUERY_CLOSEST: an any-hit query has no hit to shade");
    if (transmit && normal) return fail(ctx, GBL_ERR_INVALID, who + ": GBL_QUERY_SHADING_NORMAL needs GBL_QUERY_CLOSEST: a transmittance query reports no hit");
    if (transmit && filter != GBL_QUERY_FILTER_NONE)
        return fail(ctx, GBL_ERR_INVALID, who + ": GBL_QUERY_TRANSMITTANCE takes GBL_QUERY_FILTER_NONE: it filters by itself");
    if (n == 0) return GBL_OK;
    gbl_status st = check_query_buffers(ctx, who, d_rays, n, d_out, transmit ? sizeof(gbl_ray_transmittance) : any ? 1 : sizeof(gbl_ray_hit));
    if (st != GBL_OK) return st;

    const DevScene& sc = ctx->scene;
    const uint32_t n32 = static_cast<uint32_t>(n);
    if (!transmit && (filter == GBL_QUERY_FILTER_NONE || (filter == GBL_QUERY_FILTER_OPAQUE && sc.has_masks == 0))) {
        st = launch_unfiltered(ctx, who, any, ties, normal, d_rays, n, d_out, max_workgroups, stream);
    } else if (sc.has_masks == 0 && !transmit) {   // GBL_QUERY_FILTER_MASK and no mask to meet: every ray misses
        if (any) HIP_TRY(ctx, hipMemsetAsync(d_out, 0, n, stream));
        else gbl_launch_query_fill_miss(static_cast<float4*>(d_out), n32, stream);
        HIP_TRY(ctx, hipGetLastError());
    } else if (sc.has_masks == 0) {   // nothing attenuates: occluded or clear
        if ((st = grow(ctx, ctx->query_any, n, "any-hit bytes of a transmittance query")) != GBL_OK) return st;
        uint8_t* bytes = static_cast<uint8_t*>(ctx->query_any.p);
        if ((st = launch_unfiltered(ctx, who, true, ties, false, d_rays, n, bytes, max_workgroups, stream)) != GBL_OK) return st;
        gbl_launch_query_any_to_transmittance(bytes, static_cast<float4*>(d_out), n32, stream);
        HIP_TRY(ctx, hipGetLastError());
    } else {
        // the walk's closest-hit queries are trace()'s, which follows the tie rule whatever the flag says: they read tri_order
        if ((st = make_orders_if(ctx, ties || transmit)) != GBL_OK) return st;
        gbl_query_filtered_kernel kernel = gbl_kernel_query_filtered(kind, ties, normal);
        if (!kernel) return fail(ctx, GBL_ERR_UNSUPPORTED, who + ": query kernel variant not built");
        if ((st = ensure_mesh_offsets(ctx)) != GBL_OK) return st;
        FilteredQueryArgs fa;
        memset(&fa, 0, sizeof(fa));
        fa.q.rays = reinterpret_cast<const float4*>(d_rays);
        fa.q.hits = kind == GBL_QUERY_CLOSEST ? static_cast<float4*>(d_out) : nullptr;
        fa.q.occluded = any ? static_cast<uint8_t*>(d_out) : nullptr;
        fa.q.mesh_tri_offset = ctx->d_mesh_tri_offset;
        fa.q.n = n32;
        fa.transmittance = transmit ? static_cast<float4*>(d_out) : nullptr;
        fa.filter = filter == GBL_QUERY_FILTER_OPAQUE ? GBL_FILTER_OPAQUE : GBL_FILTER_MASK;
        size_t lds = 0;
        uint64_t wgs = 0;
        if ((st = persistent_layout(ctx, reinterpret_cast<const void*>(kernel), n, max_workgroups, fa.q, &lds, &wgs)) != GBL_OK) return st;
        if ((st = allow_lds(ctx, kernel, lds)) != GBL_OK) return st;
        hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(wgs)), dim3(GBL_BLOCK), lds, stream, sc, fa);
        HIP_TRY(ctx, hipGetLastError());
    }
    if (st != GBL_OK) return st;
    if (sync) HIP_TRY(ctx, hipDeviceSynchronize());
    return GBL_OK;
}

}   // namespace

extern "C" {

gbl_status gbl_trace_rays(gbl_ctx* ctx, uint32_t kind, const gbl_ray* d_rays, uint64_t n, void* d_out, uint32_t flags, void* stream) {
    return gbl_guard([&] { return trace_rays_impl(ctx, "gbl_trace_rays", kind, d_rays, n, d_out, flags, 0, static_cast<hipStream_t>(stream), false); },
                     [&](const std::string& what) { if (ctx) ctx->error = what; });
}

gbl_status gbl_selftest_query(gbl_ctx* ctx, uint32_t kind, const gbl_ray* d_rays, uint64_t n, void* d_out, uint32_t flags, uint32_t max_workgroups) {
    return gbl_guard([&] { return trace_rays_impl(ctx, "gbl_selftest_query", kind, d_rays, n, d_out, flags, max_workgroups, nullptr, true); },
                     [&](const std::string& what) { if (ctx) ctx->error = what; });
}

gbl_status gbl_trace_rays_filtered(gbl_ctx* ctx, uint32_t kind, uint32_t filter, const gbl_ray* d_rays, uint64_t n, void* d_out, uint32_t flags, void* stream) {
    return gbl_guard([&] { return trace_rays_filtered_impl(ctx, "gbl_trace_rays_filtered", kind, filter, d_rays, n, d_out, flags, 0, static_cast<hipStream_t>(stream), false); },
                     [&](const std::string& what) { if (ctx) ctx->error = what; });
}

gbl_status gbl_selftest_query_filtered(gbl_ctx* ctx, uint32_t kind, uint32_t filter, const gbl_ray* d_rays, uint64_t n, void* d_out, uint32_t flags,
                                       uint32_t max_workgroups) {
    return gbl_guard([&] { return trace_rays_filtered_impl(ctx, "gbl_selftest_query_filtered", kind, filter, d_rays, n, d_out, flags, max_workgroups, nullptr, true); },
                     [&](const std::string& what) { if (ctx) ctx->error = what; });
}

}   // extern "C"
