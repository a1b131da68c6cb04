// libgoblin_hip.so -- C ABI of the device integrator (include/goblin_hip.h): gbl_radiance_rays, path-traced radiance along rays in
// device memory (kernels/radiance.h), and its self-test hook, the same call with its persistent grid capped.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>

#include "gbl_host.h"

namespace {

// sync: the self-test hook's synchronise behind the launch
gbl_status radiance_rays_impl(gbl_ctx* ctx, const char* who_c, const gbl_ray* d_rays, uint64_t n, const gbl_radiance_params* p, float* d_out, uint32_t max_workgroups,
                              bool sync) {
    if (!ctx) return GBL_ERR_INVALID;
    const std::string who = who_c;
    if (!p) return fail(ctx, GBL_ERR_INVALID, who + ": null params");
    if (p->reserved != 0u) return fail(ctx, GBL_ERR_INVALID, who + ": reserved must be 0");
    if ((p->flags & ~(GBL_RADIANCE_EXACT_TIES | GBL_RADIANCE_RUSSIAN_ROULETTE)) != 0u) return fail(ctx, GBL_ERR_INVALID, who + ": unknown bits in flags");
    // (above 16384 the 1D pattern numbers 3 b + 2 reach the 2D patterns' base 0x10000)
    if (p->max_ray_depth < 1 || p->max_ray_depth > 16384) return fail(ctx, GBL_ERR_INVALID, who + ": max_ray_depth must lie in [1, 16384]");
    const uint32_t S = p->samples_per_group;
    const uint32_t root = static_cast<uint32_t>(std::lround(std::sqrt(static_cast<double>(S))));
    if (S < 1u || static_cast<uint64_t>(root) * root != S || S > 0x7fffffffu)   // (the sampler keeps the count in an int)
        return fail(ctx, GBL_ERR_INVALID, who + ": samples_per_group must be a perfect square >= 1 (below 2^31)");
    if (n % S != 0u) return fail(ctx, GBL_ERR_INVALID, who + ": n is not a multiple of samples_per_group");
    if (static_cast<uint64_t>(p->first_group) + n / S > (1ull << 32)) return fail(ctx, GBL_ERR_INVALID, who + ": first_group + n / samples_per_group passes 2^32 groups");
    const bool replay = p->d_records != nullptr, rr = (p->flags & GBL_RADIANCE_RUSSIAN_ROULETTE) != 0u;
    if (replay && rr) return fail(ctx, GBL_ERR_INVALID, who + ": GBL_RADIANCE_RUSSIAN_ROULETTE needs native draws: the records hold no roulette draw");
    const DevScene& sc = ctx->scene;
    // the record layout gbl_render replays for the path tracer at this depth in this scene (gbl_host_sample_dimension_scene)
    gbl_render_params rp;
    memset(&rp, 0, sizeof(rp));
    rp.integrator = GBL_INTEGRATOR_PATH;
    rp.sample_per_pixel = static_cast<int32_t>(S);
    rp.max_ray_depth = p->max_ray_depth;
    rp.bssrdf_sample_num = ctx->h_setting.bssrdf_sample_num;
    rp.ao_sample_num = 1;
    RenderArgs layout;
    memset(&layout, 0, sizeof(layout));
    sample_layout(sc, &rp, layout);
    if (replay && p->record_stride != static_cast<uint32_t>(layout.dims))
        return fail(ctx, GBL_ERR_INVALID, who + ": record_stride is " + std::to_string(p->record_stride) + ", the path tracer's record at this max_ray_depth holds " +
                                              std::to_string(layout.dims) + " floats");
    if (n == 0) return GBL_OK;
    gbl_status st = check_query_buffers(ctx, who, d_rays, n, d_out, 4 * sizeof(float));
    if (st != GBL_OK) return st;
    if (replay) {
        const uint64_t rec_bytes = n * p->record_stride * sizeof(float);
        if ((st = check_device_pointer(ctx, p->d_records, rec_bytes, who, "d_records")) != GBL_OK) return st;
        if (overlaps(p->d_records, rec_bytes, d_out, n * 4 * sizeof(float))) return fail(ctx, GBL_ERR_INVALID, who + ": d_out overlaps d_records");
    }
    // the medium and Lsubsurface are computed per CAMERA sample by kernels of their own (kernels/volume.h, kernels/subsurface.h):
    // radiance through fog without the fog would be silently wrong
    if (sc.volume.on != 0u) return fail(ctx, GBL_ERR_UNSUPPORTED, who + ": the scene has a participating medium, which only gbl_render integrates");
    if (sc.has_bssrdf != 0) return fail(ctx, GBL_ERR_UNSUPPORTED, who + ": the scene has a subsurface material, whose Lsubsurface only gbl_render computes");

    // Which build, as gbl_render picks the megakernel's: the EXT one for a scene beyond the headline feature set; the tie rule in
    // every replay and EXT build, and in the lean native one where the caller asks for it.  Only that last choice leaves a deferred
    // vertex edit's tie order pending.
    const bool ext = sc.extended != 0;
    const bool ties = replay || ext || (p->flags & GBL_RADIANCE_EXACT_TIES) != 0u;
    if ((st = make_orders_if(ctx, ties)) != GBL_OK) return st;
    gbl_radiance_kernel kernel = gbl_kernel_radiance(replay, ext, ties);
    if (!kernel) return fail(ctx, GBL_ERR_UNSUPPORTED, who + ": radiance kernel variant not built");

    RadianceArgs ra;
    memset(&ra, 0, sizeof(ra));
    ra.rays = reinterpret_cast<const float4*>(d_rays);
    ra.out = reinterpret_cast<float4*>(d_out);
    ra.records = p->d_records;
    ra.n = static_cast<uint32_t>(n);
    ra.max_depth = p->max_ray_depth;
    ra.dims = layout.dims;
    ra.off2_base = layout.off2_base;
    ra.spp = static_cast<int32_t>(S);
    ra.root = static_cast<int32_t>(root);
    ra.first_group = p->first_group;
    ra.seed_key = native_seed_key(p->seed);
    ra.russian_roulette = rr ? 1u : 0u;
    QueryArgs lay;   // the stacks' backing and LDS layout, as the query kernels take them
    memset(&lay, 0, sizeof(lay));
    size_t lds = 0;
    uint64_t wgs = 0;
    if ((st = persistent_layout(ctx, reinterpret_cast<const void*>(kernel), n, max_workgroups, lay, &lds, &wgs)) != GBL_OK) return st;
    ra.stack_spill = lay.stack_spill;
    ra.hot_word = lay.hot_word;
    ra.hot_count = lay.hot_count;
    if ((st = allow_lds(ctx, kernel, lds)) != GBL_OK) return st;
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(wgs)), dim3(GBL_BLOCK), lds, static_cast<hipStream_t>(p->stream), sc, ra);
    HIP_TRY(ctx, hipGetLastError());
    if (sync) HIP_TRY(ctx, hipDeviceSynchronize());
    return GBL_OK;
}

}   // namespace

extern "C" {

gbl_status gbl_radiance_rays(gbl_ctx* ctx, const gbl_ray* d_rays, uint64_t n, const gbl_radiance_params* params, float* d_out) {
    return gbl_guard([&] { return radiance_rays_impl(ctx, "gbl_radiance_rays", d_rays, n, params, d_out, 0, false); },
                     [&](const std::string& what) { if (ctx) ctx->error = what; });
}

gbl_status gbl_selftest_radiance(gbl_ctx* ctx, const gbl_ray* d_rays, uint64_t n, const gbl_radiance_params* params, float* d_out, uint32_t max_workgroups) {
    return gbl_guard([&] { return radiance_rays_impl(ctx, "gbl_selftest_radiance", d_rays, n, params, d_out, max_workgroups, true); },
                     [&](const std::string& what) { if (ctx) ctx->error = what; });
}

}   // extern "C"
