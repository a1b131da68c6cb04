// libgoblin_hip.so -- C ABI of the device integrator (include/goblin_hip.h): gbl_render_aov, the first-hit feature pass
// (kernels/aov.h) and one wf_splat per requested film, a chunk of the samples per pixel at a time; and the depth film's resolve.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <string>

#include "gbl_host.h"

namespace {

struct AovKnobs {
    bool packet;     // GBL_AOV_PACKET=0: one ray per lane also where the packet kernel applies (A/B, bit-identity test)
    int pass_spp;    // GBL_AOV_PASS_SPP: at most this many samples per pixel per chunk (tests: force several chunks); 0: the budget's
};
AovKnobs read_aov_knobs() {
    AovKnobs k;
    const char* e = getenv("GBL_AOV_PACKET");
    k.packet = e == nullptr || e[0] != '0';
    e = getenv("GBL_AOV_PASS_SPP");
    k.pass_spp = e ? std::max(0, atoi(e)) : 0;
    return k;
}

// The plan of the call's camera samples (plan_samples) and none of the integrators' checks and budgets
gbl_status plan_aov(gbl_ctx* ctx, const gbl_render_params* p, SamplePlan* pl) {
    if (p->sample_mode == GBL_SAMPLES_STREAM)
        return fail(ctx, GBL_ERR_UNSUPPORTED, "gbl_render_aov: the image positions of GBL_SAMPLES_STREAM depend on the draws Li makes");
    const gbl_status st = plan_samples(ctx, p, false, pl);
    if (st != GBL_OK) return st;
    pl->ra.chunks = 1;   // (the integrator and depth fields of the layout only size the replay record)
    pl->ra.chunk_spp = pl->ra.spp;
    if (stack_lds_bytes(ctx->scene) > 160 * 1024) return fail(ctx, GBL_ERR_UNSUPPORTED, "scene's BVH is too deep for the LDS traversal stacks");
    return GBL_OK;
}

gbl_status gbl_render_aov_impl(gbl_ctx* ctx, const gbl_render_params* p, const gbl_aov_targets* tg, gbl_stats* stats, const AovKnobs& knobs) {
    if (!ctx) return GBL_ERR_INVALID;
    if (!p || !tg) return fail(ctx, GBL_ERR_INVALID, "null argument");
    if (!tg->albedo_accum && !tg->normal_accum && !tg->depth_accum && !tg->samples_out)
        return fail(ctx, GBL_ERR_INVALID, "gbl_render_aov: every target is NULL");
    SamplePlan pl;
    gbl_status st = plan_aov(ctx, p, &pl);
    if (st != GBL_OK) return st;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (pl.ra.local_tiles == 0 || pl.entries == 0) return GBL_OK;
    const DevScene& sc = ctx->scene;
    RenderArgs ra = pl.ra;
    hipStream_t stream = static_cast<hipStream_t>(p->stream);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (pl.want_stats) HIP_TRY(ctx, hipMemsetAsync(ctx->stats, 0, 32 * sizeof(unsigned long long), stream));

    // a chunk's planes: 16 bytes per sample and requested film, inside the per-sample budget gbl_render keeps to
    float* const films[3] = {tg->albedo_accum, tg->normal_accum, tg->depth_accum};
    const int n_films = (films[0] ? 1 : 0) + (films[1] ? 1 : 0) + (films[2] ? 1 : 0);
    int pass_spp = ra.spp;
    if (n_films > 0) {
        const uint64_t per_spp = pl.npix * sizeof(float4) * n_films;
        pass_spp = static_cast<int>(std::max<uint64_t>(1, std::min<uint64_t>(ra.spp, li_budget_bytes(ctx) / per_spp)));
    }
    if (knobs.pass_spp > 0) pass_spp = std::min(pass_spp, knobs.pass_spp);
    float4* planes[3] = {nullptr, nullptr, nullptr};
    if (n_films > 0) {
        const uint64_t plane = pl.npix * static_cast<uint64_t>(pass_spp);
        if ((st = grow(ctx, ctx->aov, plane * sizeof(float4) * n_films, "feature planes")) != GBL_OK) return st;
        float4* q = static_cast<float4*>(ctx->aov.p);
        for (int f = 0; f < 3; ++f)
            if (films[f]) {
                planes[f] = q;
                q += plane;
            }
    }
    // Kernel: packets for the lean scenes under the native sampler (see aov_packet_kernel), one ray per lane otherwise.  The
    // EXT build wherever gbl_render takes one -- feature scenes, replay, instrumented calls -- and with it the tie rule.
    const bool ext = sc.extended != 0 || pl.replay || pl.want_stats;
    const bool packet = !ext && knobs.packet && sc.stack_entries <= 64;   // (kernels/packet.h GBL_PACKET_STACK, as primary_pass)
    gbl_aov_kernel kernel = packet ? gbl_kernel_aov_packet(p->exact_ties != 0) : gbl_kernel_aov(pl.replay, pl.want_stats, ext, p->exact_ties != 0);
    // (every EXT build and both exact_ties builds read tri_order; the two lean ones leave a deferred vertex edit's tie order pending)
    if ((st = make_orders_if(ctx, ext || p->exact_ties != 0)) != GBL_OK) return st;
    const size_t lds = stack_lds_bytes(sc);
    if ((st = allow_lds(ctx, kernel, lds + (packet ? 4096 : 0))) != GBL_OK) return st;   // (the packet kernel's static 3 KB count against the same limit)
    if (stats) HIP_TRY(ctx, hipEventRecord(ctx->ev0, stream));
    for (int k0 = 0; k0 < ra.spp; k0 += pass_spp) {
        AovArgs aa;
        aa.albedo = planes[0];
        aa.normal = planes[1];
        aa.depth = planes[2];
        aa.samples = tg->samples_out;
        aa.pass_k0 = k0;
        aa.pass_spp = std::min(pass_spp, ra.spp - k0);
        const uint64_t threads = packet ? static_cast<uint64_t>(ra.local_tiles) * 64 * ((aa.pass_spp + 63) / 64) * 64
                                        : static_cast<uint64_t>(ra.local_tiles) * 64 * aa.pass_spp;
        const uint64_t cap = static_cast<uint64_t>(ctx->num_cus) * (packet ? 64 : 8);   // grid-stride (the primary pass's grid: 64 workgroups per CU)
        const dim3 grid(static_cast<unsigned>(std::max<uint64_t>(1, std::min<uint64_t>((threads + GBL_BLOCK - 1) / GBL_BLOCK, cap))));
        hipLaunchKernelGGL(kernel, grid, dim3(GBL_BLOCK), lds, stream, sc, ra, aa);
        HIP_TRY(ctx, hipGetLastError());
        for (int f = 0; f < 3; ++f) {
            if (!films[f]) continue;
            ra.film = films[f];
            if ((st = launch_splat(ctx, ra, planes[f], k0, aa.pass_spp, pl.replay, pl.want_stats, stream)) != GBL_OK) return st;
        }
    }
    if (!stats) return GBL_OK;
    unsigned long long h[32];
    if ((st = close_call(ctx, pl, stream, stats, h)) != GBL_OK) return st;
    stats->extension_rays = stats->paths;
    if (pl.want_stats) {
        stats->nodes = h[3];
        stats->tris = h[4];
        stats->splats = h[5];
    }
    return GBL_OK;
}

}   // namespace

extern "C" {

gbl_status gbl_render_aov(gbl_ctx* ctx, const gbl_render_params* params, const gbl_aov_targets* targets, gbl_stats* stats) {
    return gbl_guard([&] { return gbl_render_aov_impl(ctx, params, targets, stats, read_aov_knobs()); }, [&](const std::string& what) { if (ctx) ctx->error = what; });
}

static gbl_status gbl_aov_resolve_depth_impl(gbl_ctx* ctx, const float* depth_accum, float* depth_out, float* coverage_out, void* stream) {
    if (!ctx || !depth_accum || !depth_out) return GBL_ERR_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    gbl_launch_aov_resolve_depth(depth_accum, depth_out, coverage_out, ctx->info.xres * ctx->info.yres, static_cast<hipStream_t>(stream));
    HIP_TRY(ctx, hipGetLastError());
    return GBL_OK;
}
gbl_status gbl_aov_resolve_depth(gbl_ctx* ctx, const float* depth_accum, float* depth_out, float* coverage_out, void* stream) {
    return gbl_guard([&] { return gbl_aov_resolve_depth_impl(ctx, depth_accum, depth_out, coverage_out, stream); }, [&](const std::string& what) { if (ctx) ctx->error = what; });
}

}  // extern "C"
