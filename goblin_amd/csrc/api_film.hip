// libgoblin_hip.so -- C ABI of the device integrator (include/goblin_hip.h): what happens to a film after the render calls --
// gbl_film_resolve, gbl_film_develop, gbl_film_variance, gbl_film_denoise, gbl_film_accumulate, gbl_film_accumulate_motion and the RCCL reduce of
// gbl_film_allreduce.
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>

#include "gbl_host.h"
#include "scene_prep.h"

extern "C" {

static gbl_status gbl_film_resolve_impl(gbl_ctx* ctx, const float* film_accum, float* rgb_out, void* stream) {
    if (!ctx || !film_accum || !rgb_out) return GBL_ERR_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int n = ctx->info.xres * ctx->info.yres;
    gbl_launch_film_resolve(film_accum, rgb_out, n, static_cast<hipStream_t>(stream));
    HIP_TRY(ctx, hipGetLastError());
    return GBL_OK;
}
gbl_status gbl_film_resolve(gbl_ctx* ctx, const float* film_accum, float* rgb_out, void* stream) {
    return gbl_guard([&] { return gbl_film_resolve_impl(ctx, film_accum, rgb_out, stream); }, [&](const std::string& what) { if (ctx) ctx->error = what; });
}

// Film::writeImage's tail (GoblinFilm.cpp:164-192 + Goblin::writeImage, GoblinImageIO.cpp:146-237) in passes on one stream:
// normalise, bloom, tone map, quantise (kernels/develop.h).  Nothing comes back to the host.
static gbl_status gbl_film_develop_impl(gbl_ctx* ctx, const float* film_accum, const gbl_develop_params* p, float* rgb_out, uint8_t* rgb8_out) {
    if (!ctx || !film_accum || !p || (!rgb_out && !rgb8_out)) return GBL_ERR_INVALID;
    if (rgb_out == film_accum) {
        ctx->error = "gbl_film_develop: rgb_out may not alias film_accum";
        return GBL_ERR_INVALID;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int width = ctx->info.xres, height = ctx->info.yres, n = width * height;
    hipStream_t stream = static_cast<hipStream_t>(p->stream);
    gbl_status st;
    float* rgb = rgb_out;
    if (!rgb) {
        if ((st = grow(ctx, ctx->dev_rgb, static_cast<uint64_t>(n) * 3 * sizeof(float), "developed image")) != GBL_OK) return st;
        rgb = static_cast<float*>(ctx->dev_rgb.p);
    }
    int fw = 0;   // Goblin::bloom's filterWidth; 0 taps: nothing to do (as gbl_host_bloom)
    if (p->bloom_radius > 0.0f && p->bloom_weight > 0.0f) fw = static_cast<int>(std::ceil(p->bloom_radius * std::max(width, height))) / 2;
    if (fw > 0) {
        const int fwx = std::min(fw, width), fwy = std::min(fw, height);
        if ((st = grow(ctx, ctx->dev_rgb1, static_cast<uint64_t>(n) * 4 * sizeof(float), "normalised image")) != GBL_OK) return st;
        if (ctx->dev_filter_fw != fw) {
            ctx->dev_filter_fw = 0;
            if ((st = grow(ctx, ctx->dev_filter, static_cast<uint64_t>(fwx) * fwy * sizeof(float), "bloom filter")) != GBL_OK) return st;
            gbl_launch_bloom_filter(static_cast<float*>(ctx->dev_filter.p), fw, fwx, fwy, stream);
            ctx->dev_filter_fw = fw;
        }
        gbl_launch_develop_resolve(film_accum, static_cast<float*>(ctx->dev_rgb1.p), n, stream);
        gbl_launch_bloom(static_cast<const float*>(ctx->dev_rgb1.p), static_cast<const float*>(ctx->dev_filter.p), rgb, width, height, fw, fwx,
                         p->bloom_weight, stream);
    } else {
        gbl_launch_film_resolve(film_accum, rgb, n, stream);
    }
    if (p->tone_mapping) {
        if ((st = grow(ctx, ctx->dev_logs, (static_cast<uint64_t>(n) + 1) * sizeof(float), "tone map sums")) != GBL_OK) return st;
        float* logs = static_cast<float*>(ctx->dev_logs.p);
        gbl_launch_tone_map(rgb, logs, logs + n, n, stream);
    }
    if (rgb8_out) gbl_launch_quantize(rgb, rgb8_out, 3 * n, stream);
    HIP_TRY(ctx, hipGetLastError());
    return GBL_OK;
}
gbl_status gbl_film_develop(gbl_ctx* ctx, const float* film_accum, const gbl_develop_params* params, float* rgb_out, uint8_t* rgb8_out) {
    return gbl_guard([&] { return gbl_film_develop_impl(ctx, film_accum, params, rgb_out, rgb8_out); }, [&](const std::string& what) { if (ctx) ctx->error = what; });
}

// Variance of the pixel mean from a call's per-sample radiance (kernels/denoise.h film_variance_kernel)
static gbl_status gbl_film_variance_impl(gbl_ctx* ctx, const float* li, const int32_t* window, int32_t sample_per_pixel, float* variance_out, void* stream) {
    if (!ctx) return GBL_ERR_INVALID;
    if (!li || !variance_out) return fail(ctx, GBL_ERR_INVALID, "gbl_film_variance: li and variance_out may not be NULL");
    if (sample_per_pixel < 2) return fail(ctx, GBL_ERR_INVALID, "gbl_film_variance: sample_per_pixel must be >= 2, a variance needs two samples");
    const int root = static_cast<int>(std::ceil(std::sqrt(static_cast<float>(sample_per_pixel))));   // roundToSquare, as gbl_render
    const int32_t* full = ctx->info.window;
    const bool whole = !window || (window[0] == 0 && window[1] == 0 && window[2] == 0 && window[3] == 0);
    int32_t w[4];
    for (int i = 0; i < 4; ++i) w[i] = whole ? full[i] : window[i];
    if (w[0] < full[0] || w[1] > full[1] || w[2] < full[2] || w[3] > full[3] || w[0] > w[1] || w[2] > w[3])
        return fail(ctx, GBL_ERR_INVALID, "gbl_film_variance: window lies outside the film's sample window");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    gbl_launch_film_variance(li, variance_out, w, root * root, ctx->info.xres, ctx->info.yres, static_cast<hipStream_t>(stream));
    HIP_TRY(ctx, hipGetLastError());
    return GBL_OK;
}
gbl_status gbl_film_variance(gbl_ctx* ctx, const float* li, const int32_t window[4], int32_t sample_per_pixel, float* variance_out, void* stream) {
    return gbl_guard([&] { return gbl_film_variance_impl(ctx, li, window, sample_per_pixel, variance_out, stream); }, [&](const std::string& what) { if (ctx) ctx->error = what; });
}

// The a-trous filter (kernels/denoise.h): prepare, one level kernel per iteration between two buffers, finish.
// Which level kernel serves a stride: the one that stages tile and halo in LDS, or the one that taps global memory.  Measured
// per stride at 512^2 and 1024^2: staging wins at strides 1 and 2 (-16 ... -35 % of the level), loses from stride 4
// on, where the halo is most of what is staged, and does not fit a workgroup's LDS from stride 16 on.  GBL_DENOISE_LDS=0 / 1,
// read per call, forces one of them wherever the staged tile fits (A/B, tests).
static bool denoise_level_in_lds(int stride) {
    if (gbl_denoise_lds_bytes(stride) == 0) return false;
    if (const char* e = getenv("GBL_DENOISE_LDS")) return e[0] != '0';
    return stride <= 2;
}
static gbl_status gbl_film_denoise_impl(gbl_ctx* ctx, const float* film_accum, const float* variance, const float* albedo_accum, const float* normal_accum,
                                        const float* depth_accum, const gbl_denoise_params* p, float* film_out) {
    if (!ctx) return GBL_ERR_INVALID;
    if (!film_accum) return fail(ctx, GBL_ERR_INVALID, "gbl_film_denoise: film_accum is NULL");
    if (!p) return fail(ctx, GBL_ERR_INVALID, "gbl_film_denoise: params is NULL");
    if (!film_out) return fail(ctx, GBL_ERR_INVALID, "gbl_film_denoise: film_out is NULL");
    if (p->iterations < 1 || p->iterations > 8) return fail(ctx, GBL_ERR_INVALID, "gbl_film_denoise: iterations must be 1..8, got " + std::to_string(p->iterations));
    const auto bad = [](float s) { return !(s > 0.0f) || !std::isfinite(s); };
    if (bad(p->sigma_luminance)) return fail(ctx, GBL_ERR_INVALID, "gbl_film_denoise: sigma_luminance must be finite and > 0");
    if (normal_accum && bad(p->sigma_normal)) return fail(ctx, GBL_ERR_INVALID, "gbl_film_denoise: sigma_normal must be finite and > 0");
    if (albedo_accum && bad(p->sigma_albedo)) return fail(ctx, GBL_ERR_INVALID, "gbl_film_denoise: sigma_albedo must be finite and > 0");
    if (depth_accum && bad(p->sigma_depth)) return fail(ctx, GBL_ERR_INVALID, "gbl_film_denoise: sigma_depth must be finite and > 0");
    if (p->demodulate && !albedo_accum) return fail(ctx, GBL_ERR_INVALID, "gbl_film_denoise: demodulate needs albedo_accum");
    const int width = ctx->info.xres, height = ctx->info.yres, n = width * height;
    const uint64_t film_bytes = static_cast<uint64_t>(n) * 4 * sizeof(float);
    if (overlaps(film_out, film_bytes, film_accum, film_bytes) || overlaps(film_out, film_bytes, variance, film_bytes / 4) ||
        overlaps(film_out, film_bytes, albedo_accum, film_bytes) || overlaps(film_out, film_bytes, normal_accum, film_bytes) ||
        overlaps(film_out, film_bytes, depth_accum, film_bytes))
        return fail(ctx, GBL_ERR_INVALID, "gbl_film_denoise: film_out may not alias an input");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = static_cast<hipStream_t>(p->stream);
    gbl_status st;
    if ((st = grow(ctx, ctx->denoise, 4 * film_bytes, "denoiser planes")) != GBL_OK) return st;
    float4* cv[2] = {static_cast<float4*>(ctx->denoise.p), static_cast<float4*>(ctx->denoise.p) + n};
    float4* const nz = cv[1] + n;
    float4* const af = nz + n;
    const uint32_t demodulate = p->demodulate ? 1u : 0u;
    gbl_launch_denoise_prepare(film_accum, variance, albedo_accum, normal_accum, depth_accum, cv[0], nz, af, n, demodulate, stream);
    HIP_TRY(ctx, hipGetLastError());
    DenoiseArgs a;
    a.W = width;
    a.H = height;
    a.sigma_l = p->sigma_luminance;
    a.inv_sn2 = normal_accum ? 1.0f / (p->sigma_normal * p->sigma_normal) : 0.0f;
    a.inv_sa2 = albedo_accum ? 1.0f / (p->sigma_albedo * p->sigma_albedo) : 0.0f;
    a.has_var = variance ? 1u : 0u;
    a.demodulate = demodulate;
    int cur = 0;
    for (int level = 0; level < p->iterations; ++level) {
        a.stride = 1 << level;
        a.sz = depth_accum ? p->sigma_depth * static_cast<float>(a.stride) : 0.0f;
        HIP_TRY(ctx, gbl_launch_denoise_level(denoise_level_in_lds(a.stride), cv[cur], nz, af, cv[cur ^ 1], a, stream, &ctx->denoise_lds_allowed));
        cur ^= 1;
    }
    gbl_launch_denoise_finish(cv[cur], af, film_out, n, demodulate, stream);
    HIP_TRY(ctx, hipGetLastError());
    return GBL_OK;
}
gbl_status gbl_film_denoise(gbl_ctx* ctx, const float* film_accum, const float* variance, const float* albedo_accum, const float* normal_accum,
                            const float* depth_accum, const gbl_denoise_params* params, float* film_out) {
    return gbl_guard([&] { return gbl_film_denoise_impl(ctx, film_accum, variance, albedo_accum, normal_accum, depth_accum, params, film_out); },
                     [&](const std::string& what) { if (ctx) ctx->error = what; });
}

// Reprojected temporal accumulation (kernels/temporal.h): prepare the current frame, then one kernel that gathers the history
// and writes every output.  with_motion: gbl_film_accumulate_motion (`who` in the messages) -- the reprojection comes from the
// planes of gbl_render_motion and params->prev_camera is not read.
static gbl_status gbl_film_accumulate_impl(gbl_ctx* ctx, const char* name, bool with_motion, const float* motion, const float* film_accum,
                                           const float* variance, const float* normal_accum, const float* depth_accum,
                                           const float* history_in, float* history_out, const gbl_temporal_params* p, float* film_out,
                                           float* variance_out) {
    if (!ctx) return GBL_ERR_INVALID;
    const std::string who = std::string(name) + ": ";
    if (!film_accum) return fail(ctx, GBL_ERR_INVALID, who + "film_accum is NULL");
    if (!depth_accum) return fail(ctx, GBL_ERR_INVALID, who + "depth_accum is NULL");
    if (!history_out) return fail(ctx, GBL_ERR_INVALID, who + "history_out is NULL");
    if (!p) return fail(ctx, GBL_ERR_INVALID, who + "params is NULL");
    if (!film_out) return fail(ctx, GBL_ERR_INVALID, who + "film_out is NULL");
    if (!std::isfinite(p->alpha_min) || !(p->alpha_min > 0.0f) || p->alpha_min > 1.0f)
        return fail(ctx, GBL_ERR_INVALID, who + "alpha_min must be in (0, 1]");
    if (!std::isfinite(p->max_history) || !(p->max_history >= 1.0f)) return fail(ctx, GBL_ERR_INVALID, who + "max_history must be finite and >= 1");
    if (!std::isfinite(p->sigma_depth) || !(p->sigma_depth > 0.0f)) return fail(ctx, GBL_ERR_INVALID, who + "sigma_depth must be finite and > 0");
    if (normal_accum && (!std::isfinite(p->cos_normal) || p->cos_normal < -1.0f || p->cos_normal > 1.0f))
        return fail(ctx, GBL_ERR_INVALID, who + "cos_normal must be in [-1, 1]");
    if (with_motion && !motion) return fail(ctx, GBL_ERR_INVALID, who + "motion is NULL");
    if (!with_motion && history_in && p->prev_camera.type > GBL_CAMERA_ORTHOGRAPHIC)
        return fail(ctx, GBL_ERR_INVALID, who + "prev_camera.type: unknown camera type");
    const int width = ctx->info.xres, height = ctx->info.yres, n = width * height;
    const uint64_t film_bytes = static_cast<uint64_t>(n) * 4 * sizeof(float), plane_bytes = film_bytes / 4;
    const uint64_t history_bytes = static_cast<uint64_t>(n) * GBL_HISTORY_FLOATS_PER_PIXEL * sizeof(float);
    if (overlaps(history_out, history_bytes, history_in, history_bytes))
        return fail(ctx, GBL_ERR_INVALID, who + "history_out may not overlap history_in (the gather reads neighbours)");
    const struct { const void* p; uint64_t bytes; const char* name; } outs[3] = {{film_out, film_bytes, "film_out"}, {variance_out, plane_bytes, "variance_out"},
                                                                                  {history_out, history_bytes, "history_out"}},
        ins[6] = {{film_accum, film_bytes, "film_accum"}, {variance, plane_bytes, "variance"}, {normal_accum, film_bytes, "normal_accum"},
                  {depth_accum, film_bytes, "depth_accum"}, {history_in, history_bytes, "history_in"},
                  {motion, static_cast<uint64_t>(n) * GBL_MOTION_FLOATS_PER_PIXEL * sizeof(float), "motion"}};
    for (int o = 0; o < 3; ++o) {
        for (const auto& in : ins)
            if (overlaps(outs[o].p, outs[o].bytes, in.p, in.bytes))
                return fail(ctx, GBL_ERR_INVALID, who + outs[o].name + " may not overlap " + in.name);
        for (int q = o + 1; q < 3; ++q)
            if (overlaps(outs[o].p, outs[o].bytes, outs[q].p, outs[q].bytes))
                return fail(ctx, GBL_ERR_INVALID, who + outs[o].name + " may not overlap " + outs[q].name);
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = static_cast<hipStream_t>(p->stream);
    gbl_status st;
    if ((st = grow(ctx, ctx->temporal, 2 * film_bytes + plane_bytes, "temporal planes")) != GBL_OK) return st;
    float4* const cl = static_cast<float4*>(ctx->temporal.p);
    float4* const nz = cl + n;
    uint32_t* const fl = reinterpret_cast<uint32_t*>(nz + n);
    gbl_launch_temporal_prepare(film_accum, variance, normal_accum, depth_accum, cl, nz, fl, n, stream);
    HIP_TRY(ctx, hipGetLastError());
    TemporalArgs a;
    memset(&a, 0, sizeof(a));
    a.W = width;
    a.H = height;
    a.cur = ctx->scene.camera;
    if (history_in && !with_motion) pack_camera(p->prev_camera, ctx->h_film, &a.prev);
    a.alpha_min = p->alpha_min;
    a.max_history = p->max_history;
    a.sigma_depth = p->sigma_depth;
    a.cos_normal = p->cos_normal;
    a.has_normal = normal_accum ? 1u : 0u;
    a.has_history = history_in ? 1u : 0u;
    if (with_motion)
        gbl_launch_temporal_accumulate_motion(!variance, cl, nz, fl, variance, history_in, history_out, film_out, variance_out, motion, a, stream);
    else
        gbl_launch_temporal_accumulate(!variance, cl, nz, fl, variance, history_in, history_out, film_out, variance_out, a, stream);
    HIP_TRY(ctx, hipGetLastError());
    return GBL_OK;
}
gbl_status gbl_film_accumulate(gbl_ctx* ctx, const float* film_accum, const float* variance, const float* normal_accum, const float* depth_accum,
                               const float* history_in, float* history_out, const gbl_temporal_params* params, float* film_out, float* variance_out) {
    return gbl_guard([&] { return gbl_film_accumulate_impl(ctx, "gbl_film_accumulate", false, nullptr, film_accum, variance, normal_accum, depth_accum,
                                                           history_in, history_out, params, film_out, variance_out); },
                     [&](const std::string& what) { if (ctx) ctx->error = what; });
}
gbl_status gbl_film_accumulate_motion(gbl_ctx* ctx, const float* film_accum, const float* variance, const float* normal_accum, const float* depth_accum,
                                      const float* history_in, float* history_out, const float* motion, const gbl_temporal_params* params, float* film_out,
                                      float* variance_out) {
    return gbl_guard([&] { return gbl_film_accumulate_impl(ctx, "gbl_film_accumulate_motion", true, motion, film_accum, variance, normal_accum, depth_accum,
                                                           history_in, history_out, params, film_out, variance_out); },
                     [&](const std::string& what) { if (ctx) ctx->error = what; });
}

// ncclAllReduce(sum, float) over the film, resolved from librccl at first use so
// single-GPU users never load RCCL.
static gbl_status gbl_film_allreduce_impl(gbl_ctx* ctx, void* rccl_comm, float* film_accum, void* stream) {
    if (!ctx || !rccl_comm || !film_accum) return GBL_ERR_INVALID;
    typedef int (*allreduce_fn)(const void*, void*, size_t, int, int, void*, hipStream_t);
    if (!ctx->rccl_allreduce) {
        ctx->rccl = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!ctx->rccl) ctx->rccl = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!ctx->rccl) {
            ctx->error = std::string("cannot load librccl: ") + dlerror();
            return GBL_ERR_DEVICE;
        }
        ctx->rccl_allreduce = dlsym(ctx->rccl, "ncclAllReduce");
        if (!ctx->rccl_allreduce) {
            ctx->error = "librccl has no ncclAllReduce";
            return GBL_ERR_DEVICE;
        }
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    size_t count = static_cast<size_t>(ctx->info.xres) * ctx->info.yres * 4;
    const int kNcclFloat32 = 7, kNcclSum = 0;
    int rc = reinterpret_cast<allreduce_fn>(ctx->rccl_allreduce)(film_accum, film_accum, count, kNcclFloat32, kNcclSum, rccl_comm,
                                                                 static_cast<hipStream_t>(stream));
    if (rc != 0) {
        ctx->error = "ncclAllReduce failed with code " + std::to_string(rc);
        return GBL_ERR_DEVICE;
    }
    return GBL_OK;
}
gbl_status gbl_film_allreduce(gbl_ctx* ctx, void* rccl_comm, float* film_accum, void* stream) {
    return gbl_guard([&] { return gbl_film_allreduce_impl(ctx, rccl_comm, film_accum, stream); }, [&](const std::string& what) { if (ctx) ctx->error = what; });
}

}  // extern "C"
