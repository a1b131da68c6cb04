// libgoblin_hip.so -- C ABI of the device integrator (include/goblin_hip.h): what happens to a film after the render calls --
// gbl_film_resolve, gbl_film_develop and the RCCL reduce of gbl_film_allreduce.
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "gbl_host.h"

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
