// libgoblin_hip.so -- C ABI of the device integrator (include/goblin_hip.h): image edits.
// gbl_update_image_device / gbl_update_image give one image of the texel pool a new level 0 -- from device memory, or from the
// caller's host memory -- and build the levels above it on the device (kernels/pyramid.h), one launch per level, so that the
// image's texels equal what gbl_create uploads for a description whose pyramid csrc/host/mipmap.cpp built from that level 0, bit
// for bit.  resizeImage's tap tables depend on the level sizes only: the host makes them at the image's first edit with the
// function the loader makes them with (csrc/host/mipmap_taps.h) and the context keeps them on the device.  Nothing is
// synchronised.  gbl_get_image reads a record and a pyramid back.  The copy and the launches are one function,
// queue_image_pyramid, which the environment edits (api_environment.hip) queue as well.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "gbl_host.h"
#include "host/mipmap_taps.h"

namespace {

uint32_t level_side(uint32_t side, uint32_t level) { return std::max(1u, side >> level); }
uint64_t level_floats(const gbl_image& gi, uint32_t level) { return static_cast<uint64_t>(level_side(gi.width, level)) * level_side(gi.height, level) * gi.channels; }
uint64_t pyramid_floats(const gbl_image& gi) {
    uint64_t floats = 0;
    for (uint32_t l = 0; l < gi.levels; ++l) floats += level_floats(gi, l);
    return floats;
}

// The image's tap tables, made at its first edit: per level l >= 1 the taps of resize_image(level l - 1 -> level l), uploaded on
// `stream`.  An edit queued on another stream later waits for that upload through the event recorded behind it.
gbl_status ensure_taps(gbl_ctx* ctx, uint32_t image, const char* who, hipStream_t stream) {
    gbl_ctx::ImageTaps& taps = ctx->image_taps[image];
    if (taps.built) return GBL_OK;
    const gbl_image& gi = ctx->h_images[image];
    std::vector<uint32_t> words;
    std::vector<gbl_ctx::ImageTaps::Level> levels;
    for (uint32_t l = 1; l < gi.levels; ++l) {
        const int sw = static_cast<int>(level_side(gi.width, l - 1)), sh = static_cast<int>(level_side(gi.height, l - 1));
        const int dw = static_cast<int>(level_side(gi.width, l)), dh = static_cast<int>(level_side(gi.height, l));
        const float filter_width = gbl_host_detail::resize_filter_width(sw, sh, dw, dh);
        const int n = gbl_host_detail::floor_int(filter_width) * 2;
        std::vector<float> s_weight(static_cast<size_t>(dw) * n), t_weight(static_cast<size_t>(dh) * n);
        std::vector<int> s_index(dw), t_index(dh);
        gbl_host_detail::resize_taps(dw, sw, filter_width, n, s_weight.data(), s_index.data());
        gbl_host_detail::resize_taps(dh, sh, filter_width, n, t_weight.data(), t_index.data());
        gbl_ctx::ImageTaps::Level at;
        at.n = n;
        const auto append = [&words](const void* p, size_t count) {
            const uint32_t first = static_cast<uint32_t>(words.size());
            words.resize(words.size() + count);
            memcpy(words.data() + first, p, count * sizeof(uint32_t));
            return first;
        };
        at.s_weight = append(s_weight.data(), s_weight.size());
        at.t_weight = append(t_weight.data(), t_weight.size());
        at.s_index = append(s_index.data(), s_index.size());
        at.t_index = append(t_index.data(), t_index.size());
        levels.push_back(at);
    }
    if (!words.empty()) {
        hipEvent_t uploaded = nullptr;
        HIP_TRY(ctx, hipEventCreateWithFlags(&uploaded, hipEventDisableTiming));
        void* d = nullptr;
        const gbl_status st = device_alloc(ctx, words.size() * sizeof(uint32_t), (std::string(who) + ": tap tables").c_str(), &d);
        if (st != GBL_OK) {
            (void)hipEventDestroy(uploaded);
            return st;
        }
        taps.d_words = static_cast<uint32_t*>(d);
        taps.uploaded = uploaded;
        taps.h_words.swap(words);   // the context's, so the source outlives the call
        HIP_TRY(ctx, hipMemcpyAsync(taps.d_words, taps.h_words.data(), taps.h_words.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        HIP_TRY(ctx, hipEventRecord(taps.uploaded, stream));
    }
    taps.levels.swap(levels);
    taps.built = true;
    return GBL_OK;
}

}   // namespace

// (gbl_host.h) What both image edits and both environment edits queue: the tap tables at the image's first edit, level 0's copy,
// then one launch per level above it
gbl_status queue_image_pyramid(gbl_ctx* ctx, uint32_t image, const float* level0, bool on_device, hipStream_t stream, const char* who) {
    const gbl_image& gi = ctx->h_images[image];
    gbl_status st = GBL_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((st = ensure_taps(ctx, image, who, stream)) != GBL_OK) return st;
    const gbl_ctx::ImageTaps& taps = ctx->image_taps[image];
    float* const texels = const_cast<float*>(ctx->scene.texels) + gi.texel_offset;
    // (a pageable source is read before the copy call returns, as gbl_render_motion's table is)
    HIP_TRY(ctx, hipMemcpyAsync(texels, level0, level_floats(gi, 0) * sizeof(float), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
    if (taps.uploaded) HIP_TRY(ctx, hipStreamWaitEvent(stream, taps.uploaded, 0));
    uint64_t src = 0;
    for (uint32_t l = 1; l < gi.levels; ++l) {   // level l reads what the launch before it wrote
        const gbl_ctx::ImageTaps::Level& at = taps.levels[l - 1];
        const uint64_t dst = src + level_floats(gi, l - 1);
        PyramidArgs a;
        a.src = texels + src;
        a.dst = texels + dst;
        a.s_weight = reinterpret_cast<const float*>(taps.d_words + at.s_weight);
        a.t_weight = reinterpret_cast<const float*>(taps.d_words + at.t_weight);
        a.s_index = reinterpret_cast<const int32_t*>(taps.d_words + at.s_index);
        a.t_index = reinterpret_cast<const int32_t*>(taps.d_words + at.t_index);
        a.sw = static_cast<int32_t>(level_side(gi.width, l - 1)), a.sh = static_cast<int32_t>(level_side(gi.height, l - 1));
        a.dw = static_cast<int32_t>(level_side(gi.width, l)), a.dh = static_cast<int32_t>(level_side(gi.height, l));
        a.n = at.n;
        a.channels = static_cast<int32_t>(gi.channels);
        gbl_launch_pyramid_level(a, stream);
        src = dst;
    }
    HIP_TRY(ctx, hipGetLastError());
    return GBL_OK;
}

namespace {

// The image based light that reads the image, or -1
int ibl_reader(const gbl_ctx* ctx, uint32_t image) {
    for (size_t i = 0; i < ctx->h_lights.size(); ++i)
        if (ctx->h_lights[i].type == GBL_LIGHT_IBL && ctx->h_lights[i].image == static_cast<int32_t>(image)) return static_cast<int>(i);
    return -1;
}

gbl_status gbl_update_image_impl(gbl_ctx* ctx, uint32_t image, const float* level0, bool on_device, void* stream_, const char* who) {
    if (!ctx) return GBL_ERR_INVALID;
    const char* const what = on_device ? "d_level0" : "level0";
    // arguments, range, the pointer, the image based lights: nothing is queued or kept before the last of them
    if (!level0) return fail(ctx, GBL_ERR_INVALID, std::string(who) + ": " + what + " is NULL");
    if (image >= ctx->h_images.size())
        return fail(ctx, GBL_ERR_INVALID, std::string(who) + ": image " + std::to_string(image) + " out of range (the context holds " + std::to_string(ctx->h_images.size()) + ")");
    const gbl_image& gi = ctx->h_images[image];
    const uint64_t bytes0 = level_floats(gi, 0) * sizeof(float);
    gbl_status st = GBL_OK;
    if (on_device) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        if ((st = check_device_pointer(ctx, level0, bytes0, who, what)) != GBL_OK) return st;
    }
    if (const int light = ibl_reader(ctx, image); light >= 0)
        return fail(ctx, GBL_ERR_UNSUPPORTED, std::string(who) + ": image " + std::to_string(image) + " is read by image based light " + std::to_string(light) +
                                              ", whose sampling distribution, average radiance and power are packed from its texels when the context is created; "
                                              "re-create the context instead");
    if ((st = queue_image_pyramid(ctx, image, level0, on_device, static_cast<hipStream_t>(stream_), who)) != GBL_OK) return st;
    ctx->auto_rays_per_path.clear();   // a mask's alpha may be read from an image: AUTO measures its rays per path again
    return GBL_OK;
}

gbl_status gbl_get_image_impl(gbl_ctx* ctx, uint32_t image, gbl_image* info_out, float* texels_out) {
    if (!ctx || image >= ctx->h_images.size() || (!info_out && !texels_out)) return GBL_ERR_INVALID;
    const gbl_image& gi = ctx->h_images[image];
    if (texels_out) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        HIP_TRY(ctx, hipDeviceSynchronize());
        HIP_TRY(ctx, hipMemcpy(texels_out, ctx->scene.texels + gi.texel_offset, pyramid_floats(gi) * sizeof(float), hipMemcpyDeviceToHost));
    }
    if (info_out) {
        *info_out = gi;
        info_out->texel_offset = 0;   // counted from the start of texels_out
    }
    return GBL_OK;
}

}   // namespace

extern "C" {

gbl_status gbl_update_image_device(gbl_ctx* ctx, uint32_t image, const float* d_level0, void* stream) {
    return gbl_guard([&] { return gbl_update_image_impl(ctx, image, d_level0, true, stream, "gbl_update_image_device"); },
                     [&](const std::string& what) { if (ctx) ctx->error = what; });
}

gbl_status gbl_update_image(gbl_ctx* ctx, uint32_t image, const float* level0, void* stream) {
    return gbl_guard([&] { return gbl_update_image_impl(ctx, image, level0, false, stream, "gbl_update_image"); },
                     [&](const std::string& what) { if (ctx) ctx->error = what; });
}

gbl_status gbl_get_image(gbl_ctx* ctx, uint32_t image, gbl_image* info_out, float* texels_out) {
    return gbl_guard([&] { return gbl_get_image_impl(ctx, image, info_out, texels_out); }, [&](const std::string& what) { if (ctx) ctx->error = what; });
}

}   // extern "C"
