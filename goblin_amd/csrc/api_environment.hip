// libgoblin_hip.so -- C ABI of the device integrator (include/goblin_hip.h): environment edits.
// gbl_update_environment_device / gbl_update_environment give the image of one image based light a new level 0 and make again,
// on the device and in stream order, everything gbl_create derives from those texels: the image's pyramid (api_images.hip's
// launches), the light's sampling distribution in DevScene::ibl_dist, its power, and with it light_cdf and light_pick_pdf
// (kernels/environment.h), bit for bit what scene_prep.cpp packs on the host.  sin(theta) per row of the distribution comes from
// the host, through the function pack_ibl_distribution makes it with (scene_prep.h), once per light.  Nothing is synchronised:
// the light's new power, which only the device knows, is copied into pinned memory behind an event, and the host code that
// needs the powers -- gbl_update_lights -- waits for it (settle_environment_power).  DESIGN.md 4.14.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "gbl_host.h"
#include "scene_prep.h"

namespace {

const char* const kLightTypes[] = {"point", "directional", "spot", "area", "image based"};

uint32_t level_side(uint32_t side, uint32_t level) { return std::max(1u, side >> level); }
// Floats of a 4-channel pyramid in front of `level`
uint64_t level_offset(const gbl_image& gi, uint32_t level) {
    uint64_t floats = 0;
    for (uint32_t l = 0; l < level; ++l) floats += static_cast<uint64_t>(level_side(gi.width, l)) * level_side(gi.height, l) * 4;
    return floats;
}
// pack_ibl_distribution's level: neither side of the distribution exceeds 256
uint32_t distribution_level(const gbl_image& gi) { return gi.levels > 9 ? gi.levels - 9 : 0; }

// GBL_ENVIRONMENT_PARTS, a measurement variable asked at every call like GBL_PROBE: a mask of the parts an edit queues (1 the
// copy and the pyramid, 2 func and the rows' CDFs, 4 the tail with the power's read-back); everything when it is not set
unsigned parts_asked() {
    const char* v = getenv("GBL_ENVIRONMENT_PARTS");
    return v ? static_cast<unsigned>(atoi(v)) : 7u;
}

// What the edits keep on the device besides the scene's tables: the light's sine table at its first edit, and at the context's
// first edit the lights' powers, both uploaded on `stream` behind events of their own
gbl_status ensure_tables(gbl_ctx* ctx, uint32_t light, uint32_t dist_h, const char* who, hipStream_t stream) {
    const size_t n = ctx->h_lights.size();
    if (!ctx->d_light_power) {
        if (!ctx->env_pinned) {
            void* pinned = nullptr;
            if (hipHostMalloc(&pinned, 2 * n * sizeof(float), hipHostMallocDefault) != hipSuccess)
                return fail(ctx, GBL_ERR_OOM, std::string(who) + ": hipHostMalloc(light powers) failed");
            ctx->env_pinned = static_cast<float*>(pinned);
        }
        if (!ctx->env_power_uploaded) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->env_power_uploaded, hipEventDisableTiming));
        void* d = nullptr;
        const gbl_status st = device_alloc(ctx, n * sizeof(float), (std::string(who) + ": light powers").c_str(), &d);
        if (st != GBL_OK) return st;
        std::copy(ctx->h_light_power.begin(), ctx->h_light_power.end(), ctx->env_pinned);   // (no edit before this one: nothing is pending)
        HIP_TRY(ctx, hipMemcpyAsync(d, ctx->env_pinned, n * sizeof(float), hipMemcpyHostToDevice, stream));
        HIP_TRY(ctx, hipEventRecord(ctx->env_power_uploaded, stream));
        ctx->d_light_power = static_cast<float*>(d);
    }
    gbl_ctx::Environment& env = ctx->environment[light];
    if (env.built) return GBL_OK;
    if (!env.uploaded) HIP_TRY(ctx, hipEventCreateWithFlags(&env.uploaded, hipEventDisableTiming));
    if (!env.power_read) HIP_TRY(ctx, hipEventCreateWithFlags(&env.power_read, hipEventDisableTiming));
    void* d = nullptr;
    const gbl_status st = device_alloc(ctx, dist_h * sizeof(float), (std::string(who) + ": sine table").c_str(), &d);
    if (st != GBL_OK) return st;
    env.d_sin_theta = static_cast<float*>(d);
    ibl_sin_theta(dist_h, &env.h_sin_theta);   // the context's, so the source outlives the call
    HIP_TRY(ctx, hipMemcpyAsync(env.d_sin_theta, env.h_sin_theta.data(), dist_h * sizeof(float), hipMemcpyHostToDevice, stream));
    HIP_TRY(ctx, hipEventRecord(env.uploaded, stream));
    env.built = true;
    return GBL_OK;
}

// Another image based light that reads the light's image, or -1
int other_reader(const gbl_ctx* ctx, uint32_t light) {
    for (size_t i = 0; i < ctx->h_lights.size(); ++i)
        if (i != light && ctx->h_lights[i].type == GBL_LIGHT_IBL && ctx->h_lights[i].image == ctx->h_lights[light].image) return static_cast<int>(i);
    return -1;
}

// NULL pointer, range, type: what the edits and the hook refuse alike, after the NULL context
gbl_status check_light(gbl_ctx* ctx, uint32_t light, const char* who) {
    if (light >= ctx->h_lights.size())
        return fail(ctx, GBL_ERR_INVALID, std::string(who) + ": light " + std::to_string(light) + " out of range (the context holds " + std::to_string(ctx->h_lights.size()) + ")");
    const uint32_t type = ctx->h_lights[light].type;
    if (type != GBL_LIGHT_IBL)
        return fail(ctx, GBL_ERR_INVALID, std::string(who) + ": light " + std::to_string(light) + " is a" + (type == GBL_LIGHT_AREA ? "n " : " ") +
                                          (type <= GBL_LIGHT_IBL ? kLightTypes[type] : "unknown") + " light (type " + std::to_string(type) + "), not an image based one");
    return GBL_OK;
}

gbl_status gbl_update_environment_impl(gbl_ctx* ctx, uint32_t light, const float* level0, bool on_device, void* stream_, const char* who) {
    if (!ctx) return GBL_ERR_INVALID;
    const char* const what = on_device ? "d_level0" : "level0";
    // arguments, range, type, the pointer, a second reader: nothing is queued or kept before the last of them
    if (!level0) return fail(ctx, GBL_ERR_INVALID, std::string(who) + ": " + what + " is NULL");
    gbl_status st = GBL_OK;
    if ((st = check_light(ctx, light, who)) != GBL_OK) return st;
    const uint32_t image = static_cast<uint32_t>(ctx->h_lights[light].image);
    const gbl_image& gi = ctx->h_images[image];
    if (on_device) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        if ((st = check_device_pointer(ctx, level0, static_cast<uint64_t>(gi.width) * gi.height * 4 * sizeof(float), who, what)) != GBL_OK) return st;
    }
    if (const int other = other_reader(ctx, light); other >= 0)
        return fail(ctx, GBL_ERR_UNSUPPORTED, std::string(who) + ": image " + std::to_string(image) + " of light " + std::to_string(light) + " is also read by image based light " +
                                              std::to_string(other) + ", whose tables this edit would leave behind; give each light an image of its own");
    const hipStream_t stream = static_cast<hipStream_t>(stream_);
    const DevLight& dl = ctx->h_dev_lights[light];
    const DevScene& sc = ctx->scene;
    const unsigned parts = parts_asked();
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((st = ensure_tables(ctx, light, dl.dist_h, who, stream)) != GBL_OK) return st;
    if ((parts & 1u) && (st = queue_image_pyramid(ctx, image, level0, on_device, stream, who)) != GBL_OK) return st;
    gbl_ctx::Environment& env = ctx->environment[light];
    HIP_TRY(ctx, hipStreamWaitEvent(stream, env.uploaded, 0));
    HIP_TRY(ctx, hipStreamWaitEvent(stream, ctx->env_power_uploaded, 0));
    const float* const texels = sc.texels + gi.texel_offset;
    EnvironmentArgs a;
    a.level = texels + level_offset(gi, distribution_level(gi));   // (above level 0 the pyramid launches have just written it)
    a.top = texels + level_offset(gi, gi.levels - 1);
    a.sin_theta = env.d_sin_theta;
    a.dist = const_cast<float*>(sc.ibl_dist) + dl.dist_offset;
    a.power = ctx->d_light_power;
    a.light_cdf = const_cast<float*>(sc.light_cdf);
    a.light_pick_pdf = const_cast<float*>(sc.light_pick_pdf);
    a.dw = dl.dist_w, a.dh = dl.dist_h;
    a.light = light, a.num_lights = static_cast<uint32_t>(ctx->h_lights.size());
    a.sphere_area = ibl_sphere_area(ctx->bound_lo, ctx->bound_hi);
    gbl_launch_environment(a, parts, stream);
    HIP_TRY(ctx, hipGetLastError());
    if (parts & 4u) {
        // the power goes to the host behind an event; whoever needs h_light_power waits for it (settle_environment_power)
        float* const word = ctx->env_pinned + ctx->h_lights.size() + light;
        HIP_TRY(ctx, hipMemcpyAsync(word, ctx->d_light_power + light, sizeof(float), hipMemcpyDeviceToHost, stream));
        HIP_TRY(ctx, hipEventRecord(env.power_read, stream));
        env.power_pending = true;
    }
    ctx->auto_rays_per_path.clear();   // the pilot's rays per path belong to the old lighting: AUTO measures again
    return GBL_OK;
}

gbl_status gbl_selftest_environment_impl(gbl_ctx* ctx, uint32_t light, float* dist_out, uint64_t* dist_floats, uint32_t dims_out[3]) {
    if (!ctx) return GBL_ERR_INVALID;
    const gbl_status st = check_light(ctx, light, "gbl_selftest_environment");
    if (st != GBL_OK) return st;
    const DevLight& dl = ctx->h_dev_lights[light];
    const uint64_t floats = (2ull * dl.dist_h + 2) + static_cast<uint64_t>(dl.dist_h) * (2ull * dl.dist_w + 2);
    if (dist_floats) *dist_floats = floats;
    if (dims_out) dims_out[0] = distribution_level(ctx->h_images[ctx->h_lights[light].image]), dims_out[1] = dl.dist_w, dims_out[2] = dl.dist_h;
    if (dist_out) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        HIP_TRY(ctx, hipDeviceSynchronize());
        HIP_TRY(ctx, hipMemcpy(dist_out, ctx->scene.ibl_dist + dl.dist_offset, floats * sizeof(float), hipMemcpyDeviceToHost));
    }
    return GBL_OK;
}

}   // namespace

gbl_status settle_environment_power(gbl_ctx* ctx) {
    bool any = false;
    for (size_t i = 0; i < ctx->environment.size(); ++i) {
        gbl_ctx::Environment& env = ctx->environment[i];
        if (!env.power_pending) continue;
        HIP_TRY(ctx, hipEventSynchronize(env.power_read));
        ctx->h_light_power[i] = ctx->env_pinned[ctx->h_lights.size() + i];
        env.power_pending = false;
        any = true;
    }
    if (any) pack_light_distribution(ctx->h_light_power, &ctx->h_light_cdf, &ctx->h_light_pick_pdf);
    return GBL_OK;
}

extern "C" {

gbl_status gbl_update_environment_device(gbl_ctx* ctx, uint32_t light, const float* d_level0, void* stream) {
    return gbl_guard([&] { return gbl_update_environment_impl(ctx, light, d_level0, true, stream, "gbl_update_environment_device"); },
                     [&](const std::string& what) { if (ctx) ctx->error = what; });
}

gbl_status gbl_update_environment(gbl_ctx* ctx, uint32_t light, const float* level0, void* stream) {
    return gbl_guard([&] { return gbl_update_environment_impl(ctx, light, level0, false, stream, "gbl_update_environment"); },
                     [&](const std::string& what) { if (ctx) ctx->error = what; });
}

gbl_status gbl_selftest_environment(gbl_ctx* ctx, uint32_t light, float* dist_out, uint64_t* dist_floats, uint32_t dims_out[3]) {
    return gbl_guard([&] { return gbl_selftest_environment_impl(ctx, light, dist_out, dist_floats, dims_out); }, [&](const std::string& what) { if (ctx) ctx->error = what; });
}

}   // extern "C"
