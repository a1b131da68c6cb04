// libgoblin_hip.so -- C ABI of the device integrator (include/goblin_hip.h): light edits.
// gbl_update_lights validates the given records against the ones the context holds, packs the light records and the power
// distribution again with the functions gbl_create packs them with (scene_prep.h repack_lights), and queues the three tables'
// uploads on the caller's stream from pinned staging the context owns: no kernel is launched and the device is not synchronised.
// A moved area light takes the instances that carry it along through move_instances, gbl_update_instances' own tail, which does
// synchronise.  gbl_get_lights and the self-test hook go with it.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "gbl_host.h"
#include "scene_prep.h"

namespace {

const char* const kWho = "gbl_update_lights";

bool same_bits(const void* a, const void* b, size_t bytes) { return memcmp(a, b, bytes) == 0; }

bool all_finite(const float* f, int n) {
    for (int k = 0; k < n; ++k)
        if (!std::isfinite(f[k])) return false;
    return true;
}

std::string light_name(uint32_t i) { return std::string(kWho) + ": light " + std::to_string(i) + ": "; }

// The fields that fix the Whitted quota, the stream sampler's layout, `extended`, `has_ibl` and light_tris
gbl_status check_fixed_fields(gbl_ctx* ctx, uint32_t i, const gbl_light& have, const gbl_light& want) {
    const auto fixed = [&](const char* field, long long h, long long w) {
        return fail(ctx, GBL_ERR_INVALID, light_name(i) + field + " cannot change (the context holds " + std::to_string(h) + ", the call gives " + std::to_string(w) + ")");
    };
    if (want.type != have.type) return fixed("type", have.type, want.type);
    if (want.mesh != have.mesh) return fixed("mesh", have.mesh, want.mesh);
    if (want.sample_num != have.sample_num) return fixed("sample_num", have.sample_num, want.sample_num);
    if (want.image != have.image) return fixed("image", have.image, want.image);
    if (have.type == GBL_LIGHT_IBL && !same_bits(want.color, have.color, sizeof(have.color)))
        return fail(ctx, GBL_ERR_UNSUPPORTED, light_name(i) + "color: an image based light's colour is baked into its texels when the scene is loaded; re-create the context instead");
    return GBL_OK;
}

// The editable fields of the light's type: finite, and a direction that has a length
gbl_status check_values(gbl_ctx* ctx, uint32_t i, const gbl_light& want) {
    const auto not_finite = [&](const char* field) { return fail(ctx, GBL_ERR_INVALID, light_name(i) + field + " is not finite"); };
    const uint32_t t = want.type;
    if (t != GBL_LIGHT_IBL && !all_finite(want.color, 3)) return not_finite("color");
    if ((t == GBL_LIGHT_POINT || t == GBL_LIGHT_SPOT) && !all_finite(want.position, 3)) return not_finite("position");
    if (t == GBL_LIGHT_SPOT || t == GBL_LIGHT_DIRECTIONAL) {
        if (!all_finite(want.direction, 3)) return not_finite("direction");
        if (want.direction[0] == 0.0f && want.direction[1] == 0.0f && want.direction[2] == 0.0f)
            return fail(ctx, GBL_ERR_INVALID, light_name(i) + "direction has no length");
    }
    if (t == GBL_LIGHT_SPOT) {
        if (!std::isfinite(want.cos_theta_max)) return not_finite("cos_theta_max");
        if (!std::isfinite(want.cos_falloff_start)) return not_finite("cos_falloff_start");
    }
    if (t == GBL_LIGHT_AREA && !(all_finite(want.to_world.position, 3) && all_finite(want.to_world.orientation, 4) && all_finite(want.to_world.scale, 3)))
        return not_finite("to_world");
    if (t == GBL_LIGHT_IBL && !all_finite(want.to_world.orientation, 4)) return not_finite("to_world.orientation");
    return GBL_OK;
}

// Where the three tables, and the powers behind them, sit in one staging slot
struct StageLayout {
    size_t lights, cdf, pick, power, slot;
    explicit StageLayout(size_t n) {
        const auto pad = [](size_t b) { return (b + 255) & ~static_cast<size_t>(255); };
        lights = 0;
        cdf = pad(n * sizeof(DevLight));
        pick = cdf + pad((n + 1) * sizeof(float));
        power = pick + pad(std::max<size_t>(1, n) * sizeof(float));
        slot = power + pad(std::max<size_t>(1, n) * sizeof(float));
    }
};

// The uploads, in the stream's order: a slot of the pinned staging is written again only after the upload that last read it
// The powers go to the device only where an environment edit has made a table of them (gbl_ctx::d_light_power), which the next one reads
gbl_status queue_tables(gbl_ctx* ctx, const std::vector<DevLight>& lights, const std::vector<float>& cdf, const std::vector<float>& pick, const std::vector<float>& power,
                        hipStream_t stream) {
    const StageLayout at(lights.size());
    if (!ctx->light_stage) {
        void* p = nullptr;
        if (hipHostMalloc(&p, at.slot * gbl_ctx::kLightSlots, hipHostMallocDefault) != hipSuccess) return fail(ctx, GBL_ERR_OOM, std::string(kWho) + ": hipHostMalloc(light staging) failed");
        ctx->light_stage = static_cast<unsigned char*>(p);
    }
    const int slot = static_cast<int>(ctx->light_edits % gbl_ctx::kLightSlots);
    if (!ctx->light_ev[slot]) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->light_ev[slot], hipEventDisableTiming));
    else HIP_TRY(ctx, hipEventSynchronize(ctx->light_ev[slot]));
    unsigned char* const s = ctx->light_stage + at.slot * slot;
    memcpy(s + at.lights, lights.data(), lights.size() * sizeof(DevLight));
    memcpy(s + at.cdf, cdf.data(), cdf.size() * sizeof(float));
    memcpy(s + at.pick, pick.data(), pick.size() * sizeof(float));
    memcpy(s + at.power, power.data(), power.size() * sizeof(float));
    const DevScene& sc = ctx->scene;
    HIP_TRY(ctx, hipMemcpyAsync(const_cast<DevLight*>(sc.lights), s + at.lights, lights.size() * sizeof(DevLight), hipMemcpyHostToDevice, stream));
    HIP_TRY(ctx, hipMemcpyAsync(const_cast<float*>(sc.light_cdf), s + at.cdf, cdf.size() * sizeof(float), hipMemcpyHostToDevice, stream));
    HIP_TRY(ctx, hipMemcpyAsync(const_cast<float*>(sc.light_pick_pdf), s + at.pick, pick.size() * sizeof(float), hipMemcpyHostToDevice, stream));
    if (ctx->d_light_power) {
        if (ctx->env_power_uploaded) HIP_TRY(ctx, hipStreamWaitEvent(stream, ctx->env_power_uploaded, 0));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_light_power, s + at.power, power.size() * sizeof(float), hipMemcpyHostToDevice, stream));
    }
    HIP_TRY(ctx, hipEventRecord(ctx->light_ev[slot], stream));
    ++ctx->light_edits;
    return GBL_OK;
}

gbl_status gbl_update_lights_impl(gbl_ctx* ctx, uint32_t first, uint32_t count, const gbl_light* lights, void* stream) {
    if (!ctx) return GBL_ERR_INVALID;
    // arguments, range, the fields that cannot change, values, the area light's rules: nothing is written before the last of them
    if (!lights) return fail(ctx, GBL_ERR_INVALID, std::string(kWho) + ": lights is NULL");
    const size_t n = ctx->h_lights.size();
    if (static_cast<uint64_t>(first) + count > n) return fail(ctx, GBL_ERR_INVALID, std::string(kWho) + ": light range out of bounds");
    if (count == 0) return GBL_OK;
    gbl_status st = GBL_OK;
    for (uint32_t i = 0; i < count; ++i)
        if ((st = check_fixed_fields(ctx, first + i, ctx->h_lights[first + i], lights[i])) != GBL_OK) return st;
    for (uint32_t i = 0; i < count; ++i)
        if ((st = check_values(ctx, first + i, lights[i])) != GBL_OK) return st;
    // an area light whose transform changes takes the instances that carry it along
    std::vector<uint32_t> which;
    std::vector<gbl_trs> to_world;
    for (uint32_t i = 0; i < count; ++i) {
        const gbl_light& have = ctx->h_lights[first + i];
        const std::vector<uint32_t>& carriers = ctx->light_instances[first + i];
        if (have.type != GBL_LIGHT_AREA || carriers.empty() || same_bits(&lights[i].to_world, &have.to_world, sizeof(gbl_trs))) continue;
        if (which.empty()) {
            if ((st = refuse_scene_bound_edit(ctx, kWho)) != GBL_OK) return st;
            if ((st = refresh_instance_mirror(ctx)) != GBL_OK) return st;
        }
        for (uint32_t k : carriers) {
            if (!same_bits(&ctx->h_instances[k].to_world, &have.to_world, sizeof(gbl_trs)))
                return fail(ctx, GBL_ERR_UNSUPPORTED, light_name(first + i) + "to_world: instance " + std::to_string(k) + " emits through this light from a transform of its own, "
                                                      "and the two can only move together while they are the same; re-create the context instead");
            which.push_back(k);
            to_world.push_back(lights[i].to_world);
        }
    }
    // an environment edit left its light's power on the device: h_light_power waits for it here (gbl_host.h)
    if ((st = settle_environment_power(ctx)) != GBL_OK) return st;
    std::vector<DevLight> records = ctx->h_dev_lights;
    std::vector<float> power = ctx->h_light_power, cdf, pick;
    repack_lights(lights, first, count, ctx->bound_lo, ctx->bound_hi, &records, &power, &cdf, &pick);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // (build_tlas's refusal of a transform the reference cannot invert comes from here, before anything is written)
    if (!which.empty() && (st = move_instances(ctx, which.data(), static_cast<uint32_t>(which.size()), to_world.data(), kWho)) != GBL_OK) return st;
    if ((st = queue_tables(ctx, records, cdf, pick, power, static_cast<hipStream_t>(stream))) != GBL_OK) return st;
    std::copy(lights, lights + count, ctx->h_lights.begin() + first);
    ctx->h_dev_lights.swap(records);
    ctx->h_light_power.swap(power);
    ctx->h_light_cdf.swap(cdf);
    ctx->h_light_pick_pdf.swap(pick);
    ctx->auto_rays_per_path.clear();   // the pilot's rays per path belong to the old lighting: AUTO measures again
    return GBL_OK;
}

gbl_status gbl_get_lights_impl(const gbl_ctx* ctx, uint32_t first, uint32_t count, gbl_light* out) {
    if (!ctx || !out || static_cast<uint64_t>(first) + count > ctx->h_lights.size()) return GBL_ERR_INVALID;
    std::copy(ctx->h_lights.begin() + first, ctx->h_lights.begin() + first + count, out);
    return GBL_OK;
}

gbl_status gbl_selftest_lights_impl(gbl_ctx* ctx, void* records_out, float* cdf_out, float* pick_pdf_out, uint64_t* total) {
    if (!ctx) return GBL_ERR_INVALID;
    const size_t n = ctx->h_lights.size();
    if (total) *total = n;
    if (!records_out && !cdf_out && !pick_pdf_out) return GBL_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipDeviceSynchronize());
    if (records_out && n > 0) HIP_TRY(ctx, hipMemcpy(records_out, ctx->scene.lights, n * sizeof(DevLight), hipMemcpyDeviceToHost));
    if (cdf_out) HIP_TRY(ctx, hipMemcpy(cdf_out, ctx->scene.light_cdf, (n + 1) * sizeof(float), hipMemcpyDeviceToHost));
    if (pick_pdf_out) HIP_TRY(ctx, hipMemcpy(pick_pdf_out, ctx->scene.light_pick_pdf, std::max<size_t>(1, n) * sizeof(float), hipMemcpyDeviceToHost));
    return GBL_OK;
}

}   // namespace

extern "C" {

gbl_status gbl_update_lights(gbl_ctx* ctx, uint32_t first, uint32_t count, const gbl_light* lights, void* stream) {
    return gbl_guard([&] { return gbl_update_lights_impl(ctx, first, count, lights, stream); }, [&](const std::string& what) { if (ctx) ctx->error = what; });
}

gbl_status gbl_get_lights(const gbl_ctx* ctx, uint32_t first, uint32_t count, gbl_light* out) {
    return gbl_guard([&] { return gbl_get_lights_impl(ctx, first, count, out); }, [&](const std::string&) {});
}

gbl_status gbl_selftest_lights(gbl_ctx* ctx, void* records_out, float* cdf_out, float* pick_pdf_out, uint64_t* total) {
    return gbl_guard([&] { return gbl_selftest_lights_impl(ctx, records_out, cdf_out, pick_pdf_out, total); }, [&](const std::string& what) { if (ctx) ctx->error = what; });
}

}   // extern "C"
