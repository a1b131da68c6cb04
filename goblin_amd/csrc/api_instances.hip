// libgoblin_hip.so -- C ABI of the device integrator (include/goblin_hip.h): instance edits, and the TLAS every scene edit ends
// in.  gbl_update_instances packs the edited list on the host (scene_prep.cpp build_tlas); its tail, move_instances, is the light
// edits' and, moving nothing, the geometry edits' (gbl_host.h).  gbl_update_instances_device composes the edited instances'
// records on the device (kernels/instances.h) and builds the TLAS on the host over the boxes read back, or --
// GBL_INSTANCES_DEVICE_TLAS -- on the device with the linear builder (kernels/lbvh.h).  gbl_get_instances_device, the self-test
// hook, and the two helpers that keep h_instances[i].to_world and the device's raw table in step go with it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gbl_host.h"
#include "kernels/instances_args.h"
#include "scene_prep.h"

gbl_status refresh_instance_mirror(gbl_ctx* ctx) {
    if (ctx->trs_stale_end <= ctx->trs_stale_first || !ctx->d_trs) return GBL_OK;
    const uint32_t first = ctx->trs_stale_first, count = std::min<uint32_t>(ctx->trs_stale_end, static_cast<uint32_t>(ctx->h_instances.size())) - first;
    std::vector<gbl_trs> fresh(count);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpy(fresh.data(), ctx->d_trs + first, count * sizeof(gbl_trs), hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < count; ++i) ctx->h_instances[first + i].to_world = fresh[i];
    ctx->trs_stale_first = ctx->trs_stale_end = 0;
    return GBL_OK;
}

gbl_status write_instance_table(gbl_ctx* ctx, uint32_t first, uint32_t count) {
    if (!ctx->d_trs || count == 0) return GBL_OK;
    std::vector<gbl_trs> out(count);
    for (uint32_t i = 0; i < count; ++i) out[i] = ctx->h_instances[first + i].to_world;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpy(ctx->d_trs + first, out.data(), count * sizeof(gbl_trs), hipMemcpyHostToDevice));
    return GBL_OK;
}

void commit_tlas(gbl_ctx* ctx, int32_t root, int depth, size_t nodes, int stack_entries) {
    ctx->scene.tlas_root = root;
    ctx->scene.stack_entries = stack_entries;   // (the wavefront stack backing is re-checked at render time)
    ctx->info.tlas_depth = depth;
    ctx->info.tlas_nodes = nodes;
    ctx->auto_rays_per_path.clear();   // the edited scene's paths may be longer or shorter: AUTO measures again
}

gbl_status refuse_scene_bound_edit(gbl_ctx* ctx, const char* who) {
    if (!ctx->has_directional) return GBL_OK;
    return fail(ctx, GBL_ERR_UNSUPPORTED, std::string(who) + ": a directional or image based light's power (and the image based light's sampling sphere) "
                                          "depends on the scene bound (GoblinLight.cpp:203-210, 590-629); re-create the context instead");
}

gbl_status move_instances(gbl_ctx* ctx, const uint32_t* which, uint32_t count, const gbl_trs* to_world, const char* who) {
    gbl_status st = refresh_instance_mirror(ctx);   // (a device instance edit may have left the transforms' host copy behind)
    if (st != GBL_OK) return st;
    std::vector<gbl_instance> edited = ctx->h_instances;
    for (uint32_t i = 0; i < count; ++i) edited[which[i]].to_world = to_world[i];
    const TlasInput in = {edited.data(),       static_cast<uint32_t>(edited.size()), ctx->h_meshes.data(),  ctx->h_materials.data(),
                          ctx->mesh_lo.data(), ctx->mesh_hi.data(),                  ctx->mesh_root.data(), ctx->tlas_base};
    TlasResult built;
    std::string err;
    if ((st = build_tlas(in, &built, &err)) != GBL_OK) return fail(ctx, st, err);
    const std::vector<DevInstance>& inst = built.instances;
    const std::vector<DevNode>& tlas = built.nodes;
    const std::vector<DevInstanceBound>& bounds = built.instance_bounds;
    if (tlas.size() > ctx->tlas_capacity) return fail(ctx, GBL_ERR_DEVICE, std::string(who) + ": rebuilt TLAS does not fit its reserved nodes");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipDeviceSynchronize());   // no render may be reading the old TLAS
    DevScene& sc = ctx->scene;
    if (!inst.empty())
        HIP_TRY(ctx, hipMemcpy(const_cast<DevInstance*>(sc.instances), inst.data(), inst.size() * sizeof(DevInstance), hipMemcpyHostToDevice));
    if (!bounds.empty())
        HIP_TRY(ctx, hipMemcpy(const_cast<DevInstanceBound*>(sc.instance_bounds), bounds.data(), bounds.size() * sizeof(DevInstanceBound), hipMemcpyHostToDevice));
    if (!tlas.empty())
        HIP_TRY(ctx, hipMemcpy(const_cast<DevNode*>(sc.nodes) + ctx->tlas_base, tlas.data(), tlas.size() * sizeof(DevNode), hipMemcpyHostToDevice));
    commit_tlas(ctx, built.root, built.depth, tlas.size(), scene_stack_entries(tlas, ctx->tlas_base, built.root, inst, ctx->mesh_stack_need));
    ctx->h_instances.swap(edited);
    for (uint32_t i = 0; i < count;) {   // the raw table, run by run
        uint32_t end = i + 1;
        while (end < count && which[end] == which[end - 1] + 1) ++end;
        if ((st = write_instance_table(ctx, which[i], end - i)) != GBL_OK) return st;
        i = end;
    }
    return GBL_OK;
}

gbl_status retlas_after_geometry_edit(gbl_ctx* ctx, const char* who) {
    if (const gbl_status st = move_instances(ctx, nullptr, 0, nullptr, who); st != GBL_OK) return st;   // (moves none: the mesh bounds and roots are what changed)
    HIP_TRY(ctx, hipDeviceSynchronize());
    return GBL_OK;
}

namespace {

// What both instance edits refuse before they look at a transform, in gbl_update_instances' order and words
gbl_status check_instance_edit(gbl_ctx* ctx, uint32_t first, uint32_t count, const gbl_trs* to_world) {
    if (!to_world || static_cast<uint64_t>(first) + count > ctx->h_instances.size()) return fail(ctx, GBL_ERR_INVALID, "gbl_update_instances: instance range out of bounds");
    if (const gbl_status st = refuse_scene_bound_edit(ctx, "gbl_update_instances"); st != GBL_OK) return st;
    for (uint32_t i = 0; i < count; ++i)
        if (ctx->h_instances[first + i].area_light >= 0)
            return fail(ctx, GBL_ERR_UNSUPPORTED, "gbl_update_instances: instance " + std::to_string(first + i) + " carries an area light, whose own transform would "
                                                  "have to move with it; re-create the context instead");
    return GBL_OK;
}

gbl_status gbl_update_instances_impl(gbl_ctx* ctx, uint32_t first, uint32_t count, const gbl_trs* to_world) {
    if (!ctx) return GBL_ERR_INVALID;
    if (const gbl_status st = check_instance_edit(ctx, first, count, to_world); st != GBL_OK) return st;
    std::vector<uint32_t> which(count);
    for (uint32_t i = 0; i < count; ++i) which[i] = first + i;
    return move_instances(ctx, which.data(), count, to_world, "gbl_update_instances");
}

// The raw table, made from the host copy at its first use (no device edit can have come before it: the copy is current)
gbl_status ensure_instance_table(gbl_ctx* ctx) {
    if (ctx->d_trs) return GBL_OK;
    const size_t n = ctx->h_instances.size();
    void* p = nullptr;
    const gbl_status st = device_alloc(ctx, std::max<size_t>(1, n) * sizeof(gbl_trs), "instance transforms", &p);
    if (st != GBL_OK) return st;
    std::vector<gbl_trs> all(n);
    for (size_t i = 0; i < n; ++i) all[i] = ctx->h_instances[i].to_world;
    if (n > 0) HIP_TRY(ctx, hipMemcpy(p, all.data(), n * sizeof(gbl_trs), hipMemcpyHostToDevice));
    ctx->d_trs = static_cast<gbl_trs*>(p);   // (an upload that failed leaves the allocation to gbl_destroy and the table unmade)
    return GBL_OK;
}

// The per-mesh object bounds on the device, as the host holds them NOW: vertex edits and mesh rebuilds write mesh_lo / mesh_hi,
// and the values last sent tell whether the table is behind
gbl_status ensure_mesh_bounds(gbl_ctx* ctx) {
    const size_t meshes = ctx->h_meshes.size();
    std::vector<float> now(6 * meshes);
    for (size_t m = 0; m < meshes; ++m)
        for (int a = 0; a < 3; ++a) now[6 * m + a] = ctx->mesh_lo[3 * m + a], now[6 * m + 3 + a] = ctx->mesh_hi[3 * m + a];
    if (!ctx->d_mesh_bounds) {
        void* p = nullptr;
        const gbl_status st = device_alloc(ctx, std::max<size_t>(1, now.size()) * sizeof(float), "mesh bounds", &p);
        if (st != GBL_OK) return st;
        ctx->d_mesh_bounds = static_cast<float*>(p);
        ctx->mesh_bounds_sent.clear();
    }
    if (now.size() == ctx->mesh_bounds_sent.size() && (now.empty() || memcmp(now.data(), ctx->mesh_bounds_sent.data(), now.size() * sizeof(float)) == 0)) return GBL_OK;
    ctx->mesh_bounds_sent.clear();   // (behind until the upload is done)
    if (!now.empty()) HIP_TRY(ctx, hipMemcpy(ctx->d_mesh_bounds, now.data(), now.size() * sizeof(float), hipMemcpyHostToDevice));
    ctx->mesh_bounds_sent.swap(now);
    return GBL_OK;
}

// What scene_stack_entries reads of an instance record: its shape and its mesh
const std::vector<DevInstance>& need_instances(gbl_ctx* ctx) {
    if (ctx->need_instances.size() != ctx->h_instances.size()) {
        ctx->need_instances.assign(ctx->h_instances.size(), DevInstance());
        for (size_t i = 0; i < ctx->h_instances.size(); ++i) {
            DevInstance& di = ctx->need_instances[i];
            memset(&di, 0, sizeof(di));
            di.mesh = static_cast<int32_t>(ctx->h_instances[i].mesh);
            di.shape = ctx->h_meshes[ctx->h_instances[i].mesh].shape;
        }
    }
    return ctx->need_instances;
}

// The refusal the compose kernel folded into its word, in words: the non-finite transform is this entry's own, the determinant
// is build_tlas's refusal with build_tlas's message (made by pack_transform over the one record, read back for it)
gbl_status refuse_word(gbl_ctx* ctx, unsigned long long word, uint32_t first, uint32_t count, const gbl_trs* d_to_world) {
    const uint32_t kind = static_cast<uint32_t>(word >> 32), index = static_cast<uint32_t>(word);
    if (index < first || index - first >= count) return fail(ctx, GBL_ERR_INTERNAL, "gbl_update_instances_device: the refusal word is out of range");
    if (kind == GBL_INST_NOT_FINITE)
        return fail(ctx, GBL_ERR_INVALID, "gbl_update_instances_device: the transform of instance " + std::to_string(index) + " is not finite");
    if (kind == GBL_INST_BOX_NOT_FINITE)
        return fail(ctx, GBL_ERR_INVALID, "gbl_update_instances_device: the world bound of instance " + std::to_string(index) + " is not finite: a device TLAS cannot hold it");
    if (kind == GBL_INST_SINGULAR) {
        gbl_trs t;
        HIP_TRY(ctx, hipMemcpy(&t, d_to_world + (index - first), sizeof(t), hipMemcpyDeviceToHost));
        float m[12], inv[12];
        std::string err;
        if (pack_transform(t, index, m, inv, &err)) return fail(ctx, GBL_ERR_INTERNAL, "gbl_update_instances_device: the device refused a transform the host inverts");
        return fail(ctx, GBL_ERR_INVALID, err);
    }
    return fail(ctx, GBL_ERR_INTERNAL, "gbl_update_instances_device: instance " + std::to_string(index) + " refers to a mesh out of range");
}

gbl_status gbl_update_instances_device_impl(gbl_ctx* ctx, uint32_t first, uint32_t count, const gbl_trs* d_to_world, uint32_t flags) {
    if (!ctx) return GBL_ERR_INVALID;
    // every refusal the host can make, before any launch: this entry's own, then gbl_update_instances' in its order and words
    if (!d_to_world) return fail(ctx, GBL_ERR_INVALID, "gbl_update_instances_device: d_to_world is NULL");
    if (flags & ~GBL_INSTANCES_DEVICE_TLAS) return fail(ctx, GBL_ERR_INVALID, "gbl_update_instances_device: unknown bits in flags");
    const size_t n = ctx->h_instances.size();
    gbl_status st = check_instance_edit(ctx, first, count, d_to_world);
    if (st != GBL_OK) return st;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    st = check_device_pointer(ctx, d_to_world, static_cast<uint64_t>(count) * sizeof(gbl_trs), "gbl_update_instances_device", "d_to_world");
    if (st != GBL_OK) return st;
    if (count == 0) return GBL_OK;
    const bool device_tlas = (flags & GBL_INSTANCES_DEVICE_TLAS) != 0 && n >= 2;   // (fewer than two instances: there is no tree to build)
    LapClock clock;
    HIP_TRY(ctx, hipDeviceSynchronize());   // no render may be reading the tables, and whatever wrote the caller's floats is done
    if ((st = ensure_instance_table(ctx)) != GBL_OK) return st;
    if ((st = ensure_mesh_bounds(ctx)) != GBL_OK) return st;
    // staging: the refusal word, the edited instances' records and bounds, and for a device TLAS the bounds of all instances
    const auto pad = [](uint64_t b) { return (b + 255) & ~static_cast<uint64_t>(255); };
    const uint64_t o_inst = 256, o_bound = o_inst + pad(static_cast<uint64_t>(count) * sizeof(DevInstance));
    const uint64_t o_merged = o_bound + pad(static_cast<uint64_t>(count) * sizeof(DevInstanceBound));
    const uint64_t stage_bytes = o_merged + (device_tlas ? pad(static_cast<uint64_t>(n) * sizeof(DevInstanceBound)) : 0);
    if ((st = grow(ctx, ctx->inst_stage, stage_bytes, "instance edit staging")) != GBL_OK) return st;
    unsigned char* const stage = static_cast<unsigned char*>(ctx->inst_stage.p);
    unsigned long long* d_word = reinterpret_cast<unsigned long long*>(stage);
    DevInstance* s_inst = reinterpret_cast<DevInstance*>(stage + o_inst);
    DevInstanceBound* s_bound = reinterpret_cast<DevInstanceBound*>(stage + o_bound);
    DevInstanceBound* s_merged = reinterpret_cast<DevInstanceBound*>(stage + o_merged);
    DevScene& sc = ctx->scene;
    HIP_TRY(ctx, hipMemsetAsync(d_word, 0xFF, sizeof(unsigned long long), 0));
    gbl_launch_inst_compose(d_to_world, first, count, sc.instances, ctx->d_mesh_bounds, static_cast<uint32_t>(ctx->h_meshes.size()), device_tlas, s_inst, s_bound, d_word, 0);
    HIP_TRY(ctx, hipGetLastError());
    unsigned long long word = 0;
    HIP_TRY(ctx, hipMemcpy(&word, d_word, sizeof(word), hipMemcpyDeviceToHost));
    if (word != ~0ull) return refuse_word(ctx, word, first, count, d_to_world);
    const double compose_ms = clock.lap_ms();

    // the TLAS over the boxes of all instances, the edited ones' from staging: nothing of the context is written before it stands
    std::vector<DevNode> tlas;
    const DevNode* d_tlas = nullptr;
    int32_t root = 0;
    int depth = 0;
    if (device_tlas) {
        HIP_TRY(ctx, hipMemcpyAsync(s_merged, sc.instance_bounds, n * sizeof(DevInstanceBound), hipMemcpyDeviceToDevice, 0));
        HIP_TRY(ctx, hipMemcpyAsync(s_merged + first, s_bound, static_cast<size_t>(count) * sizeof(DevInstanceBound), hipMemcpyDeviceToDevice, 0));
        uint32_t used = 0;
        if ((st = gbl_build_tlas_device(ctx, s_merged, static_cast<uint32_t>(n), ctx->tlas_base, ctx->tlas_capacity, &d_tlas, &used, &depth)) != GBL_OK) return st;
        // stack_entries by the exact rule, over the records the kernels will read (64 bytes per node cross the bus)
        tlas.resize(used);
        HIP_TRY(ctx, hipMemcpy(tlas.data(), d_tlas, static_cast<size_t>(used) * sizeof(DevNode), hipMemcpyDeviceToHost));
        root = ctx->tlas_base;
    } else {
        std::vector<DevInstanceBound> bounds(n);
        HIP_TRY(ctx, hipMemcpy(bounds.data(), sc.instance_bounds, n * sizeof(DevInstanceBound), hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(bounds.data() + first, s_bound, static_cast<size_t>(count) * sizeof(DevInstanceBound), hipMemcpyDeviceToHost));
        build_tlas_nodes(bounds.data(), static_cast<uint32_t>(n), ctx->tlas_base, &tlas, &root, &depth);
    }
    if (tlas.size() > ctx->tlas_capacity) return fail(ctx, GBL_ERR_DEVICE, "gbl_update_instances_device: rebuilt TLAS does not fit its reserved nodes");
    const int stack_entries = scene_stack_entries(tlas, ctx->tlas_base, root, need_instances(ctx), ctx->mesh_stack_need);
    const double tlas_ms = clock.lap_ms();

    // commit: the device is idle, the copies are ordered by the null stream
    HIP_TRY(ctx, hipMemcpyAsync(const_cast<DevInstance*>(sc.instances) + first, s_inst, static_cast<size_t>(count) * sizeof(DevInstance), hipMemcpyDeviceToDevice, 0));
    HIP_TRY(ctx, hipMemcpyAsync(const_cast<DevInstanceBound*>(sc.instance_bounds) + first, s_bound, static_cast<size_t>(count) * sizeof(DevInstanceBound),
                                hipMemcpyDeviceToDevice, 0));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_trs + first, d_to_world, static_cast<size_t>(count) * sizeof(gbl_trs), hipMemcpyDeviceToDevice, 0));
    if (!tlas.empty()) {
        DevNode* const dst = const_cast<DevNode*>(sc.nodes) + ctx->tlas_base;
        if (device_tlas) HIP_TRY(ctx, hipMemcpyAsync(dst, d_tlas, tlas.size() * sizeof(DevNode), hipMemcpyDeviceToDevice, 0));
        else HIP_TRY(ctx, hipMemcpy(dst, tlas.data(), tlas.size() * sizeof(DevNode), hipMemcpyHostToDevice));
    }
    HIP_TRY(ctx, hipDeviceSynchronize());
    commit_tlas(ctx, root, depth, tlas.size(), stack_entries);
    const bool none_stale = ctx->trs_stale_end <= ctx->trs_stale_first;   // the host copy's stale range takes the edit in
    ctx->trs_stale_first = none_stale ? first : std::min(ctx->trs_stale_first, first);
    ctx->trs_stale_end = none_stale ? first + count : std::max(ctx->trs_stale_end, first + count);
    if (probing())
        fprintf(stderr, "probe: gbl_update_instances_device %u of %zu instances (flags %u): synchronise, tables, compose and its word %.3f ms, TLAS on the %s (%zu nodes, "
                        "%d levels, stack entries %d) %.3f ms, commit %.3f ms\n", count, n, flags, compose_ms, device_tlas ? "device" : "host", tlas.size(), depth,
                stack_entries, tlas_ms, clock.lap_ms());
    return GBL_OK;
}

gbl_status gbl_get_instances_device_impl(gbl_ctx* ctx, uint32_t first, uint32_t count, gbl_trs* d_out) {
    if (!ctx) return GBL_ERR_INVALID;
    if (!d_out) return fail(ctx, GBL_ERR_INVALID, "gbl_get_instances_device: d_out is NULL");
    if (static_cast<uint64_t>(first) + count > ctx->h_instances.size()) return fail(ctx, GBL_ERR_INVALID, "gbl_get_instances_device: instance range out of bounds");
    const uint64_t bytes = static_cast<uint64_t>(count) * sizeof(gbl_trs);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    gbl_status st = check_device_pointer(ctx, d_out, bytes, "gbl_get_instances_device", "d_out");
    if (st != GBL_OK) return st;
    if ((st = ensure_instance_table(ctx)) != GBL_OK) return st;
    // the table changes only inside calls that synchronise, so the null stream's order is all the copy needs
    if (count > 0) {
        HIP_TRY(ctx, hipMemcpyAsync(d_out, ctx->d_trs + first, bytes, hipMemcpyDeviceToDevice, 0));
        HIP_TRY(ctx, hipStreamSynchronize(0));
    }
    return GBL_OK;
}

gbl_status gbl_selftest_instances_impl(gbl_ctx* ctx, uint64_t first, uint64_t count, void* records_out, void* bounds_out, uint64_t* total, int32_t* tlas_root,
                                       int32_t* stack_entries) {
    if (!ctx) return GBL_ERR_INVALID;
    const uint64_t n = ctx->h_instances.size();
    if (total) *total = n;
    if (tlas_root) *tlas_root = ctx->scene.tlas_root;
    if (stack_entries) *stack_entries = ctx->scene.stack_entries;
    if (first > n || count > n - first) return fail(ctx, GBL_ERR_INVALID, "gbl_selftest_instances: record range out of bounds");
    if (count == 0 || (!records_out && !bounds_out)) return GBL_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipDeviceSynchronize());
    if (records_out) HIP_TRY(ctx, hipMemcpy(records_out, ctx->scene.instances + first, count * sizeof(DevInstance), hipMemcpyDeviceToHost));
    if (bounds_out) HIP_TRY(ctx, hipMemcpy(bounds_out, ctx->scene.instance_bounds + first, count * sizeof(DevInstanceBound), hipMemcpyDeviceToHost));
    return GBL_OK;
}

}   // namespace

extern "C" {

gbl_status gbl_update_instances(gbl_ctx* ctx, uint32_t first, uint32_t count, const gbl_trs* to_world) {
    return gbl_guard([&] { return gbl_update_instances_impl(ctx, first, count, to_world); }, [&](const std::string& what) { if (ctx) ctx->error = what; });
}

gbl_status gbl_update_instances_device(gbl_ctx* ctx, uint32_t first, uint32_t count, const gbl_trs* d_to_world, uint32_t flags) {
    return gbl_guard([&] { return gbl_update_instances_device_impl(ctx, first, count, d_to_world, flags); }, [&](const std::string& what) { if (ctx) ctx->error = what; });
}

gbl_status gbl_get_instances_device(gbl_ctx* ctx, uint32_t first, uint32_t count, gbl_trs* d_out) {
    return gbl_guard([&] { return gbl_get_instances_device_impl(ctx, first, count, d_out); }, [&](const std::string& what) { if (ctx) ctx->error = what; });
}

gbl_status gbl_selftest_instances(gbl_ctx* ctx, uint64_t first, uint64_t count, void* records_out, void* bounds_out, uint64_t* total, int32_t* tlas_root,
                                  int32_t* stack_entries) {
    return gbl_guard([&] { return gbl_selftest_instances_impl(ctx, first, count, records_out, bounds_out, total, tlas_root, stack_entries); },
                     [&](const std::string& what) { if (ctx) ctx->error = what; });
}

}   // extern "C"
