// libgoblin_hip.so -- C ABI of the device integrator (include/goblin_hip.h): gbl_get_instances, gbl_render_motion,
// gbl_render_motion_deform and gbl_render_motion_deform_device, the per-pixel "where was this surface point in the previous frame" (kernels/motion.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "gbl_host.h"
#include "motion_stage.h"
#include "scene_prep.h"

namespace {

gbl_status gbl_get_instances_impl(const gbl_ctx* cctx, uint32_t first, uint32_t count, gbl_trs* out) {
    if (!cctx || !out || static_cast<uint64_t>(first) + count > cctx->h_instances.size()) return GBL_ERR_INVALID;
    gbl_ctx* ctx = const_cast<gbl_ctx*>(cctx);   // (the transforms' host copy is a cache of the device's after a device edit: refreshing it changes nothing a caller can see)
    const gbl_status st = refresh_instance_mirror(ctx);
    if (st != GBL_OK) return st;
    for (uint32_t i = 0; i < count; ++i) out[i] = ctx->h_instances[first + i].to_world;
    return GBL_OK;
}

// One device-to-device copy of a deformed mesh's previous pose into the context's table
struct PoseCopy {
    const float* src;
    uint64_t first_vertex, vertex_count;   // where it lands among the packed positions
};

// stage_motion_meshes for previous poses in device memory (gbl_render_motion_deform_device): the same refusals in the same
// order, the pointer checks beside "positions is NULL"; finiteness by vertices_check_kernel, one word per listed mesh; deformed
// or not by pose_differs_kernel against the context's device positions, one word per listed mesh.  Both read-backs wait for
// `stream`.  *table is stage_motion_meshes' table, `copies` the packed block's contents in its order, *total its vertices.
gbl_status stage_device_poses(gbl_ctx* ctx, const gbl_motion_mesh* prev, uint32_t num_prev, const char* who, hipStream_t stream, std::vector<int32_t>* table,
                              std::vector<PoseCopy>* copies, uint64_t* total) {
    const size_t num_meshes = ctx->h_meshes.size();
    table->assign(num_meshes, GBL_MOTION_NOT_DEFORMED);
    copies->clear();
    *total = 0;
    if (num_prev == 0) return GBL_OK;
    if (!prev) return fail(ctx, GBL_ERR_INVALID, std::string(who) + ": prev_meshes is NULL with num_prev_meshes > 0");
    // the entries' checks that need no coordinate, up to the first that fails: the entries before it may still hold a
    // non-finite float, which stage_motion_meshes would have met first
    std::vector<bool> listed(num_meshes, false);
    uint32_t checked = 0;
    gbl_status pending = GBL_OK;
    std::string pending_err;
    for (; checked < num_prev; ++checked) {
        const gbl_motion_mesh& pm = prev[checked];
        if (!check_motion_mesh(ctx->h_meshes.data(), num_meshes, pm, checked, &listed, who, &pending_err)) {
            pending = GBL_ERR_INVALID;
            break;
        }
        const gbl_mesh& gm = ctx->h_meshes[pm.mesh];
        if (3 * static_cast<uint64_t>(gm.vertex_count) >= 0xFFFFFFFFull) {
            pending = GBL_ERR_UNSUPPORTED;
            pending_err = std::string(who) + ": a mesh of 2^32 / 3 vertices or more (the check word holds a float's index)";
            break;
        }
        pending = check_device_pointer(ctx, pm.positions, 3 * static_cast<uint64_t>(gm.vertex_count) * sizeof(float), who,
                                       ("prev_meshes[" + std::to_string(checked) + "].positions").c_str());
        if (pending != GBL_OK) {
            pending_err = ctx->error;
            break;
        }
    }
    // per listed mesh: a check word, a differs flag, a PoseList record
    const uint64_t words_bytes = (static_cast<uint64_t>(num_prev) * sizeof(uint32_t) + 15) / 16 * 16;
    gbl_status st = grow(ctx, ctx->pose_words, 2 * words_bytes + static_cast<uint64_t>(num_prev) * sizeof(PoseList), "previous pose words");
    if (st != GBL_OK) return st;
    unsigned char* base = static_cast<unsigned char*>(ctx->pose_words.p);
    uint32_t* d_check = reinterpret_cast<uint32_t*>(base);
    uint32_t* d_differs = reinterpret_cast<uint32_t*>(base + words_bytes);
    PoseList* d_list = reinterpret_cast<PoseList*>(base + 2 * words_bytes);
    std::vector<uint32_t> words(num_prev);
    if (checked > 0) {
        HIP_TRY(ctx, hipMemsetAsync(d_check, 0xFF, words_bytes, stream));
        for (uint32_t k = 0; k < checked; ++k)
            gbl_launch_vertices_check(prev[k].positions, nullptr, 3 * ctx->h_meshes[prev[k].mesh].vertex_count, d_check + k, stream);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(words.data(), d_check, checked * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        HIP_TRY(ctx, hipStreamSynchronize(stream));
        for (uint32_t k = 0; k < checked; ++k)
            if (words[k] != 0xFFFFFFFFu) return fail(ctx, GBL_ERR_INVALID, motion_mesh_not_finite(who, k, words[k]));
    }
    if (pending != GBL_OK) return fail(ctx, pending, pending_err);
    // deformed or unchanged, bitwise against the positions the device holds
    std::vector<PoseList> list(num_prev);
    uint32_t max_floats = 0;
    for (uint32_t k = 0; k < num_prev; ++k) {
        const gbl_mesh& gm = ctx->h_meshes[prev[k].mesh];
        list[k].prev = prev[k].positions;
        list[k].first_float = 3 * gm.vertex_offset;
        list[k].num_floats = 3 * gm.vertex_count;
        max_floats = std::max(max_floats, list[k].num_floats);
    }
    if (ctx->h_positions.size() >= 0xFFFFFFFFull) return fail(ctx, GBL_ERR_UNSUPPORTED, std::string(who) + ": a scene of 2^32 / 3 vertices or more");
    HIP_TRY(ctx, hipMemcpyAsync(d_list, list.data(), num_prev * sizeof(PoseList), hipMemcpyHostToDevice, stream));   // (pageable: read before the call returns)
    HIP_TRY(ctx, hipMemsetAsync(d_differs, 0, words_bytes, stream));
    gbl_launch_pose_differs(d_list, num_prev, max_floats, ctx->scene.positions, static_cast<uint32_t>(ctx->h_positions.size()), d_differs, stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(words.data(), d_differs, num_prev * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    for (uint32_t k = 0; k < num_prev; ++k) {
        const gbl_mesh& gm = ctx->h_meshes[prev[k].mesh];
        if (gm.vertex_count == 0 || words[k] == 0u) continue;   // unchanged
        const uint64_t at = *total;
        std::string err;
        if (!place_motion_mesh(gm, prev[k].mesh, total, table, who, &err)) return fail(ctx, GBL_ERR_INVALID, err);
        copies->push_back(PoseCopy{prev[k].positions, at, gm.vertex_count});
    }
    return GBL_OK;
}

// gbl_render_motion (prev_meshes NULL, num_prev_meshes 0), gbl_render_motion_deform and, with device_poses, its _device form;
// `who` starts the error messages
gbl_status gbl_render_motion_impl(gbl_ctx* ctx, const gbl_motion_params* p, const gbl_motion_mesh* prev_meshes, uint32_t num_prev_meshes, float* motion_out,
                                  const char* who_name, bool device_poses = false) {
    if (!ctx) return GBL_ERR_INVALID;
    const std::string who = who_name;
    if (!p) return fail(ctx, GBL_ERR_INVALID, who + ": params is NULL");
    if (!motion_out) return fail(ctx, GBL_ERR_INVALID, who + ": motion_out is NULL");
    if (p->prev_camera.type > GBL_CAMERA_ORTHOGRAPHIC) return fail(ctx, GBL_ERR_INVALID, who + ": prev_camera.type: unknown camera type");
    const size_t count = ctx->h_instances.size();
    if (count >= (1u << 24) - 1u)
        return fail(ctx, GBL_ERR_UNSUPPORTED, who + ": 2^24 - 1 or more instances, an instance id would not be exact in the plane's float");
    const int width = ctx->info.xres, height = ctx->info.yres, n = width * height;
    const uint64_t film_bytes = static_cast<uint64_t>(n) * 4 * sizeof(float);
    if (overlaps(motion_out, 2 * film_bytes, p->normal_accum, film_bytes)) return fail(ctx, GBL_ERR_INVALID, who + ": motion_out may not overlap normal_accum");
    const DevScene& sc = ctx->scene;
    if (stack_lds_bytes(sc) > 160 * 1024) return fail(ctx, GBL_ERR_UNSUPPORTED, "scene's BVH is too deep for the LDS traversal stacks");

    // The previous transforms of the instances that moved, composed as build_tlas composes the current ones.  Everything is
    // checked and staged on the host before the context is touched.
    const uint64_t xf_bytes = static_cast<uint64_t>(count) * GBL_MOTION_XF_FLOATS * sizeof(float), flag_bytes = static_cast<uint64_t>(count) * sizeof(uint32_t);
    bool any_moved = false;
    std::vector<unsigned char> staged;
    if (p->prev_to_world && count > 0) {
        const gbl_status fresh = refresh_instance_mirror(ctx);   // (the current transforms are compared and composed on the host)
        if (fresh != GBL_OK) return fresh;
        staged.assign(xf_bytes + flag_bytes, 0);
        float* xf = reinterpret_cast<float*>(staged.data());
        uint32_t* moved = reinterpret_cast<uint32_t*>(staged.data() + xf_bytes);
        for (size_t i = 0; i < count; ++i) {
            const gbl_trs& prev = p->prev_to_world[i];
            const float* f = reinterpret_cast<const float*>(&prev);
            for (size_t k = 0; k < sizeof(gbl_trs) / sizeof(float); ++k)
                if (!std::isfinite(f[k])) return fail(ctx, GBL_ERR_INVALID, who + ": prev_to_world[" + std::to_string(i) + "] is not finite");
            if (memcmp(&prev, &ctx->h_instances[i].to_world, sizeof(gbl_trs)) == 0) continue;   // bitwise: an unmoved instance takes no round trip
            std::string err;
            if (!pack_transform(prev, static_cast<uint32_t>(i), xf + GBL_MOTION_XF_FLOATS * i, xf + GBL_MOTION_XF_FLOATS * i + 12, &err))
                return fail(ctx, GBL_ERR_INVALID, who + ": prev_to_world: " + err);
            moved[i] = 1u;
            any_moved = true;
        }
    }
    // The previous poses of the meshes that deformed (motion_stage.h): the per-mesh table, then their positions, in one block
    MotionStage stage;
    std::vector<unsigned char> staged_deform;
    const uint64_t table_bytes = static_cast<uint64_t>(ctx->h_meshes.size()) * sizeof(int32_t);
    std::vector<PoseCopy> copies;
    uint64_t packed_vertices = 0;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = static_cast<hipStream_t>(p->stream);
    if (num_prev_meshes > 0 && device_poses) {
        // (its launches read the caller's memory and the context's positions and write words of their own: the context's tables
        //  are untouched until every refusal is past)
        const gbl_status st = stage_device_poses(ctx, prev_meshes, num_prev_meshes, who_name, stream, &stage.table, &copies, &packed_vertices);
        if (st != GBL_OK) return st;
        if (!copies.empty()) staged_deform.assign(reinterpret_cast<const unsigned char*>(stage.table.data()), reinterpret_cast<const unsigned char*>(stage.table.data()) + table_bytes);
    } else if (num_prev_meshes > 0) {
        std::string err;
        for (uint32_t k = 0; prev_meshes && k < num_prev_meshes; ++k) {   // a device edit may have left a listed mesh's mirror behind
            const gbl_status st = prev_meshes[k].mesh < ctx->h_meshes.size() ? refresh_mirror(ctx, prev_meshes[k].mesh) : GBL_OK;
            if (st != GBL_OK) return st;
        }
        if (!stage_motion_meshes(ctx->h_meshes.data(), ctx->h_meshes.size(), ctx->h_positions.data(), prev_meshes, num_prev_meshes, who_name, &stage, &err))
            return fail(ctx, GBL_ERR_INVALID, err);
        if (stage.any()) {
            staged_deform.resize(table_bytes + stage.packed.size() * sizeof(float));
            memcpy(staged_deform.data(), stage.table.data(), table_bytes);
            memcpy(staged_deform.data() + table_bytes, stage.packed.data(), stage.packed.size() * sizeof(float));
            packed_vertices = stage.packed.size() / 3;
        }
    }
    const bool any_deformed = packed_vertices > 0;
    MotionArgs a;
    memset(&a, 0, sizeof(a));
    a.W = width;
    a.H = height;
    pack_camera(p->prev_camera, ctx->h_film, &a.prev);
    a.normal = reinterpret_cast<const float4*>(p->normal_accum);
    a.out = reinterpret_cast<float4*>(motion_out);
    if (any_moved) {
        gbl_status st;
        if ((st = grow(ctx, ctx->motion, xf_bytes + flag_bytes, "previous instance transforms")) != GBL_OK) return st;
        // the staging copy is the context's, so it outlives the call; a pageable source is read before the copy call returns
        ctx->h_motion.swap(staged);
        HIP_TRY(ctx, hipMemcpyAsync(ctx->motion.p, ctx->h_motion.data(), xf_bytes + flag_bytes, hipMemcpyHostToDevice, stream));
        a.prev_xf = static_cast<const float*>(ctx->motion.p);
        a.moved = reinterpret_cast<const uint32_t*>(static_cast<const unsigned char*>(ctx->motion.p) + xf_bytes);
    }
    if (any_deformed) {
        gbl_status st;
        if ((st = grow(ctx, ctx->motion_deform, table_bytes + packed_vertices * 3 * sizeof(float), "previous vertex positions")) != GBL_OK) return st;
        ctx->h_motion_deform.swap(staged_deform);   // (the context's, as h_motion above)
        HIP_TRY(ctx, hipMemcpyAsync(ctx->motion_deform.p, ctx->h_motion_deform.data(), ctx->h_motion_deform.size(), hipMemcpyHostToDevice, stream));
        for (const PoseCopy& c : copies)   // device poses: the table came from the host, the positions come from where they are
            HIP_TRY(ctx, hipMemcpyAsync(static_cast<unsigned char*>(ctx->motion_deform.p) + table_bytes + c.first_vertex * 3 * sizeof(float), c.src,
                                        c.vertex_count * 3 * sizeof(float), hipMemcpyDeviceToDevice, stream));
        a.mesh_prev = static_cast<const int32_t*>(ctx->motion_deform.p);
        a.prev_pos = reinterpret_cast<const float*>(static_cast<const unsigned char*>(ctx->motion_deform.p) + table_bytes);
        a.num_meshes = static_cast<uint32_t>(ctx->h_meshes.size());
        a.prev_count = static_cast<uint32_t>(packed_vertices);
    }
    // Kernel: the packet for the lean scenes it serves (as gbl_render_aov chooses), one ray per lane otherwise; the DEFORM
    // flavours only when some mesh is deformed, so a call without one launches gbl_render_motion's code.  None of the flavours
    // is compiled with the tie rule (kernels/motion.h traces with TIES = false, lean and EXT alike): no gbl_render_motion* reads
    // tri_order, and a pending tie order (make_pending_orders) stays pending
    const bool ext = sc.extended != 0;
    const bool packet = !ext && sc.stack_entries <= 64;   // (kernels/packet.h GBL_PACKET_STACK)
    gbl_motion_kernel kernel = gbl_kernel_motion(packet, ext, any_deformed);
    const size_t lds = stack_lds_bytes(sc);
    gbl_status st;
    if ((st = allow_lds(ctx, kernel, lds + (packet ? 4096 : 0))) != GBL_OK) return st;   // (the packet kernel's static 3 KB count against the same limit)
    const unsigned tiles = static_cast<unsigned>(((width + GBL_TILE - 1) / GBL_TILE) * ((height + GBL_TILE - 1) / GBL_TILE));
    const unsigned per_block = GBL_BLOCK / 64;
    hipLaunchKernelGGL(kernel, dim3((tiles + per_block - 1) / per_block), dim3(GBL_BLOCK), lds, stream, sc, a);
    HIP_TRY(ctx, hipGetLastError());
    return GBL_OK;
}

}   // namespace

extern "C" {

gbl_status gbl_get_instances(const gbl_ctx* ctx, uint32_t first, uint32_t count, gbl_trs* out) {
    return gbl_guard([&] { return gbl_get_instances_impl(ctx, first, count, out); }, [&](const std::string&) {});
}

gbl_status gbl_render_motion(gbl_ctx* ctx, const gbl_motion_params* params, float* motion_out) {
    return gbl_guard([&] { return gbl_render_motion_impl(ctx, params, nullptr, 0, motion_out, "gbl_render_motion"); }, [&](const std::string& what) { if (ctx) ctx->error = what; });
}

gbl_status gbl_render_motion_deform(gbl_ctx* ctx, const gbl_motion_params* params, const gbl_motion_mesh* prev_meshes, uint32_t num_prev_meshes, float* motion_out) {
    return gbl_guard([&] { return gbl_render_motion_impl(ctx, params, prev_meshes, num_prev_meshes, motion_out, "gbl_render_motion_deform"); },
                     [&](const std::string& what) { if (ctx) ctx->error = what; });
}

gbl_status gbl_render_motion_deform_device(gbl_ctx* ctx, const gbl_motion_params* params, const gbl_motion_mesh* prev_meshes, uint32_t num_prev_meshes,
                                           float* motion_out) {
    return gbl_guard([&] { return gbl_render_motion_impl(ctx, params, prev_meshes, num_prev_meshes, motion_out, "gbl_render_motion_deform_device", true); },
                     [&](const std::string& what) { if (ctx) ctx->error = what; });
}

}  // extern "C"
