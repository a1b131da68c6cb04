// libgoblin_hip.so -- C ABI of the device integrator (include/goblin_hip.h): gbl_get_instances, gbl_render_motion and
// gbl_render_motion_deform, the per-pixel "where was this surface point in the previous frame" (kernels/motion.h).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>

#include "gbl_host.h"
#include "motion_stage.h"
#include "scene_prep.h"

namespace {

gbl_status gbl_get_instances_impl(const gbl_ctx* ctx, uint32_t first, uint32_t count, gbl_trs* out) {
    if (!ctx || !out || static_cast<uint64_t>(first) + count > ctx->h_instances.size()) return GBL_ERR_INVALID;
    for (uint32_t i = 0; i < count; ++i) out[i] = ctx->h_instances[first + i].to_world;
    return GBL_OK;
}

// gbl_render_motion (prev_meshes NULL, num_prev_meshes 0) and gbl_render_motion_deform; `who` starts the error messages
gbl_status gbl_render_motion_impl(gbl_ctx* ctx, const gbl_motion_params* p, const gbl_motion_mesh* prev_meshes, uint32_t num_prev_meshes, float* motion_out,
                                  const char* who_name) {
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
    if (num_prev_meshes > 0) {
        std::string err;
        if (!stage_motion_meshes(ctx->h_meshes.data(), ctx->h_meshes.size(), ctx->h_positions.data(), prev_meshes, num_prev_meshes, who_name, &stage, &err))
            return fail(ctx, GBL_ERR_INVALID, err);
        if (stage.any()) {
            staged_deform.resize(table_bytes + stage.packed.size() * sizeof(float));
            memcpy(staged_deform.data(), stage.table.data(), table_bytes);
            memcpy(staged_deform.data() + table_bytes, stage.packed.data(), stage.packed.size() * sizeof(float));
        }
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = static_cast<hipStream_t>(p->stream);
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
    if (stage.any()) {
        gbl_status st;
        if ((st = grow(ctx, ctx->motion_deform, staged_deform.size(), "previous vertex positions")) != GBL_OK) return st;
        ctx->h_motion_deform.swap(staged_deform);   // (the context's, as h_motion above)
        HIP_TRY(ctx, hipMemcpyAsync(ctx->motion_deform.p, ctx->h_motion_deform.data(), ctx->h_motion_deform.size(), hipMemcpyHostToDevice, stream));
        a.mesh_prev = static_cast<const int32_t*>(ctx->motion_deform.p);
        a.prev_pos = reinterpret_cast<const float*>(static_cast<const unsigned char*>(ctx->motion_deform.p) + table_bytes);
        a.num_meshes = static_cast<uint32_t>(ctx->h_meshes.size());
        a.prev_count = static_cast<uint32_t>(stage.packed.size() / 3);
    }
    // Kernel: the packet for the lean scenes it serves (as gbl_render_aov chooses), one ray per lane otherwise; the DEFORM
    // flavours only when some mesh is deformed, so a call without one launches gbl_render_motion's code
    const bool ext = sc.extended != 0;
    const bool packet = !ext && sc.stack_entries <= 64;   // (kernels/packet.h GBL_PACKET_STACK)
    gbl_motion_kernel kernel = gbl_kernel_motion(packet, ext, stage.any());
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

}  // extern "C"
