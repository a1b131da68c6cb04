// libgoblin_hip.so -- C ABI of the device integrator (include/goblin_hip.h): vertex edits.  gbl_update_vertices refits a
// mesh's BLAS on the device in place (kernels/refit.h over the plan of scene_refit.h); gbl_get_vertices and the
// geometry tables' read-back go with it.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gbl_host.h"
#include "scene_prep.h"
#include "scene_refit.h"

namespace {

// The mesh's refit plan, built at its first edit: the node array is downloaded once per context, walked on the host, and the
// plan is checked there (build_refit_plan) before the kernels may index from it.
gbl_status ensure_plan(gbl_ctx* ctx, uint32_t mesh) {
    gbl_ctx::MeshRefit& mr = ctx->refit[mesh];
    if (mr.built) return GBL_OK;
    const gbl_mesh& gm = ctx->h_meshes[mesh];
    const uint32_t tri_first = ctx->mesh_tri_first[mesh];
    if (static_cast<uint64_t>(tri_first) + gm.tri_count > ctx->info.triangles)
        return fail(ctx, GBL_ERR_INTERNAL, "gbl_update_vertices: the mesh's triangles lie outside the triangle table");
    if (ctx->h_nodes.empty() && ctx->num_nodes > 0) {
        ctx->h_nodes.resize(ctx->num_nodes);
        const hipError_t e = hipMemcpy(ctx->h_nodes.data(), ctx->scene.nodes, ctx->num_nodes * sizeof(DevNode), hipMemcpyDeviceToHost);
        if (e != hipSuccess) {
            ctx->h_nodes.clear();
            return fail(ctx, GBL_ERR_DEVICE, std::string("gbl_update_vertices: node download: ") + hipGetErrorString(e));
        }
    }
    RefitPlan plan;
    std::string err;
    if (!build_refit_plan(ctx->h_nodes.data(), ctx->h_nodes.size(), ctx->mesh_root[mesh], tri_first, gm.tri_count, &plan, &err))
        return fail(ctx, GBL_ERR_INTERNAL, "gbl_update_vertices: " + err);
    if (!plan.records.empty()) {
        gbl_status st = device_alloc(ctx, plan.records.size() * sizeof(RefitRecord), "refit plan", reinterpret_cast<void**>(&mr.plan));
        if (st == GBL_OK) st = device_alloc(ctx, plan.records.size() * sizeof(RefitBox), "refit boxes", reinterpret_cast<void**>(&mr.node_box));
        if (st != GBL_OK) return st;
        HIP_TRY(ctx, hipMemcpy(mr.plan, plan.records.data(), plan.records.size() * sizeof(RefitRecord), hipMemcpyHostToDevice));
    }
    mr.level_first.swap(plan.level_first);
    mr.built = true;
    return GBL_OK;
}

gbl_status gbl_update_vertices_impl(gbl_ctx* ctx, uint32_t mesh, uint32_t first, uint32_t count, const float* positions, const float* normals) {
    if (!ctx) return GBL_ERR_INVALID;
    if (!positions) return fail(ctx, GBL_ERR_INVALID, "gbl_update_vertices: positions is NULL");
    if (mesh >= ctx->h_meshes.size()) return fail(ctx, GBL_ERR_INVALID, "gbl_update_vertices: mesh " + std::to_string(mesh) + " is out of range");
    const gbl_mesh& gm = ctx->h_meshes[mesh];
    if (gm.shape != GBL_SHAPE_MESH) return fail(ctx, GBL_ERR_INVALID, "gbl_update_vertices: mesh " + std::to_string(mesh) + " is a sphere or a disk: it has no vertices");
    if (static_cast<uint64_t>(first) + count > gm.vertex_count) return fail(ctx, GBL_ERR_INVALID, "gbl_update_vertices: vertex range out of bounds");
    for (size_t i = 0; i < 3 * static_cast<size_t>(count); ++i)
        if (!std::isfinite(positions[i]) || (normals && !std::isfinite(normals[i])))
            return fail(ctx, GBL_ERR_INVALID, std::string("gbl_update_vertices: a ") + (std::isfinite(positions[i]) ? "normal" : "position") + " of vertex " +
                                                  std::to_string(first + i / 3) + " is not finite");
    if (normals && !gm.has_normal) return fail(ctx, GBL_ERR_INVALID, "gbl_update_vertices: normals given for a mesh without vertex normals (has_normal)");
    if (ctx->mesh_emits[mesh])
        return fail(ctx, GBL_ERR_UNSUPPORTED, "gbl_update_vertices: mesh " + std::to_string(mesh) + " is the geometry of an area light, whose emitting "
                                              "triangles, area distribution and power would have to follow; re-create the context instead");
    if (ctx->has_directional)
        return fail(ctx, GBL_ERR_UNSUPPORTED, "gbl_update_vertices: a directional or image based light's power (and the image based light's sampling sphere) "
                                              "depends on the scene bound (GoblinLight.cpp:203-210, 590-629); re-create the context instead");
    const auto now = [] { return std::chrono::steady_clock::now(); };
    const auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    const auto t0 = now();
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipDeviceSynchronize());   // no render may be reading the tables
    gbl_status st = ensure_plan(ctx, mesh);
    if (st != GBL_OK) return st;
    const gbl_ctx::MeshRefit& mr = ctx->refit[mesh];
    DevScene& sc = ctx->scene;
    const size_t v0 = static_cast<size_t>(gm.vertex_offset) + first, floats = 3 * static_cast<size_t>(count);
    if (count > 0) {
        memcpy(ctx->h_positions.data() + 3 * v0, positions, floats * sizeof(float));
        HIP_TRY(ctx, hipMemcpy(const_cast<float*>(sc.positions) + 3 * v0, positions, floats * sizeof(float), hipMemcpyHostToDevice));
        if (normals) HIP_TRY(ctx, hipMemcpy(const_cast<float*>(sc.normals) + 3 * v0, normals, floats * sizeof(float), hipMemcpyHostToDevice));
    }
    // triangles and their bounds, then the nodes from the deepest level to the root (the stream orders the launches)
    gbl_launch_refit_tris(const_cast<DevTri*>(sc.tris), const_cast<DevTriBound*>(sc.tri_bounds), sc.tri_shade, sc.positions,
                          static_cast<uint32_t>(ctx->h_positions.size() / 3), ctx->mesh_tri_first[mesh], gm.tri_count, 0);
    for (size_t l = mr.level_first.size(); l-- > 1;)
        gbl_launch_refit_level(const_cast<DevNode*>(sc.nodes), sc.tri_bounds, mr.plan, mr.node_box, mr.level_first[l - 1], mr.level_first[l], 0);
    HIP_TRY(ctx, hipGetLastError());
    const auto t1 = now();
    // while the device works: the reference's visiting order over the edited positions (what exact_ties, replay, stream and the
    // EXT builds break ties by), and the mesh's object bound
    const float* mesh_pos = ctx->h_positions.data() + 3 * static_cast<size_t>(gm.vertex_offset);
    std::vector<DevTriOrder> order(gm.tri_count);
    mesh_reference_order(mesh_pos, ctx->h_indices.data() + 3 * static_cast<size_t>(gm.tri_offset), gm.tri_count, order.data());
    if (!order.empty())
        HIP_TRY(ctx, hipMemcpy(const_cast<DevTriOrder*>(sc.tri_order) + gm.tri_offset, order.data(), order.size() * sizeof(DevTriOrder), hipMemcpyHostToDevice));
    const auto t2 = now();
    mesh_object_bound(mesh_pos, gm.vertex_count, &ctx->mesh_lo[3 * mesh], &ctx->mesh_hi[3 * mesh]);
    std::vector<gbl_instance> instances = ctx->h_instances;
    st = rebuild_tlas(ctx, instances, "gbl_update_vertices");   // (synchronises before its uploads, and clears the AUTO pilot)
    if (st != GBL_OK) return st;
    HIP_TRY(ctx, hipDeviceSynchronize());
    if (getenv("GBL_PROBE"))
        fprintf(stderr, "probe: gbl_update_vertices mesh %u (%u triangles, %zu refit levels): synchronise, plan, uploads and launches %.3f ms, tri_order on the host and "
                        "its upload (behind the kernels) %.3f ms, mesh bound and TLAS %.3f ms\n", mesh, gm.tri_count, mr.level_first.empty() ? size_t(0) : mr.level_first.size() - 1,
                ms(t0, t1), ms(t1, t2), ms(t2, now()));
    return GBL_OK;
}

gbl_status gbl_get_vertices_impl(const gbl_ctx* ctx, uint32_t mesh, uint32_t first, uint32_t count, float* positions_out) {
    if (!ctx || !positions_out || mesh >= ctx->h_meshes.size()) return GBL_ERR_INVALID;
    const gbl_mesh& gm = ctx->h_meshes[mesh];
    if (gm.shape != GBL_SHAPE_MESH || static_cast<uint64_t>(first) + count > gm.vertex_count) return GBL_ERR_INVALID;
    if (count > 0) memcpy(positions_out, ctx->h_positions.data() + 3 * (static_cast<size_t>(gm.vertex_offset) + first), 3 * static_cast<size_t>(count) * sizeof(float));
    return GBL_OK;
}

gbl_status gbl_selftest_geometry_impl(gbl_ctx* ctx, int table, uint64_t first, uint64_t count, void* out, uint64_t* total) {
    if (!ctx) return GBL_ERR_INVALID;
    const DevScene& sc = ctx->scene;
    const void* base[4] = {sc.nodes, sc.tris, sc.tri_bounds, sc.tri_order};
    const uint64_t size[5] = {sizeof(DevNode), sizeof(DevTri), sizeof(DevTriBound), sizeof(DevTriOrder), sizeof(int32_t)};
    if (table < 0 || table > 4)
        return fail(ctx, GBL_ERR_INVALID, "gbl_selftest_geometry: table must be 0 (nodes), 1 (tris), 2 (tri_bounds), 3 (tri_order) or 4 (mesh_root)");
    const uint64_t records[5] = {ctx->num_nodes, ctx->info.triangles, ctx->info.triangles, ctx->h_indices.size() / 3, ctx->mesh_root.size()};
    if (total) *total = records[table];
    if (first > records[table] || count > records[table] - first) return fail(ctx, GBL_ERR_INVALID, "gbl_selftest_geometry: record range out of bounds");
    if (count == 0) return GBL_OK;
    if (!out) return fail(ctx, GBL_ERR_INVALID, "gbl_selftest_geometry: out is NULL");
    if (table == 4) {   // host side: what the instances' `root` fields were filled from
        memcpy(out, ctx->mesh_root.data() + first, count * sizeof(int32_t));
        return GBL_OK;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipDeviceSynchronize());
    HIP_TRY(ctx, hipMemcpy(out, static_cast<const unsigned char*>(base[table]) + first * size[table], count * size[table], hipMemcpyDeviceToHost));
    return GBL_OK;
}

}   // namespace

extern "C" {

gbl_status gbl_update_vertices(gbl_ctx* ctx, uint32_t mesh, uint32_t first, uint32_t count, const float* positions, const float* normals) {
    return gbl_guard([&] { return gbl_update_vertices_impl(ctx, mesh, first, count, positions, normals); }, [&](const std::string& what) { if (ctx) ctx->error = what; });
}

gbl_status gbl_get_vertices(const gbl_ctx* ctx, uint32_t mesh, uint32_t first, uint32_t count, float* positions_out) {
    return gbl_guard([&] { return gbl_get_vertices_impl(ctx, mesh, first, count, positions_out); }, [&](const std::string&) {});
}

gbl_status gbl_selftest_geometry(gbl_ctx* ctx, int table, uint64_t first, uint64_t count, void* out, uint64_t* total) {
    return gbl_guard([&] { return gbl_selftest_geometry_impl(ctx, table, first, count, out, total); }, [&](const std::string& what) { if (ctx) ctx->error = what; });
}

}   // extern "C"
