// libgoblin_hip.so -- C ABI of the device integrator (include/goblin_hip.h): vertex edits.  gbl_update_vertices refits a
// mesh's BLAS on the device in place (kernels/refit.h over the plan of scene_refit.h); gbl_get_vertices and the
// geometry tables' read-back go with it.  gbl_update_vertices_device and gbl_get_vertices_device are the same two over device
// memory (kernels/vertices.h): the host copy of the positions turns into a mirror refreshed on demand, and the tie order may
// wait for its first reader (make_pending_orders, gbl_host.h).  gbl_rebuild_mesh builds a deformed mesh's tree again with the
// device builder (kernels/lbvh.h), and gbl_mesh_tree_stats (kernels/treestats.h) tells a caller when that pays.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gbl_host.h"
#include "scene_prep.h"
#include "scene_refit.h"

gbl_status refresh_mirror(gbl_ctx* ctx, uint32_t mesh) {
    if (mesh >= ctx->mirror_stale.size() || !ctx->mirror_stale[mesh]) return GBL_OK;
    const gbl_mesh& gm = ctx->h_meshes[mesh];
    const size_t f0 = 3 * static_cast<size_t>(gm.vertex_offset), floats = 3 * static_cast<size_t>(gm.vertex_count);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (floats > 0) HIP_TRY(ctx, hipMemcpy(ctx->h_positions.data() + f0, ctx->scene.positions + f0, floats * sizeof(float), hipMemcpyDeviceToHost));
    ctx->mirror_stale[mesh] = 0;
    return GBL_OK;
}

gbl_status check_device_pointer(gbl_ctx* ctx, const void* p, uint64_t bytes, const std::string& who, const char* what) {
    hipPointerAttribute_t attr;
    memset(&attr, 0, sizeof(attr));
    const hipError_t e = hipPointerGetAttributes(&attr, p);
    if (e != hipSuccess) (void)hipGetLastError();   // (a plain host pointer: the runtime would hand the error to the next call that asks)
    if (e != hipSuccess || (attr.type != hipMemoryTypeDevice && attr.type != hipMemoryTypeManaged) || attr.device != ctx->device)
        return fail(ctx, GBL_ERR_INVALID, who + ": " + what + " is not device memory of device " + std::to_string(ctx->device));
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void*>(p)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(ctx, GBL_ERR_INVALID, who + ": " + what + ": the allocation it points into is not known");
    }
    const uint64_t at = static_cast<uint64_t>(reinterpret_cast<uintptr_t>(p) - reinterpret_cast<uintptr_t>(base));
    if (at > size || size - at < bytes)
        return fail(ctx, GBL_ERR_INVALID, who + ": " + what + ": its allocation ends after " + std::to_string(size - std::min<uint64_t>(at, size)) + " bytes, " +
                                              std::to_string(bytes) + " are read or written");
    return GBL_OK;
}

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
    mr.leaves = plan.records.empty() ? 1u : 0u;   // (a root that is itself a leaf)
    for (const RefitRecord& rec : plan.records)
        for (int c = 0; c < 4; ++c) mr.leaves += ctx->h_nodes[rec.node].child[c] < 0 ? 1u : 0u;
    mr.level_first.swap(plan.level_first);
    mr.built = true;
    return GBL_OK;
}

// Forget the mesh's refit plan (its tree is about to be replaced): the next edit, or gbl_mesh_tree_stats, makes it again
void drop_plan(gbl_ctx* ctx, uint32_t mesh) {
    gbl_ctx::MeshRefit& mr = ctx->refit[mesh];
    device_free(ctx, mr.plan);
    device_free(ctx, mr.node_box);
    mr = gbl_ctx::MeshRefit();
}

// The node array regrown by `extra` zeroed records behind the ones it holds: every index stays valid, tlas_base included.  The
// caller has synchronised the device; the old array is freed once the copy is done.
gbl_status grow_nodes(gbl_ctx* ctx, uint32_t extra, int32_t* first_new) {
    const uint64_t old_n = ctx->num_nodes, new_n = old_n + extra;
    if (new_n >= static_cast<uint64_t>(GBL_REF_NONE)) return fail(ctx, GBL_ERR_UNSUPPORTED, "gbl_rebuild_mesh: the node array would outgrow a child reference");
    void* grown = nullptr;
    const gbl_status st = device_alloc(ctx, new_n * sizeof(DevNode), "nodes", &grown);
    if (st != GBL_OK) return st;
    DevNode* const old = const_cast<DevNode*>(ctx->scene.nodes);
    if (old_n > 0) HIP_TRY(ctx, hipMemcpy(grown, old, old_n * sizeof(DevNode), hipMemcpyDeviceToDevice));
    HIP_TRY(ctx, hipMemset(static_cast<DevNode*>(grown) + old_n, 0, extra * sizeof(DevNode)));
    HIP_TRY(ctx, hipDeviceSynchronize());
    device_free(ctx, old);
    ctx->scene.nodes = static_cast<const DevNode*>(grown);
    ctx->num_nodes = new_n;
    ctx->info.scene_bytes += static_cast<uint64_t>(extra) * sizeof(DevNode);
    *first_new = static_cast<int32_t>(old_n);
    return GBL_OK;
}

// What both vertex edits refuse before they look at a coordinate, in gbl_update_vertices' order and words
gbl_status check_edit_range(gbl_ctx* ctx, uint32_t mesh, uint32_t first, uint32_t count, const float* positions) {
    if (!positions) return fail(ctx, GBL_ERR_INVALID, "gbl_update_vertices: positions is NULL");
    if (mesh >= ctx->h_meshes.size()) return fail(ctx, GBL_ERR_INVALID, "gbl_update_vertices: mesh " + std::to_string(mesh) + " is out of range");
    const gbl_mesh& gm = ctx->h_meshes[mesh];
    if (gm.shape != GBL_SHAPE_MESH) return fail(ctx, GBL_ERR_INVALID, "gbl_update_vertices: mesh " + std::to_string(mesh) + " is a sphere or a disk: it has no vertices");
    if (static_cast<uint64_t>(first) + count > gm.vertex_count) return fail(ctx, GBL_ERR_INVALID, "gbl_update_vertices: vertex range out of bounds");
    return GBL_OK;
}

// ... and after they have: float `i` of the edit is not finite, in its positions or else in its normals
gbl_status fail_not_finite(gbl_ctx* ctx, uint32_t first, size_t i, bool position) {
    return fail(ctx, GBL_ERR_INVALID, std::string("gbl_update_vertices: a ") + (position ? "position" : "normal") + " of vertex " + std::to_string(first + i / 3) + " is not finite");
}

gbl_status check_edit_allowed(gbl_ctx* ctx, uint32_t mesh, bool normals) {
    if (normals && !ctx->h_meshes[mesh].has_normal) return fail(ctx, GBL_ERR_INVALID, "gbl_update_vertices: normals given for a mesh without vertex normals (has_normal)");
    if (ctx->mesh_emits[mesh])
        return fail(ctx, GBL_ERR_UNSUPPORTED, "gbl_update_vertices: mesh " + std::to_string(mesh) + " is the geometry of an area light, whose emitting "
                                              "triangles, area distribution and power would have to follow; re-create the context instead");
    return refuse_scene_bound_edit(ctx, "gbl_update_vertices");
}

// The refit launches over the mesh's positions as the device holds them: triangles and their bounds, then the nodes from the
// deepest level to the root (the stream orders the launches)
void launch_refit(gbl_ctx* ctx, uint32_t mesh) {
    const gbl_ctx::MeshRefit& mr = ctx->refit[mesh];
    const DevScene& sc = ctx->scene;
    gbl_launch_refit_tris(const_cast<DevTri*>(sc.tris), const_cast<DevTriBound*>(sc.tri_bounds), sc.tri_shade, sc.positions,
                          static_cast<uint32_t>(ctx->h_positions.size() / 3), ctx->mesh_tri_first[mesh], ctx->h_meshes[mesh].tri_count, 0);
    for (size_t l = mr.level_first.size(); l-- > 1;)
        gbl_launch_refit_level(const_cast<DevNode*>(sc.nodes), sc.tri_bounds, mr.plan, mr.node_box, mr.level_first[l - 1], mr.level_first[l], 0);
}

// The reference's visiting order over the mesh's positions as the (fresh) mirror holds them -- what exact_ties, replay, stream
// and the EXT builds break ties by -- into the mesh's slice of tri_order; the mesh is no longer pending
gbl_status make_order(gbl_ctx* ctx, uint32_t mesh) {
    const gbl_mesh& gm = ctx->h_meshes[mesh];
    std::vector<DevTriOrder> order(gm.tri_count);
    mesh_reference_order(ctx->h_positions.data() + 3 * static_cast<size_t>(gm.vertex_offset), ctx->h_indices.data() + 3 * static_cast<size_t>(gm.tri_offset), gm.tri_count,
                         order.data());
    if (!order.empty())
        HIP_TRY(ctx, hipMemcpy(const_cast<DevTriOrder*>(ctx->scene.tri_order) + gm.tri_offset, order.data(), order.size() * sizeof(DevTriOrder), hipMemcpyHostToDevice));
    if (mesh < ctx->order_pending.size() && ctx->order_pending[mesh]) {
        ctx->order_pending[mesh] = 0;
        ctx->orders_pending -= 1;
    }
    return GBL_OK;
}

gbl_status gbl_update_vertices_impl(gbl_ctx* ctx, uint32_t mesh, uint32_t first, uint32_t count, const float* positions, const float* normals) {
    if (!ctx) return GBL_ERR_INVALID;
    gbl_status st = check_edit_range(ctx, mesh, first, count, positions);
    if (st != GBL_OK) return st;
    const gbl_mesh& gm = ctx->h_meshes[mesh];
    for (size_t i = 0; i < 3 * static_cast<size_t>(count); ++i)
        if (!std::isfinite(positions[i]) || (normals && !std::isfinite(normals[i]))) return fail_not_finite(ctx, first, i, !std::isfinite(positions[i]));
    if ((st = check_edit_allowed(ctx, mesh, normals != nullptr)) != GBL_OK) return st;
    LapClock clock;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipDeviceSynchronize());   // no render may be reading the tables
    if ((st = ensure_plan(ctx, mesh)) != GBL_OK) return st;
    if ((st = refresh_mirror(ctx, mesh)) != GBL_OK) return st;   // (a device edit may have left the mirror behind: the patch goes onto the current positions)
    const gbl_ctx::MeshRefit& mr = ctx->refit[mesh];
    DevScene& sc = ctx->scene;
    const size_t v0 = static_cast<size_t>(gm.vertex_offset) + first, floats = 3 * static_cast<size_t>(count);
    if (count > 0) {
        memcpy(ctx->h_positions.data() + 3 * v0, positions, floats * sizeof(float));
        HIP_TRY(ctx, hipMemcpy(const_cast<float*>(sc.positions) + 3 * v0, positions, floats * sizeof(float), hipMemcpyHostToDevice));
        if (normals) HIP_TRY(ctx, hipMemcpy(const_cast<float*>(sc.normals) + 3 * v0, normals, floats * sizeof(float), hipMemcpyHostToDevice));
    }
    launch_refit(ctx, mesh);
    HIP_TRY(ctx, hipGetLastError());
    const double launch_ms = clock.lap_ms();
    // while the device works: the reference's visiting order over the edited positions (what exact_ties, replay, stream and the
    // EXT builds break ties by), and the mesh's object bound
    if ((st = make_order(ctx, mesh)) != GBL_OK) return st;
    const double order_ms = clock.lap_ms();
    mesh_object_bound(ctx->h_positions.data() + 3 * static_cast<size_t>(gm.vertex_offset), gm.vertex_count, &ctx->mesh_lo[3 * mesh], &ctx->mesh_hi[3 * mesh]);
    if ((st = retlas_after_geometry_edit(ctx, "gbl_update_vertices")) != GBL_OK) return st;
    if (probing())
        fprintf(stderr, "probe: gbl_update_vertices mesh %u (%u triangles, %zu refit levels): synchronise, plan, uploads and launches %.3f ms, tri_order on the host and "
                        "its upload (behind the kernels) %.3f ms, mesh bound and TLAS %.3f ms\n", mesh, gm.tri_count, mr.level_first.empty() ? size_t(0) : mr.level_first.size() - 1,
                launch_ms, order_ms, clock.lap_ms());
    return GBL_OK;
}

// gbl_update_vertices over device memory.  Every refusal the host can make comes first; the finiteness check is the one launch
// ahead of the context's first change.
gbl_status gbl_update_vertices_device_impl(gbl_ctx* ctx, uint32_t mesh, uint32_t first, uint32_t count, const float* d_positions, const float* d_normals,
                                           uint32_t flags) {
    if (!ctx) return GBL_ERR_INVALID;
    gbl_status st = check_edit_range(ctx, mesh, first, count, d_positions);
    if (st != GBL_OK) return st;
    if (flags & ~GBL_VERTICES_DEFER_ORDER) return fail(ctx, GBL_ERR_INVALID, "gbl_update_vertices_device: unknown bits in flags");
    if ((st = check_edit_allowed(ctx, mesh, d_normals != nullptr)) != GBL_OK) return st;
    const gbl_mesh& gm = ctx->h_meshes[mesh];
    const uint64_t floats = 3 * static_cast<uint64_t>(count);
    if (3 * static_cast<uint64_t>(gm.vertex_count) >= 0xFFFFFFFFull)
        return fail(ctx, GBL_ERR_UNSUPPORTED, "gbl_update_vertices_device: a mesh of 2^32 / 3 vertices or more (the check word holds a float's index)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((st = check_device_pointer(ctx, d_positions, floats * sizeof(float), "gbl_update_vertices_device", "d_positions")) != GBL_OK) return st;
    if (d_normals && (st = check_device_pointer(ctx, d_normals, floats * sizeof(float), "gbl_update_vertices_device", "d_normals")) != GBL_OK) return st;
    LapClock clock;
    if (!ctx->vertex_words.p && (st = grow(ctx, ctx->vertex_words, GBL_VW_BYTES, "vertex edit words")) != GBL_OK) return st;
    unsigned char* words = static_cast<unsigned char*>(ctx->vertex_words.p);
    HIP_TRY(ctx, hipDeviceSynchronize());   // no render may be reading the tables, and whatever wrote the caller's floats is done
    HIP_TRY(ctx, hipMemsetAsync(words, 0xFF, GBL_VW_FILL, 0));
    if (count > 0) {
        uint32_t bad = 0xFFFFFFFFu;
        gbl_launch_vertices_check(d_positions, d_normals, static_cast<uint32_t>(floats), reinterpret_cast<uint32_t*>(words + GBL_VW_CHECK), 0);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpy(&bad, words + GBL_VW_CHECK, sizeof(bad), hipMemcpyDeviceToHost));
        if (bad != 0xFFFFFFFFu) {   // which of the two at that index: a position comes before a normal
            if (bad >= floats) return fail(ctx, GBL_ERR_INTERNAL, "gbl_update_vertices_device: the check word is out of range");
            float v = 0.0f;
            HIP_TRY(ctx, hipMemcpy(&v, d_positions + bad, sizeof(v), hipMemcpyDeviceToHost));
            return fail_not_finite(ctx, first, bad, !std::isfinite(v));
        }
    }
    const double check_ms = clock.lap_ms();
    if ((st = ensure_plan(ctx, mesh)) != GBL_OK) return st;
    DevScene& sc = ctx->scene;
    const size_t m0 = 3 * static_cast<size_t>(gm.vertex_offset), v0 = m0 + 3 * static_cast<size_t>(first);
    if (ctx->mirror_stale.size() != ctx->h_meshes.size()) ctx->mirror_stale.assign(ctx->h_meshes.size(), 0);
    if (ctx->order_pending.size() != ctx->h_meshes.size()) ctx->order_pending.assign(ctx->h_meshes.size(), 0);
    if (count > 0) {
        ctx->mirror_stale[mesh] = 1;
        HIP_TRY(ctx, hipMemcpyAsync(const_cast<float*>(sc.positions) + v0, d_positions, floats * sizeof(float), hipMemcpyDeviceToDevice, 0));
        if (d_normals) HIP_TRY(ctx, hipMemcpyAsync(const_cast<float*>(sc.normals) + v0, d_normals, floats * sizeof(float), hipMemcpyDeviceToDevice, 0));
    }
    launch_refit(ctx, mesh);
    gbl_launch_mesh_bound(sc.positions + m0, gm.vertex_count, reinterpret_cast<unsigned long long*>(words + GBL_VW_KEYS), reinterpret_cast<float*>(words + GBL_VW_BOUND), 0);
    HIP_TRY(ctx, hipGetLastError());
    const double launch_ms = clock.lap_ms();
    // the tie order: now, on the host over the refreshed mirror (while the device works), or left to its first reader
    if (flags & GBL_VERTICES_DEFER_ORDER) {
        if (!ctx->order_pending[mesh]) {
            ctx->order_pending[mesh] = 1;
            ctx->orders_pending += 1;
        }
    } else {
        if ((st = refresh_mirror(ctx, mesh)) != GBL_OK) return st;
        if ((st = make_order(ctx, mesh)) != GBL_OK) return st;
    }
    const double order_ms = clock.lap_ms();
    float bound[6];
    HIP_TRY(ctx, hipMemcpy(bound, words + GBL_VW_BOUND, sizeof(bound), hipMemcpyDeviceToHost));
    for (int a = 0; a < 3; ++a) ctx->mesh_lo[3 * mesh + a] = bound[a], ctx->mesh_hi[3 * mesh + a] = bound[3 + a];
    if ((st = retlas_after_geometry_edit(ctx, "gbl_update_vertices_device")) != GBL_OK) return st;
    if (probing())
        fprintf(stderr, "probe: gbl_update_vertices_device mesh %u (%u triangles, flags %u): synchronise, check and its word %.3f ms, plan, copies and launches %.3f ms, "
                        "tri_order %.3f ms, bound read-back and TLAS %.3f ms\n", mesh, gm.tri_count, flags, check_ms, launch_ms, order_ms, clock.lap_ms());
    return GBL_OK;
}

// What gbl_rebuild_mesh and gbl_mesh_tree_stats refuse alike: the mesh must be a triangle mesh of the scene
gbl_status check_tree_mesh(gbl_ctx* ctx, uint32_t mesh, const char* who) {
    if (mesh >= ctx->h_meshes.size()) return fail(ctx, GBL_ERR_INVALID, std::string(who) + ": mesh " + std::to_string(mesh) + " is out of range");
    if (ctx->h_meshes[mesh].shape != GBL_SHAPE_MESH)
        return fail(ctx, GBL_ERR_INVALID, std::string(who) + ": mesh " + std::to_string(mesh) + " is a sphere or a disk: it has no tree");
    if (static_cast<uint64_t>(ctx->mesh_tri_first[mesh]) + ctx->h_meshes[mesh].tri_count > ctx->info.triangles)
        return fail(ctx, GBL_ERR_INTERNAL, std::string(who) + ": the mesh's triangles lie outside the triangle table");
    return GBL_OK;
}

// The mesh's BLAS built again by the device builder (kernels/lbvh.h through gbl_build_blas_device) over the positions the
// device holds: triangles in the new Morton order in the mesh's own range, their bounds by refit_tris' rule, the tree in the
// mesh's tail slot of the node array.  Neither tri_order nor the pending state nor the mirror is read or written.
gbl_status gbl_rebuild_mesh_impl(gbl_ctx* ctx, uint32_t mesh, uint32_t flags) {
    if (!ctx) return GBL_ERR_INVALID;
    gbl_status st = check_tree_mesh(ctx, mesh, "gbl_rebuild_mesh");
    if (st != GBL_OK) return st;
    if (flags != 0) return fail(ctx, GBL_ERR_INVALID, "gbl_rebuild_mesh: flags is reserved and must be 0");
    if (ctx->mesh_emits[mesh])
        return fail(ctx, GBL_ERR_UNSUPPORTED, "gbl_rebuild_mesh: mesh " + std::to_string(mesh) + " is the geometry of an area light, whose emitting "
                                              "triangles are listed by their place in the triangle table; re-create the context instead");
    const gbl_mesh& gm = ctx->h_meshes[mesh];
    const uint32_t n = gm.tri_count, tri_first = ctx->mesh_tri_first[mesh];
    if (n == 0) return GBL_OK;
    LapClock clock;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipDeviceSynchronize());   // no render may be reading the tables
    // first rebuild of the mesh: its index slice goes up (a host-built context has none on the device), and a mesh with a tree
    // gets tri_count records behind the node array -- gbl_create's own bound for a device-built mesh -- for good
    if (!ctx->rebuild_idx[mesh]) {
        void* p = nullptr;
        if ((st = device_alloc(ctx, 3 * static_cast<size_t>(n) * sizeof(uint32_t), "rebuild indices", &p)) != GBL_OK) return st;
        HIP_TRY(ctx, hipMemcpy(p, ctx->h_indices.data() + 3 * static_cast<size_t>(gm.tri_offset), 3 * static_cast<size_t>(n) * sizeof(uint32_t), hipMemcpyHostToDevice));
        ctx->rebuild_idx[mesh] = static_cast<uint32_t*>(p);
    }
    if (n > GBL_MAX_LEAF_TRIS && ctx->rebuild_slot[mesh] < 0) {
        if ((st = grow_nodes(ctx, n, &ctx->rebuild_slot[mesh])) != GBL_OK) return st;
        ctx->h_nodes.clear();
    }
    const double slot_ms = clock.lap_ms();
    DevScene& sc = ctx->scene;
    int32_t root = 0;
    uint32_t used = 0;
    int depth = 0;
    st = gbl_build_blas_device(ctx, sc.positions + 3 * static_cast<size_t>(gm.vertex_offset), ctx->rebuild_idx[mesh], n, &ctx->mesh_lo[3 * mesh], &ctx->mesh_hi[3 * mesh],
                               const_cast<DevNode*>(sc.nodes), std::max(ctx->rebuild_slot[mesh], 0), const_cast<DevTri*>(sc.tris), tri_first, gm.tri_offset,
                               (gm.has_normal ? 1u : 0u) | (gm.has_uv ? 2u : 0u), &root, &used, &depth);
    if (st != GBL_OK) return st;
    if (used > n) return fail(ctx, GBL_ERR_INTERNAL, "gbl_rebuild_mesh: the tree outgrew the mesh's node records");
    const double build_ms = clock.lap_ms();
    gbl_launch_refit_tris(const_cast<DevTri*>(sc.tris), const_cast<DevTriBound*>(sc.tri_bounds), sc.tri_shade, sc.positions,
                          static_cast<uint32_t>(ctx->h_positions.size() / 3), tri_first, n, 0);
    HIP_TRY(ctx, hipGetLastError());
    drop_plan(ctx, mesh);     // the next edit makes its plan over the new tree ...
    ctx->h_nodes.clear();     // ... from a new download of the node array
    ctx->mesh_root[mesh] = root;
    ctx->mesh_stack_need[mesh] = 3 * depth;
    ctx->blas_depth = std::max(ctx->blas_depth, depth);
    ctx->info.blas_depth = ctx->blas_depth;   // (a bound from here on: the deepest tree any mesh of the context has had)
    if ((st = retlas_after_geometry_edit(ctx, "gbl_rebuild_mesh")) != GBL_OK) return st;
    if (probing())
        fprintf(stderr, "probe: gbl_rebuild_mesh mesh %u (%u triangles -> %u nodes, %d levels, slot %d): synchronise, indices and slot %.3f ms, build kernels "
                        "(one read-back per level) %.3f ms, triangle bounds and TLAS %.3f ms\n", mesh, n, used, depth, ctx->rebuild_slot[mesh], slot_ms, build_ms,
                clock.lap_ms());
    return GBL_OK;
}

gbl_status gbl_mesh_tree_stats_impl(gbl_ctx* ctx, uint32_t mesh, gbl_tree_stats* out) {
    if (!ctx) return GBL_ERR_INVALID;
    if (!out) return fail(ctx, GBL_ERR_INVALID, "gbl_mesh_tree_stats: out is NULL");
    gbl_status st = check_tree_mesh(ctx, mesh, "gbl_mesh_tree_stats");
    if (st != GBL_OK) return st;
    memset(out, 0, sizeof(*out));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipDeviceSynchronize());   // (an edit's launches are done: the boxes read are the ones the next render tests)
    if ((st = ensure_plan(ctx, mesh)) != GBL_OK) return st;
    const gbl_ctx::MeshRefit& mr = ctx->refit[mesh];
    const uint32_t records = mr.level_first.empty() ? 0u : mr.level_first.back();
    out->nodes = records;
    out->levels = mr.level_first.empty() ? 0u : static_cast<uint32_t>(mr.level_first.size() - 1);
    out->leaves = mr.leaves;
    if (records == 0) return GBL_OK;   // the root is a leaf
    const uint32_t blocks = (records + GBL_BLOCK - 1) / GBL_BLOCK;
    if ((st = grow(ctx, ctx->tree_stats, (3 + 2 * static_cast<uint64_t>(blocks)) * sizeof(double), "tree statistics")) != GBL_OK) return st;
    double* sums = static_cast<double*>(ctx->tree_stats.p);
    HIP_TRY(ctx, hipMemsetAsync(sums, 0, 3 * sizeof(double), 0));
    gbl_launch_tree_stats(ctx->scene.nodes, ctx->num_nodes, mr.plan, records, sums, sums + 3, 0);
    HIP_TRY(ctx, hipGetLastError());
    double h[3] = {0.0, 0.0, 0.0};
    HIP_TRY(ctx, hipMemcpy(h, sums, sizeof(h), hipMemcpyDeviceToHost));
    out->root_area = h[0];
    out->node_area = h[1];
    out->tri_area = h[2];
    return GBL_OK;
}

gbl_status gbl_get_vertices_impl(const gbl_ctx* cctx, uint32_t mesh, uint32_t first, uint32_t count, float* positions_out) {
    if (!cctx || !positions_out || mesh >= cctx->h_meshes.size()) return GBL_ERR_INVALID;
    gbl_ctx* ctx = const_cast<gbl_ctx*>(cctx);   // (the mirror is a cache of the device's positions: refreshing it changes nothing a caller can see)
    const gbl_mesh& gm = ctx->h_meshes[mesh];
    if (gm.shape != GBL_SHAPE_MESH || static_cast<uint64_t>(first) + count > gm.vertex_count) return GBL_ERR_INVALID;
    const gbl_status st = refresh_mirror(ctx, mesh);
    if (st != GBL_OK) return st;
    if (count > 0) memcpy(positions_out, ctx->h_positions.data() + 3 * (static_cast<size_t>(gm.vertex_offset) + first), 3 * static_cast<size_t>(count) * sizeof(float));
    return GBL_OK;
}

gbl_status gbl_get_vertices_device_impl(gbl_ctx* ctx, uint32_t mesh, uint32_t first, uint32_t count, float* d_positions_out) {
    if (!ctx) return GBL_ERR_INVALID;
    if (!d_positions_out) return fail(ctx, GBL_ERR_INVALID, "gbl_get_vertices_device: d_positions_out is NULL");
    if (mesh >= ctx->h_meshes.size()) return fail(ctx, GBL_ERR_INVALID, "gbl_get_vertices_device: mesh " + std::to_string(mesh) + " is out of range");
    const gbl_mesh& gm = ctx->h_meshes[mesh];
    if (gm.shape != GBL_SHAPE_MESH) return fail(ctx, GBL_ERR_INVALID, "gbl_get_vertices_device: mesh " + std::to_string(mesh) + " is a sphere or a disk: it has no vertices");
    if (static_cast<uint64_t>(first) + count > gm.vertex_count) return fail(ctx, GBL_ERR_INVALID, "gbl_get_vertices_device: vertex range out of bounds");
    const uint64_t bytes = 3 * static_cast<uint64_t>(count) * sizeof(float);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const gbl_status st = check_device_pointer(ctx, d_positions_out, bytes, "gbl_get_vertices_device", "d_positions_out");
    if (st != GBL_OK) return st;
    // the positions change only inside calls that synchronise, so the null stream's order is all the copy needs
    if (count > 0) {
        HIP_TRY(ctx, hipMemcpyAsync(d_positions_out, ctx->scene.positions + 3 * (static_cast<size_t>(gm.vertex_offset) + first), bytes, hipMemcpyDeviceToDevice, 0));
        HIP_TRY(ctx, hipStreamSynchronize(0));
    }
    return GBL_OK;
}

gbl_status gbl_order_pending_impl(const gbl_ctx* ctx, uint32_t mesh, uint32_t* pending) {
    if (!ctx || !pending || mesh >= ctx->h_meshes.size()) return GBL_ERR_INVALID;
    *pending = mesh < ctx->order_pending.size() && ctx->order_pending[mesh] ? 1u : 0u;
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
    if (table == 3) {   // a reader of the tie order
        const gbl_status st = make_orders_if(ctx, true);
        if (st != GBL_OK) return st;
    }
    HIP_TRY(ctx, hipMemcpy(out, static_cast<const unsigned char*>(base[table]) + first * size[table], count * size[table], hipMemcpyDeviceToHost));
    return GBL_OK;
}

}   // namespace

gbl_status make_pending_orders(gbl_ctx* ctx) {
    if (ctx->orders_pending == 0) return GBL_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipDeviceSynchronize());   // no launch in flight may be reading the table
    for (uint32_t mesh = 0; mesh < ctx->order_pending.size(); ++mesh) {
        if (!ctx->order_pending[mesh]) continue;
        gbl_status st = refresh_mirror(ctx, mesh);
        if (st == GBL_OK) st = make_order(ctx, mesh);
        if (st != GBL_OK) return st;
    }
    return GBL_OK;
}

extern "C" {

gbl_status gbl_update_vertices(gbl_ctx* ctx, uint32_t mesh, uint32_t first, uint32_t count, const float* positions, const float* normals) {
    return gbl_guard([&] { return gbl_update_vertices_impl(ctx, mesh, first, count, positions, normals); }, [&](const std::string& what) { if (ctx) ctx->error = what; });
}

gbl_status gbl_get_vertices(const gbl_ctx* ctx, uint32_t mesh, uint32_t first, uint32_t count, float* positions_out) {
    return gbl_guard([&] { return gbl_get_vertices_impl(ctx, mesh, first, count, positions_out); }, [&](const std::string&) {});
}

gbl_status gbl_update_vertices_device(gbl_ctx* ctx, uint32_t mesh, uint32_t first, uint32_t count, const float* d_positions, const float* d_normals, uint32_t flags) {
    return gbl_guard([&] { return gbl_update_vertices_device_impl(ctx, mesh, first, count, d_positions, d_normals, flags); },
                     [&](const std::string& what) { if (ctx) ctx->error = what; });
}

gbl_status gbl_get_vertices_device(gbl_ctx* ctx, uint32_t mesh, uint32_t first, uint32_t count, float* d_positions_out) {
    return gbl_guard([&] { return gbl_get_vertices_device_impl(ctx, mesh, first, count, d_positions_out); }, [&](const std::string& what) { if (ctx) ctx->error = what; });
}

gbl_status gbl_order_pending(const gbl_ctx* ctx, uint32_t mesh, uint32_t* pending) {
    return gbl_guard([&] { return gbl_order_pending_impl(ctx, mesh, pending); }, [&](const std::string&) {});
}

gbl_status gbl_rebuild_mesh(gbl_ctx* ctx, uint32_t mesh, uint32_t flags) {
    return gbl_guard([&] { return gbl_rebuild_mesh_impl(ctx, mesh, flags); }, [&](const std::string& what) { if (ctx) ctx->error = what; });
}

gbl_status gbl_mesh_tree_stats(gbl_ctx* ctx, uint32_t mesh, gbl_tree_stats* out) {
    return gbl_guard([&] { return gbl_mesh_tree_stats_impl(ctx, mesh, out); }, [&](const std::string& what) { if (ctx) ctx->error = what; });
}

gbl_status gbl_selftest_geometry(gbl_ctx* ctx, int table, uint64_t first, uint64_t count, void* out, uint64_t* total) {
    return gbl_guard([&] { return gbl_selftest_geometry_impl(ctx, table, first, count, out, total); }, [&](const std::string& what) { if (ctx) ctx->error = what; });
}

}   // extern "C"
