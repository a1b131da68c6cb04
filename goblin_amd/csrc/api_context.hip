// libgoblin_hip.so -- C ABI of the device integrator (include/goblin_hip.h): the context.
//
// gbl_create   packs the scene on the host (scene_prep.cpp) and uploads it once.
// There is no CPU fallback anywhere in this library: every entry point that
// computes something needs a HIP device and fails with GBL_ERR_DEVICE otherwise.
#include <dlfcn.h>
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

gbl_status fail(gbl_ctx* ctx, gbl_status st, std::string what) {
    ctx->error = std::move(what);
    return st;
}

gbl_status device_alloc(gbl_ctx* ctx, size_t bytes, const char* what, void** out) {
    const hipError_t e = hipMalloc(out, bytes);
    if (e != hipSuccess)
        return fail(ctx, e == hipErrorOutOfMemory ? GBL_ERR_OOM : GBL_ERR_DEVICE, std::string("hipMalloc(") + what + "): " + hipGetErrorString(e));
    ctx->allocations.push_back(*out);
    return GBL_OK;
}

// Grow a device buffer of the context to at least `bytes`; what it held is not kept
gbl_status grow(gbl_ctx* ctx, gbl_buf& b, uint64_t bytes, const char* what) {
    if (bytes <= b.bytes) return GBL_OK;
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.bytes = 0;
    const hipError_t e = hipMalloc(&b.p, bytes);
    if (e != hipSuccess) {
        b.p = nullptr;
        ctx->error = std::string("hipMalloc(") + what + "): " + hipGetErrorString(e);
        return GBL_ERR_OOM;
    }
    b.bytes = bytes;
    return GBL_OK;
}

gbl_status rebuild_tlas(gbl_ctx* ctx, std::vector<gbl_instance>& edited, const char* who) {
    const TlasInput in = {edited.data(),       static_cast<uint32_t>(edited.size()), ctx->h_meshes.data(),  ctx->h_materials.data(),
                          ctx->mesh_lo.data(), ctx->mesh_hi.data(),                  ctx->mesh_root.data(), ctx->tlas_base};
    TlasResult built;
    std::string err;
    gbl_status st = build_tlas(in, &built, &err);
    if (st != GBL_OK) {
        ctx->error = err;
        return st;
    }
    const std::vector<DevInstance>& inst = built.instances;
    const std::vector<DevNode>& tlas = built.nodes;
    const std::vector<DevInstanceBound>& bounds = built.instance_bounds;
    if (tlas.size() > ctx->tlas_capacity) {
        ctx->error = std::string(who) + ": rebuilt TLAS does not fit its reserved nodes";
        return GBL_ERR_DEVICE;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipDeviceSynchronize());   // no render may be reading the old TLAS
    DevScene& sc = ctx->scene;
    if (!inst.empty())
        HIP_TRY(ctx, hipMemcpy(const_cast<DevInstance*>(sc.instances), inst.data(), inst.size() * sizeof(DevInstance), hipMemcpyHostToDevice));
    if (!bounds.empty())
        HIP_TRY(ctx, hipMemcpy(const_cast<DevInstanceBound*>(sc.instance_bounds), bounds.data(), bounds.size() * sizeof(DevInstanceBound), hipMemcpyHostToDevice));
    if (!tlas.empty())
        HIP_TRY(ctx, hipMemcpy(const_cast<DevNode*>(sc.nodes) + ctx->tlas_base, tlas.data(), tlas.size() * sizeof(DevNode), hipMemcpyHostToDevice));
    sc.tlas_root = built.root;
    sc.stack_entries = scene_stack_entries(tlas, ctx->tlas_base, built.root, inst, ctx->mesh_stack_need);   // (the wavefront stack backing is re-checked at render time)
    ctx->info.tlas_depth = built.depth;
    ctx->info.tlas_nodes = tlas.size();
    ctx->h_instances.swap(edited);
    ctx->auto_rays_per_path.clear();   // the edited scene's paths may be longer or shorter: AUTO measures again
    return GBL_OK;
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
    if ((st = rebuild_tlas(ctx, edited, who)) != GBL_OK) return st;
    for (uint32_t i = 0; i < count;) {   // the raw table, run by run
        uint32_t end = i + 1;
        while (end < count && which[end] == which[end - 1] + 1) ++end;
        if ((st = write_instance_table(ctx, which[i], end - i)) != GBL_OK) return st;
        i = end;
    }
    return GBL_OK;
}

namespace {
thread_local std::string g_create_error;

// A scene array: hipMalloc `capacity` elements and copy the first `count` from the host
template <class T>
gbl_status upload_raw(gbl_ctx* ctx, const T* src, size_t count, size_t capacity, const T** out) {
    const size_t bytes = std::max<size_t>(1, capacity) * sizeof(T);
    void* p = nullptr;
    const gbl_status st = device_alloc(ctx, bytes, "scene", &p);
    if (st != GBL_OK) return st;
    ctx->info.scene_bytes += bytes;
    if (count) HIP_TRY(ctx, hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice));
    *out = static_cast<const T*>(p);
    return GBL_OK;
}

template <class T>
gbl_status upload(gbl_ctx* ctx, const std::vector<T>& v, const T** out) {
    return upload_raw(ctx, v.data(), v.size(), v.size(), out);
}
}   // namespace

extern "C" {

int gbl_abi_version(void) { return GBL_ABI_VERSION; }

const char* gbl_last_error(const gbl_ctx* ctx) { return ctx ? ctx->error.c_str() : g_create_error.c_str(); }

gbl_status gbl_create(const gbl_scene_desc* desc, int device, gbl_ctx** out) {
    const char* e = getenv("GBL_BVH_BUILD");
    return gbl_create_ex(desc, device, (e && !strcmp(e, "device")) ? GBL_CREATE_DEVICE_BVH : 0u, out);
}

static gbl_status gbl_create_ex_impl(const gbl_scene_desc* desc, int device, uint32_t flags, gbl_ctx** out) {
    const bool device_bvh = (flags & GBL_CREATE_DEVICE_BVH) != 0;
    if (!desc || !out) {
        g_create_error = "null argument";
        return GBL_ERR_INVALID;
    }
    *out = nullptr;
    PackedScene packed;
    std::string err;
    auto t_pack0 = std::chrono::steady_clock::now();
    gbl_status st = pack_scene(desc, &packed, &err, device_bvh);
    if (st != GBL_OK) {
        g_create_error = err;
        return st;
    }
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || device < 0 || device >= count) {
        g_create_error = "no HIP device " + std::to_string(device) + " (" +
                         (e != hipSuccess ? hipGetErrorString(e) : "device count " + std::to_string(count)) +
                         "); the device integrator has no CPU fallback";
        return GBL_ERR_DEVICE;
    }
    gbl_ctx* ctx = new gbl_ctx();
    ctx->device = device;
    memset(&ctx->scene, 0, sizeof(ctx->scene));
    memset(&ctx->info, 0, sizeof(ctx->info));
    auto bail = [&](gbl_status s) {
        g_create_error = ctx->error;
        gbl_destroy(ctx);
        return s;
    };
    if (hipSetDevice(device) != hipSuccess) {
        ctx->error = "hipSetDevice failed";
        return bail(GBL_ERR_DEVICE);
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) ctx->num_cus = prop.multiProcessorCount;
    DevScene& sc = ctx->scene;
    std::vector<float> ftab(packed.filter_table, packed.filter_table + 256);
    if (!device_bvh) {
        if ((st = upload(ctx, packed.nodes, &sc.nodes)) != GBL_OK) return bail(st);
        if ((st = upload(ctx, packed.tris, &sc.tris)) != GBL_OK) return bail(st);
        ctx->num_nodes = packed.nodes.size();
    } else {
        // nodes = [TLAS (from the host) | mesh 0 | mesh 1 | ...], tris = every mesh's triangles in Morton order
        size_t node_cap = packed.nodes.size(), tri_cap = 0;
        for (uint32_t m = 0; m < desc->num_meshes; ++m)
            if (desc->meshes[m].shape == GBL_SHAPE_MESH) {
                node_cap += desc->meshes[m].tri_count;
                tri_cap += desc->meshes[m].tri_count;
            }
        // device buffers are allocated at their final size; only the TLAS nodes and the raw geometry cross PCIe
        if ((st = upload_raw(ctx, packed.nodes.data(), packed.nodes.size(), node_cap, &sc.nodes)) != GBL_OK) return bail(st);
        ctx->num_nodes = node_cap;
        if ((st = upload_raw(ctx, static_cast<const DevTri*>(nullptr), 0, tri_cap, &sc.tris)) != GBL_OK) return bail(st);
        const float* d_pos = nullptr;
        const uint32_t* d_idx = nullptr;
        const size_t n_pos = 3 * static_cast<size_t>(desc->num_vertices), n_idx = 3 * static_cast<size_t>(desc->num_triangles);
        if ((st = upload_raw(ctx, desc->positions, n_pos, n_pos, &d_pos)) != GBL_OK) return bail(st);
        if ((st = upload_raw(ctx, desc->indices, n_idx, n_idx, &d_idx)) != GBL_OK) return bail(st);
        std::vector<int32_t> mesh_root(desc->num_meshes, 0);
        int32_t node_base = static_cast<int32_t>(packed.nodes.size());
        uint32_t tri_base = 0;
        int max_depth = 0;
        for (uint32_t m = 0; m < desc->num_meshes; ++m) {
            const gbl_mesh& gm = desc->meshes[m];
            if (gm.shape != GBL_SHAPE_MESH) continue;
            uint32_t used = 0;
            int depth = 0;
            st = gbl_build_blas_device(ctx, d_pos + 3 * static_cast<size_t>(gm.vertex_offset), d_idx + 3 * static_cast<size_t>(gm.tri_offset), gm.tri_count,
                                   &packed.mesh_lo[3 * m], &packed.mesh_hi[3 * m], const_cast<DevNode*>(sc.nodes), node_base,
                                   const_cast<DevTri*>(sc.tris), tri_base, gm.tri_offset, (gm.has_normal ? 1u : 0u) | (gm.has_uv ? 2u : 0u), &mesh_root[m], &used, &depth);
            if (st != GBL_OK) return bail(st);
            node_base += static_cast<int32_t>(used);
            tri_base += gm.tri_count;
            max_depth = std::max(max_depth, depth);
            packed.mesh_stack_need[m] = 3 * depth;
        }
        for (size_t i = 0; i < packed.instances.size(); ++i)
            if (packed.instances[i].shape == 0u) packed.instances[i].root = mesh_root[packed.instances[i].mesh];
        for (uint32_t m = 0; m < desc->num_meshes; ++m)
            if (desc->meshes[m].shape == GBL_SHAPE_MESH) packed.mesh_root[m] = mesh_root[m];
        packed.blas_max_depth = max_depth;
        packed.blas_nodes = static_cast<uint64_t>(node_base) - packed.nodes.size();
        if (ctx->lbvh_scratch.p) (void)hipFree(ctx->lbvh_scratch.p);   // a context that never rebuilds a mesh holds no builder scratch
        ctx->lbvh_scratch = gbl_buf();
        {   // device-built trees: the per-level bound of each mesh's BLAS under the exact TLAS sum
            const std::vector<DevNode> tl(packed.nodes.begin() + packed.tlas_base, packed.nodes.begin() + packed.tlas_base + static_cast<std::ptrdiff_t>(packed.tlas_nodes));
            packed.stack_entries = scene_stack_entries(tl, packed.tlas_base, packed.tlas_root, packed.instances, packed.mesh_stack_need);
        }
        packed.tris.resize(tri_cap);   // for gbl_info only
    }
    ctx->build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_pack0).count();
    if ((st = upload(ctx, packed.tri_shade, &sc.tri_shade)) != GBL_OK) return bail(st);
    if (!device_bvh) {
        if ((st = upload(ctx, packed.tri_bounds_leaf, &sc.tri_bounds)) != GBL_OK) return bail(st);
    } else {
        const DevTriBound* by_id = nullptr;
        if ((st = upload(ctx, packed.tri_bounds, &by_id)) != GBL_OK) return bail(st);
        if ((st = upload_raw(ctx, static_cast<const DevTriBound*>(nullptr), 0, packed.tris.size(), &sc.tri_bounds)) != GBL_OK) return bail(st);
        gbl_launch_tri_bounds_gather(sc.tris, by_id, const_cast<DevTriBound*>(sc.tri_bounds), static_cast<uint32_t>(packed.tris.size()));
        if (hipError_t le = hipGetLastError(); le != hipSuccess) {
            ctx->error = std::string("triangle bound gather: ") + hipGetErrorString(le);
            return bail(GBL_ERR_DEVICE);
        }
    }
    if ((st = upload(ctx, packed.tri_order, &sc.tri_order)) != GBL_OK) return bail(st);
    if ((st = upload(ctx, packed.instance_bounds, &sc.instance_bounds)) != GBL_OK) return bail(st);
    if ((st = upload(ctx, packed.positions, &sc.positions)) != GBL_OK) return bail(st);
    if ((st = upload(ctx, packed.normals, &sc.normals)) != GBL_OK) return bail(st);
    if ((st = upload(ctx, packed.uvs, &sc.uvs)) != GBL_OK) return bail(st);
    if ((st = upload(ctx, packed.instances, &sc.instances)) != GBL_OK) return bail(st);
    if ((st = upload(ctx, packed.materials, &sc.materials)) != GBL_OK) return bail(st);
    if ((st = upload(ctx, packed.textures, &sc.textures)) != GBL_OK) return bail(st);
    if ((st = upload(ctx, packed.lights, &sc.lights)) != GBL_OK) return bail(st);
    if ((st = upload(ctx, packed.light_tris, &sc.light_tris)) != GBL_OK) return bail(st);
    if ((st = upload(ctx, packed.light_cdf, &sc.light_cdf)) != GBL_OK) return bail(st);
    if ((st = upload(ctx, packed.light_pick_pdf, &sc.light_pick_pdf)) != GBL_OK) return bail(st);
    if ((st = upload(ctx, ftab, &sc.filter_table)) != GBL_OK) return bail(st);
    if ((st = upload(ctx, packed.images, &sc.images)) != GBL_OK) return bail(st);
    if ((st = upload_raw(ctx, desc->texels, desc->num_texels, desc->num_texels, &sc.texels)) != GBL_OK) return bail(st);
    if ((st = upload(ctx, packed.ewa_lut, &sc.ewa_lut)) != GBL_OK) return bail(st);
    if ((st = upload(ctx, packed.ibl_dist, &sc.ibl_dist)) != GBL_OK) return bail(st);
    if ((st = upload(ctx, packed.vol_density, &sc.vol_density)) != GBL_OK) return bail(st);
    sc.has_ibl = packed.has_ibl;
    sc.hot_nodes = packed.hot_nodes;
    ctx->has_images = desc->num_images > 0;
    sc.tlas_root = packed.tlas_root;
    sc.num_instances = static_cast<int32_t>(packed.instances.size());
    sc.num_lights = static_cast<int32_t>(packed.lights.size());
    for (const DevLight& l : packed.lights) ctx->h_light_slots.push_back(l.wh_n);
    // what gbl_update_lights needs (api_lights.hip)
    ctx->h_lights.assign(desc->lights, desc->lights + desc->num_lights);
    ctx->h_dev_lights = packed.lights;
    ctx->h_light_power = packed.light_power;
    ctx->h_light_cdf = packed.light_cdf;
    ctx->h_light_pick_pdf = packed.light_pick_pdf;
    memcpy(ctx->bound_lo, packed.bound_lo, sizeof(ctx->bound_lo));
    memcpy(ctx->bound_hi, packed.bound_hi, sizeof(ctx->bound_hi));
    ctx->light_instances.assign(desc->num_lights, std::vector<uint32_t>());
    for (uint32_t i = 0; i < desc->num_instances; ++i)
        if (desc->instances[i].area_light >= 0) ctx->light_instances[desc->instances[i].area_light].push_back(i);
    sc.stack_entries = packed.stack_entries;
    sc.extended = packed.extended;
    sc.has_masks = packed.has_masks;
    sc.has_bssrdf = packed.has_bssrdf;
    sc.wh_slots = packed.wh_slots;
    sc.volume = packed.volume;
    sc.camera = packed.camera;
    sc.film = packed.film;
    ctx->h_camera = desc->camera;
    ctx->h_film = desc->film;
    ctx->scene_extended = packed.scene_extended;
    if ((st = device_alloc(ctx, sizeof(uint32_t), "work counter", reinterpret_cast<void**>(&ctx->work_counter))) != GBL_OK) return bail(st);
    if ((st = device_alloc(ctx, 32 * sizeof(unsigned long long), "stats", reinterpret_cast<void**>(&ctx->stats))) != GBL_OK) return bail(st);
    if (hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->ev1) != hipSuccess) {
        ctx->error = "hipEventCreate failed";
        return bail(GBL_ERR_DEVICE);
    }
    ctx->info.xres = packed.film.xres;
    ctx->info.yres = packed.film.yres;
    memcpy(ctx->info.window, packed.film.window, sizeof(ctx->info.window));
    ctx->info.blas_nodes = packed.blas_nodes;
    ctx->info.tlas_nodes = packed.tlas_nodes;
    ctx->info.triangles = packed.tris.size();
    ctx->info.instances = packed.instances.size();
    ctx->h_instances.assign(desc->instances, desc->instances + desc->num_instances);
    ctx->h_meshes.assign(desc->meshes, desc->meshes + desc->num_meshes);
    ctx->h_materials.assign(desc->materials, desc->materials + desc->num_materials);
    ctx->mesh_lo = packed.mesh_lo;
    ctx->mesh_hi = packed.mesh_hi;
    ctx->mesh_root = packed.mesh_root;
    ctx->tlas_base = packed.tlas_base;
    ctx->tlas_capacity = packed.tlas_capacity;
    ctx->blas_depth = packed.blas_max_depth;
    ctx->mesh_stack_need = packed.mesh_stack_need;
    // what gbl_update_vertices needs (api_geometry.hip)
    ctx->h_positions.assign(desc->positions, desc->positions + 3 * static_cast<size_t>(desc->num_vertices));
    ctx->h_indices.assign(desc->indices, desc->indices + 3 * static_cast<size_t>(desc->num_triangles));
    ctx->mesh_tri_first.assign(desc->num_meshes, 0u);
    ctx->mesh_emits.assign(desc->num_meshes, 0);
    for (uint32_t m = 0, tri_first = 0; m < desc->num_meshes; ++m)
        if (desc->meshes[m].shape == GBL_SHAPE_MESH) {
            ctx->mesh_tri_first[m] = tri_first;
            tri_first += desc->meshes[m].tri_count;
        }
    for (uint32_t i = 0; i < desc->num_instances; ++i)
        if (desc->instances[i].area_light >= 0) ctx->mesh_emits[desc->instances[i].mesh] = 1;
    for (uint32_t i = 0; i < desc->num_lights; ++i)
        if (desc->lights[i].type == GBL_LIGHT_AREA && desc->lights[i].mesh < desc->num_meshes) ctx->mesh_emits[desc->lights[i].mesh] = 1;
    ctx->refit.assign(desc->num_meshes, gbl_ctx::MeshRefit());
    ctx->rebuild_slot.assign(desc->num_meshes, -1);
    ctx->rebuild_idx.assign(desc->num_meshes, nullptr);
    if (getenv("GBL_PROBE"))
        fprintf(stderr, "probe: traversal stack entries %d (per-level bound %d: TLAS depth %d, BLAS depth %d)\n", packed.stack_entries,
                3 * (packed.tlas_depth + packed.blas_max_depth) + 2, packed.tlas_depth, packed.blas_max_depth);
    for (uint32_t i = 0; i < desc->num_lights; ++i)
        if (desc->lights[i].type == GBL_LIGHT_DIRECTIONAL || desc->lights[i].type == GBL_LIGHT_IBL) ctx->has_directional = true;   // lights sized by the scene bound
    ctx->info.build_ms = ctx->build_ms;
    ctx->info.blas_depth = packed.blas_max_depth;
    ctx->info.tlas_depth = packed.tlas_depth;
    ctx->info.instanced_triangles = 0;
    for (uint32_t i = 0; i < desc->num_instances; ++i) ctx->info.instanced_triangles += desc->meshes[desc->instances[i].mesh].tri_count;
    *out = ctx;
    return GBL_OK;
}
gbl_status gbl_create_ex(const gbl_scene_desc* desc, int device, uint32_t flags, gbl_ctx** out) {
    return gbl_guard([&] { return gbl_create_ex_impl(desc, device, flags, out); }, [&](const std::string& what) { g_create_error = what; });
}

static gbl_status gbl_update_instances_impl(gbl_ctx* ctx, uint32_t first, uint32_t count, const gbl_trs* to_world) {
    if (!ctx) return GBL_ERR_INVALID;
    if (!to_world || static_cast<uint64_t>(first) + count > ctx->h_instances.size()) {
        ctx->error = "gbl_update_instances: instance range out of bounds";
        return GBL_ERR_INVALID;
    }
    gbl_status st = refuse_scene_bound_edit(ctx, "gbl_update_instances");
    if (st != GBL_OK) return st;
    for (uint32_t i = 0; i < count; ++i)
        if (ctx->h_instances[first + i].area_light >= 0) {
            ctx->error = "gbl_update_instances: instance " + std::to_string(first + i) + " carries an area light, whose own transform would "
                         "have to move with it; re-create the context instead";
            return GBL_ERR_UNSUPPORTED;
        }
    std::vector<uint32_t> which(count);
    for (uint32_t i = 0; i < count; ++i) which[i] = first + i;
    return move_instances(ctx, which.data(), count, to_world, "gbl_update_instances");
}
gbl_status gbl_update_instances(gbl_ctx* ctx, uint32_t first, uint32_t count, const gbl_trs* to_world) {
    return gbl_guard([&] { return gbl_update_instances_impl(ctx, first, count, to_world); }, [&](const std::string& what) { if (ctx) ctx->error = what; });
}

// Host only: the camera travels to every kernel by value inside DevScene, so nothing on the device changes here and work
// already queued keeps the camera it was launched with.
static gbl_status gbl_update_camera_impl(gbl_ctx* ctx, const gbl_camera* camera) {
    if (!ctx) return GBL_ERR_INVALID;
    if (!camera) return fail(ctx, GBL_ERR_INVALID, "gbl_update_camera: camera is NULL");
    if (camera->type > GBL_CAMERA_ORTHOGRAPHIC) return fail(ctx, GBL_ERR_INVALID, "gbl_update_camera: type: unknown camera type");
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(camera->position[k])) return fail(ctx, GBL_ERR_INVALID, "gbl_update_camera: position is not finite");
    for (int k = 0; k < 4; ++k)
        if (!std::isfinite(camera->orientation[k])) return fail(ctx, GBL_ERR_INVALID, "gbl_update_camera: orientation is not finite");
    if (!std::isfinite(camera->fov_degrees)) return fail(ctx, GBL_ERR_INVALID, "gbl_update_camera: fov_degrees is not finite");
    pack_camera(*camera, ctx->h_film, &ctx->scene.camera);
    ctx->scene.extended = (ctx->scene_extended || camera_extended(*camera)) ? 1 : 0;
    ctx->h_camera = *camera;
    ctx->auto_rays_per_path.clear();   // the pilot's rays per path belong to the old view: AUTO measures again
    return GBL_OK;
}
gbl_status gbl_update_camera(gbl_ctx* ctx, const gbl_camera* camera) {
    return gbl_guard([&] { return gbl_update_camera_impl(ctx, camera); }, [&](const std::string& what) { if (ctx) ctx->error = what; });
}

gbl_status gbl_get_camera(const gbl_ctx* ctx, gbl_camera* out) {
    if (!ctx || !out) return GBL_ERR_INVALID;
    *out = ctx->h_camera;
    return GBL_OK;
}

void gbl_destroy(gbl_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    for (void* p : ctx->allocations) (void)hipFree(p);
    for (gbl_buf* b : {&ctx->li, &ctx->prim_hits, &ctx->prim_items, &ctx->vol, &ctx->sss, &ctx->aov, &ctx->stream_scratch, &ctx->stream_xy, &ctx->wf_spill,
                       &ctx->dev_rgb1, &ctx->dev_rgb, &ctx->dev_logs, &ctx->dev_filter, &ctx->denoise, &ctx->temporal, &ctx->motion, &ctx->motion_deform, &ctx->vertex_words, &ctx->pose_words,
                       &ctx->lbvh_scratch, &ctx->tree_stats, &ctx->inst_stage, &ctx->query_spill})
        if (b->p) (void)hipFree(b->p);
    if (ctx->stream_seeds) (void)hipFree(ctx->stream_seeds);
    if (ctx->wf_ev_shade) (void)hipEventDestroy(ctx->wf_ev_shade);
    if (ctx->wf_ev_shadow) (void)hipEventDestroy(ctx->wf_ev_shadow);
    if (ctx->wf_aux) (void)hipStreamDestroy(ctx->wf_aux);
    if (ctx->wf_host_flags) (void)hipHostFree(ctx->wf_host_flags);
    for (hipEvent_t ev : ctx->light_ev)
        if (ev) (void)hipEventDestroy(ev);   // (hipHostFree below waits for whatever upload still reads the staging)
    if (ctx->light_stage) (void)hipHostFree(ctx->light_stage);
    for (int i = 0; i < gbl_ctx::kTimingRing; ++i)
        for (int k = 0; k < 3; ++k)
            if (ctx->t_ev[i][k]) (void)hipEventDestroy(ctx->t_ev[i][k]);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    if (ctx->rccl) dlclose(ctx->rccl);
    delete ctx;
}

gbl_status gbl_get_info(const gbl_ctx* ctx, gbl_info* out) {
    if (!ctx || !out) return GBL_ERR_INVALID;
    *out = ctx->info;
    return GBL_OK;
}

}   // extern "C"
