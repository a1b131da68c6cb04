// libgoblin_hip.so -- C ABI of the device integrator (include/goblin_hip.h): the context.  gbl_create packs the scene on the
// host (scene_prep.cpp) and uploads it once, step by step below; gbl_destroy, gbl_get_info, the camera edit, the error text and
// the allocation helpers of gbl_host.h go with it.  There is no CPU fallback anywhere in this library: every entry point that
// computes something needs a HIP device and fails with GBL_ERR_DEVICE otherwise.
#include <dlfcn.h>
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

void device_free(gbl_ctx* ctx, void* p) {
    if (!p) return;
    ctx->allocations.erase(std::remove(ctx->allocations.begin(), ctx->allocations.end(), p), ctx->allocations.end());
    (void)hipFree(p);
}

// Grow a device buffer of the context to at least `bytes`; what it held is not kept
gbl_status grow(gbl_ctx* ctx, gbl_buf& b, uint64_t bytes, const char* what) {
    if (bytes <= b.bytes) return GBL_OK;
    if (b.p) (void)hipFree(b.p);
    b = gbl_buf();
    const hipError_t e = hipMalloc(&b.p, bytes);
    if (e != hipSuccess) {
        b.p = nullptr;
        return fail(ctx, GBL_ERR_OOM, std::string("hipMalloc(") + what + "): " + hipGetErrorString(e));
    }
    b.bytes = bytes;
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

// The steps of gbl_create, in its order.  The context on its device: a failure that leaves no *out has set gbl_last_error(NULL)'s text
gbl_status open_device(int device, gbl_ctx** out) {
    int count = 0;
    const hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || device < 0 || device >= count) {
        g_create_error = "no HIP device " + std::to_string(device) + " (" + (e != hipSuccess ? hipGetErrorString(e) : "device count " + std::to_string(count)) +
                         "); the device integrator has no CPU fallback";
        return GBL_ERR_DEVICE;
    }
    gbl_ctx* ctx = *out = new gbl_ctx();
    ctx->device = device;
    memset(&ctx->scene, 0, sizeof(ctx->scene));
    memset(&ctx->info, 0, sizeof(ctx->info));
    if (hipSetDevice(device) != hipSuccess) return fail(ctx, GBL_ERR_DEVICE, "hipSetDevice failed");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) ctx->num_cus = prop.multiProcessorCount;
    return GBL_OK;
}

// The trees pack_scene built: nodes and triangles (where build_ms stops), then the triangles' bounds in leaf order
gbl_status upload_host_built_geometry(gbl_ctx* ctx, const PackedScene& packed, LapClock& since_pack) {
    DevScene& sc = ctx->scene;
    gbl_status st = upload(ctx, packed.nodes, &sc.nodes);
    if (st == GBL_OK) st = upload(ctx, packed.tris, &sc.tris);
    if (st != GBL_OK) return st;
    ctx->num_nodes = packed.nodes.size();
    ctx->build_ms = since_pack.lap_ms();
    return upload(ctx, packed.tri_bounds_leaf, &sc.tri_bounds);
}

// GBL_CREATE_DEVICE_BVH: nodes = [TLAS (from the host) | mesh 0 | mesh 1 | ...], tris = every mesh's triangles in Morton order,
// allocated at their final size: only the TLAS nodes and the raw geometry cross PCIe.  `packed` takes what the device found
gbl_status build_geometry_on_device(gbl_ctx* ctx, const gbl_scene_desc* desc, PackedScene& packed, LapClock& since_pack) {
    DevScene& sc = ctx->scene;
    size_t node_cap = packed.nodes.size(), tri_cap = 0;
    for (uint32_t m = 0; m < desc->num_meshes; ++m)
        if (desc->meshes[m].shape == GBL_SHAPE_MESH) {
            node_cap += desc->meshes[m].tri_count;
            tri_cap += desc->meshes[m].tri_count;
        }
    gbl_status st = upload_raw(ctx, packed.nodes.data(), packed.nodes.size(), node_cap, &sc.nodes);
    if (st != GBL_OK) return st;
    ctx->num_nodes = node_cap;
    if ((st = upload_raw(ctx, static_cast<const DevTri*>(nullptr), 0, tri_cap, &sc.tris)) != GBL_OK) return st;
    const float* d_pos = nullptr;
    const uint32_t* d_idx = nullptr;
    const size_t n_pos = 3 * static_cast<size_t>(desc->num_vertices), n_idx = 3 * static_cast<size_t>(desc->num_triangles);
    if ((st = upload_raw(ctx, desc->positions, n_pos, n_pos, &d_pos)) != GBL_OK) return st;
    if ((st = upload_raw(ctx, desc->indices, n_idx, n_idx, &d_idx)) != GBL_OK) return st;
    int32_t node_base = static_cast<int32_t>(packed.nodes.size());
    uint32_t tri_base = 0;
    for (uint32_t m = 0; m < desc->num_meshes; ++m) {   // (pack_scene left every triangle mesh's root and blas_max_depth 0 for this loop)
        const gbl_mesh& gm = desc->meshes[m];
        if (gm.shape != GBL_SHAPE_MESH) continue;
        uint32_t used = 0;
        int depth = 0;
        st = gbl_build_blas_device(ctx, d_pos + 3 * static_cast<size_t>(gm.vertex_offset), d_idx + 3 * static_cast<size_t>(gm.tri_offset), gm.tri_count,
                                   &packed.mesh_lo[3 * m], &packed.mesh_hi[3 * m], const_cast<DevNode*>(sc.nodes), node_base,
                                   const_cast<DevTri*>(sc.tris), tri_base, gm.tri_offset, (gm.has_normal ? 1u : 0u) | (gm.has_uv ? 2u : 0u), &packed.mesh_root[m], &used, &depth);
        if (st != GBL_OK) return st;
        node_base += static_cast<int32_t>(used);
        tri_base += gm.tri_count;
        packed.blas_max_depth = std::max(packed.blas_max_depth, depth);
        packed.mesh_stack_need[m] = 3 * depth;
    }
    for (DevInstance& inst : packed.instances)
        if (inst.shape == 0u) inst.root = packed.mesh_root[inst.mesh];
    packed.blas_nodes = static_cast<uint64_t>(node_base) - packed.nodes.size();
    if (ctx->lbvh_scratch.p) (void)hipFree(ctx->lbvh_scratch.p);   // a context that never rebuilds a mesh holds no builder scratch
    ctx->lbvh_scratch = gbl_buf();
    // device-built trees: the per-level bound of each mesh's BLAS under the exact TLAS sum
    const std::vector<DevNode> tl(packed.nodes.begin() + packed.tlas_base, packed.nodes.begin() + packed.tlas_base + static_cast<std::ptrdiff_t>(packed.tlas_nodes));
    packed.stack_entries = scene_stack_entries(tl, packed.tlas_base, packed.tlas_root, packed.instances, packed.mesh_stack_need);
    packed.tris.resize(tri_cap);   // for gbl_info only
    ctx->build_ms = since_pack.lap_ms();   // (the bounds are not in it: by id from the host, gathered into the triangles' order)
    const DevTriBound* by_id = nullptr;
    if ((st = upload(ctx, packed.tri_bounds, &by_id)) != GBL_OK) return st;
    if ((st = upload_raw(ctx, static_cast<const DevTriBound*>(nullptr), 0, tri_cap, &sc.tri_bounds)) != GBL_OK) return st;
    gbl_launch_tri_bounds_gather(sc.tris, by_id, const_cast<DevTriBound*>(sc.tri_bounds), static_cast<uint32_t>(tri_cap));
    if (const hipError_t le = hipGetLastError(); le != hipSuccess) return fail(ctx, GBL_ERR_DEVICE, std::string("triangle bound gather: ") + hipGetErrorString(le));
    return GBL_OK;
}

// Every DevScene array but the geometry's
gbl_status upload_tables(gbl_ctx* ctx, const gbl_scene_desc* desc, const PackedScene& packed) {
    DevScene& sc = ctx->scene;
    const std::vector<float> ftab(packed.filter_table, packed.filter_table + 256);
    gbl_status st;
    if ((st = upload(ctx, packed.tri_shade, &sc.tri_shade)) != GBL_OK) return st;
    if ((st = upload(ctx, packed.tri_order, &sc.tri_order)) != GBL_OK) return st;
    if ((st = upload(ctx, packed.instance_bounds, &sc.instance_bounds)) != GBL_OK) return st;
    if ((st = upload(ctx, packed.positions, &sc.positions)) != GBL_OK) return st;
    if ((st = upload(ctx, packed.normals, &sc.normals)) != GBL_OK) return st;
    if ((st = upload(ctx, packed.uvs, &sc.uvs)) != GBL_OK) return st;
    if ((st = upload(ctx, packed.instances, &sc.instances)) != GBL_OK) return st;
    if ((st = upload(ctx, packed.materials, &sc.materials)) != GBL_OK) return st;
    if ((st = upload(ctx, packed.textures, &sc.textures)) != GBL_OK) return st;
    if ((st = upload(ctx, packed.lights, &sc.lights)) != GBL_OK) return st;
    if ((st = upload(ctx, packed.light_tris, &sc.light_tris)) != GBL_OK) return st;
    if ((st = upload(ctx, packed.light_cdf, &sc.light_cdf)) != GBL_OK) return st;
    if ((st = upload(ctx, packed.light_pick_pdf, &sc.light_pick_pdf)) != GBL_OK) return st;
    if ((st = upload(ctx, ftab, &sc.filter_table)) != GBL_OK) return st;
    if ((st = upload(ctx, packed.images, &sc.images)) != GBL_OK) return st;
    if ((st = upload_raw(ctx, desc->texels, desc->num_texels, desc->num_texels, &sc.texels)) != GBL_OK) return st;
    if ((st = upload(ctx, packed.ewa_lut, &sc.ewa_lut)) != GBL_OK) return st;
    if ((st = upload(ctx, packed.ibl_dist, &sc.ibl_dist)) != GBL_OK) return st;
    return upload(ctx, packed.vol_density, &sc.vol_density);
}

// DevScene's scalar fields
void set_scene_header(DevScene& sc, const PackedScene& packed) {
    sc.has_ibl = packed.has_ibl;
    sc.hot_nodes = packed.hot_nodes;
    sc.tlas_root = packed.tlas_root;
    sc.num_instances = static_cast<int32_t>(packed.instances.size());
    sc.num_lights = static_cast<int32_t>(packed.lights.size());
    sc.stack_entries = packed.stack_entries;
    sc.extended = packed.extended;
    sc.has_masks = packed.has_masks;
    sc.has_bssrdf = packed.has_bssrdf;
    sc.wh_slots = packed.wh_slots;
    sc.volume = packed.volume;
    sc.camera = packed.camera;
    sc.film = packed.film;
}

// The host copies the edit entry points work from, grouped as gbl_ctx declares them (gbl_internal.h)
void keep_for_edits(gbl_ctx* ctx, const gbl_scene_desc* desc, const PackedScene& packed) {
    // camera and film: gbl_update_camera, gbl_film_accumulate
    ctx->h_camera = desc->camera, ctx->h_film = desc->film, ctx->h_setting = desc->setting;
    ctx->scene_extended = packed.scene_extended;
    // instances and TLAS: gbl_update_instances and every edit that ends in its tail (api_instances.hip)
    ctx->h_instances.assign(desc->instances, desc->instances + desc->num_instances);
    for (const DevLight& l : packed.lights) ctx->h_light_slots.push_back(l.wh_n);
    ctx->h_meshes.assign(desc->meshes, desc->meshes + desc->num_meshes);
    ctx->h_materials.assign(desc->materials, desc->materials + desc->num_materials);
    ctx->mesh_lo = packed.mesh_lo, ctx->mesh_hi = packed.mesh_hi;
    ctx->mesh_root = packed.mesh_root;
    ctx->tlas_base = packed.tlas_base, ctx->tlas_capacity = packed.tlas_capacity;
    ctx->blas_depth = packed.blas_max_depth;
    ctx->mesh_stack_need = packed.mesh_stack_need;
    for (uint32_t i = 0; i < desc->num_lights; ++i)
        if (desc->lights[i].type == GBL_LIGHT_DIRECTIONAL || desc->lights[i].type == GBL_LIGHT_IBL) ctx->has_directional = true;   // lights sized by the scene bound
    // vertices and refit: gbl_update_vertices, gbl_rebuild_mesh (api_geometry.hip)
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
    // lights: gbl_update_lights (api_lights.hip)
    ctx->h_lights.assign(desc->lights, desc->lights + desc->num_lights);
    ctx->h_dev_lights = packed.lights;
    ctx->h_light_power = packed.light_power;
    ctx->h_light_cdf = packed.light_cdf, ctx->h_light_pick_pdf = packed.light_pick_pdf;
    memcpy(ctx->bound_lo, packed.bound_lo, sizeof(ctx->bound_lo));
    memcpy(ctx->bound_hi, packed.bound_hi, sizeof(ctx->bound_hi));
    ctx->light_instances.assign(desc->num_lights, std::vector<uint32_t>());
    for (uint32_t i = 0; i < desc->num_instances; ++i)
        if (desc->instances[i].area_light >= 0) ctx->light_instances[desc->instances[i].area_light].push_back(i);
    // materials and textures: gbl_update_materials*, gbl_update_textures* (api_materials.hip; h_materials is kept above)
    ctx->h_textures.assign(desc->textures, desc->textures + desc->num_textures);
    ctx->mat_records = packed.materials;
    ctx->tex_records = packed.textures;
    // images: gbl_update_image* (api_images.hip)
    ctx->h_images.assign(desc->images, desc->images + desc->num_images);
    ctx->image_taps.assign(desc->num_images, gbl_ctx::ImageTaps());
    ctx->environment.assign(desc->num_lights, gbl_ctx::Environment());
}

// gbl_info but scene_bytes, which the uploads have summed
void fill_info(gbl_ctx* ctx, const gbl_scene_desc* desc, const PackedScene& packed) {
    gbl_info& info = ctx->info;
    info.xres = packed.film.xres, info.yres = packed.film.yres;
    memcpy(info.window, packed.film.window, sizeof(info.window));
    info.blas_nodes = packed.blas_nodes;
    info.tlas_nodes = packed.tlas_nodes;
    info.triangles = packed.tris.size();
    info.instances = packed.instances.size();
    info.build_ms = ctx->build_ms;
    info.blas_depth = packed.blas_max_depth;
    info.tlas_depth = packed.tlas_depth;
    for (uint32_t i = 0; i < desc->num_instances; ++i) info.instanced_triangles += desc->meshes[desc->instances[i].mesh].tri_count;
}

gbl_status gbl_create_ex_impl(const gbl_scene_desc* desc, int device, uint32_t flags, gbl_ctx** out) {
    const bool device_bvh = (flags & GBL_CREATE_DEVICE_BVH) != 0;
    if (!desc || !out) {
        g_create_error = "null argument";
        return GBL_ERR_INVALID;
    }
    *out = nullptr;
    PackedScene packed;
    std::string err;
    LapClock since_pack;   // build_ms: pack_scene, BVH construction, node / triangle upload
    gbl_status st = pack_scene(desc, &packed, &err, device_bvh);
    if (st != GBL_OK) {
        g_create_error = err;
        return st;
    }
    gbl_ctx* ctx = nullptr;
    auto bail = [&](gbl_status s) {
        if (ctx) g_create_error = ctx->error;
        gbl_destroy(ctx);
        return s;
    };
    if ((st = open_device(device, &ctx)) != GBL_OK) return bail(st);
    st = device_bvh ? build_geometry_on_device(ctx, desc, packed, since_pack) : upload_host_built_geometry(ctx, packed, since_pack);
    if (st != GBL_OK) return bail(st);
    if ((st = upload_tables(ctx, desc, packed)) != GBL_OK) return bail(st);
    set_scene_header(ctx->scene, packed);
    ctx->has_images = desc->num_images > 0;
    keep_for_edits(ctx, desc, packed);
    if ((st = device_alloc(ctx, sizeof(uint32_t), "work counter", reinterpret_cast<void**>(&ctx->work_counter))) != GBL_OK) return bail(st);
    if ((st = device_alloc(ctx, 32 * sizeof(unsigned long long), "stats", reinterpret_cast<void**>(&ctx->stats))) != GBL_OK) return bail(st);
    if (hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->ev1) != hipSuccess) return bail(fail(ctx, GBL_ERR_DEVICE, "hipEventCreate failed"));
    fill_info(ctx, desc, packed);
    if (probing())
        fprintf(stderr, "probe: traversal stack entries %d (per-level bound %d: TLAS depth %d, BLAS depth %d)\n", packed.stack_entries,
                3 * (packed.tlas_depth + packed.blas_max_depth) + 2, packed.tlas_depth, packed.blas_max_depth);
    *out = ctx;
    return GBL_OK;
}

// Host only: the camera travels to every kernel by value inside DevScene, so nothing on the device changes here and work
// already queued keeps the camera it was launched with.
gbl_status gbl_update_camera_impl(gbl_ctx* ctx, const gbl_camera* camera) {
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
}   // namespace

extern "C" {

int gbl_abi_version(void) { return GBL_ABI_VERSION; }

const char* gbl_last_error(const gbl_ctx* ctx) { return ctx ? ctx->error.c_str() : g_create_error.c_str(); }

gbl_status gbl_create(const gbl_scene_desc* desc, int device, gbl_ctx** out) {
    const char* e = getenv("GBL_BVH_BUILD");
    return gbl_create_ex(desc, device, (e && !strcmp(e, "device")) ? GBL_CREATE_DEVICE_BVH : 0u, out);
}

gbl_status gbl_create_ex(const gbl_scene_desc* desc, int device, uint32_t flags, gbl_ctx** out) {
    return gbl_guard([&] { return gbl_create_ex_impl(desc, device, flags, out); }, [&](const std::string& what) { g_create_error = what; });
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
                       &ctx->lbvh_scratch, &ctx->tree_stats, &ctx->inst_stage, &ctx->query_spill, &ctx->query_any})
        if (b->p) (void)hipFree(b->p);
    if (ctx->stream_seeds) (void)hipFree(ctx->stream_seeds);
    if (ctx->wf_ev_shade) (void)hipEventDestroy(ctx->wf_ev_shade);
    if (ctx->wf_ev_shadow) (void)hipEventDestroy(ctx->wf_ev_shadow);
    if (ctx->wf_aux) (void)hipStreamDestroy(ctx->wf_aux);
    if (ctx->wf_host_flags) (void)hipHostFree(ctx->wf_host_flags);
    for (hipEvent_t ev : ctx->light_ev)
        if (ev) (void)hipEventDestroy(ev);   // (hipHostFree below waits for whatever upload still reads the staging)
    if (ctx->light_stage) (void)hipHostFree(ctx->light_stage);
    for (gbl_ctx::EditTable* e : {&ctx->mat_edit, &ctx->tex_edit}) {   // (the row tables themselves are among ctx->allocations)
        for (hipEvent_t ev : e->ev)
            if (ev) (void)hipEventDestroy(ev);
        if (e->rows_uploaded) (void)hipEventDestroy(e->rows_uploaded);
        if (e->stage) (void)hipHostFree(e->stage);
    }
    for (const gbl_ctx::ImageTaps& taps : ctx->image_taps)
        if (taps.uploaded) (void)hipEventDestroy(taps.uploaded);   // (the tables themselves are among ctx->allocations)
    for (const gbl_ctx::Environment& env : ctx->environment)
        for (hipEvent_t ev : {env.uploaded, env.power_read})
            if (ev) (void)hipEventDestroy(ev);
    if (ctx->env_power_uploaded) (void)hipEventDestroy(ctx->env_power_uploaded);
    if (ctx->env_pinned) (void)hipHostFree(ctx->env_pinned);   // (it waits for whatever copy still uses it)
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
