// libgoblin_hip.so -- C ABI of the device integrator (include/goblin_hip.h): material and texture edits.
// The host forms validate the given records against the ones the context holds, pack them with the functions gbl_create packs
// them with (scene_prep.h repack_materials / repack_textures) and queue the uploads on the caller's stream from pinned staging the
// context owns: no kernel is launched and the device is not synchronised.  The device forms read raw rows from device memory: one
// copy into the context's row table and one compose kernel (kernels/materials.h), whose arithmetic is the packers' own.  The host
// description becomes a mirror that the next reader refreshes.  gbl_get_* and the self-test hook go with them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "gbl_host.h"
#include "kernels/materials.h"
#include "scene_prep.h"

namespace {

const char* const kWhoMat = "gbl_update_materials";
const char* const kWhoTex = "gbl_update_textures";
const char* const kWhoMatDev = "gbl_update_materials_device";
const char* const kWhoTexDev = "gbl_update_textures_device";

bool all_finite(const float* f, int n) {
    for (int k = 0; k < n; ++k)
        if (!std::isfinite(f[k])) return false;
    return true;
}

std::string material_name(uint32_t i) { return std::string(kWhoMat) + ": material " + std::to_string(i) + ": "; }
std::string texture_name(uint32_t i) { return std::string(kWhoTex) + ": texture " + std::to_string(i) + ": "; }

// What the two tables' edits differ in
struct MatTable {
    typedef gbl_material Desc;
    typedef DevMaterial Record;
    static const int kRow = GBL_MAT_ROW_FLOATS;
    static std::vector<Desc>& desc(gbl_ctx* ctx) { return ctx->h_materials; }
    static gbl_ctx::EditTable& edit(gbl_ctx* ctx) { return ctx->mat_edit; }
    static Record* device(gbl_ctx* ctx) { return const_cast<Record*>(ctx->scene.materials); }
    static void row_of(const Desc& d, float* row) { mat_row_of(d, row); }
    static void row_into(const float* row, Desc* d) {
        for (int k = 0; k < 3; ++k) d->color[k] = row[k], d->color2[k] = row[3 + k], d->color3[k] = row[6 + k];
        d->index = row[9], d->k = row[10], d->exponent = row[11];
    }
    static void launch(gbl_ctx* ctx, const float* rows, uint32_t first, uint32_t count, hipStream_t stream) {
        gbl_launch_mat_compose(MatComposeArgs{device(ctx), rows, first, count}, stream);
    }
};
struct TexTable {
    typedef gbl_texture Desc;
    typedef DevTexture Record;
    static const int kRow = GBL_TEX_ROW_FLOATS;
    static std::vector<Desc>& desc(gbl_ctx* ctx) { return ctx->h_textures; }
    static gbl_ctx::EditTable& edit(gbl_ctx* ctx) { return ctx->tex_edit; }
    static Record* device(gbl_ctx* ctx) { return const_cast<Record*>(ctx->scene.textures); }
    static void row_of(const Desc& d, float* row) { tex_row_of(d, row); }
    static void row_into(const float* row, Desc* d) {
        for (int k = 0; k < 3; ++k) d->value[k] = row[k];
        for (int k = 0; k < 2; ++k) d->uv_scale[k] = row[3 + k], d->uv_offset[k] = row[5 + k];
    }
    static void launch(gbl_ctx* ctx, const float* rows, uint32_t first, uint32_t count, hipStream_t stream) {
        gbl_launch_tex_compose(TexComposeArgs{device(ctx), rows, first, count}, stream);
    }
};

// The host description of a table brought up to the device's raw rows, if a device edit left a range of it stale: one
// device-to-host copy of that range behind a synchronise (refresh_instance_mirror's pattern).  Every reader of the editable
// fields calls it first: gbl_get_*, and the host forms, whose fixed-field checks read the mirror.
template <class T>
gbl_status refresh_table_mirror(gbl_ctx* ctx) {
    gbl_ctx::EditTable& e = T::edit(ctx);
    if (e.stale_end <= e.stale_first || !e.d_rows) return GBL_OK;
    const uint32_t first = e.stale_first, count = std::min<uint32_t>(e.stale_end, static_cast<uint32_t>(T::desc(ctx).size())) - first;
    std::vector<float> fresh(static_cast<size_t>(count) * T::kRow);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipDeviceSynchronize());
    HIP_TRY(ctx, hipMemcpy(fresh.data(), e.d_rows + static_cast<size_t>(first) * T::kRow, fresh.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < count; ++i) T::row_into(&fresh[static_cast<size_t>(i) * T::kRow], &T::desc(ctx)[first + i]);
    e.stale_first = e.stale_end = 0;
    return GBL_OK;
}

// ---------------------------------------------------------------- the host forms' checks
// The fields that fix `extended`, has_masks, has_bssrdf, DevInstance::is_mask and the choice of kernels
gbl_status check_fixed_fields(gbl_ctx* ctx, uint32_t i, const gbl_material& have, const gbl_material& want) {
    const auto fixed = [&](const char* field, long long h, long long w) {
        return fail(ctx, GBL_ERR_INVALID, material_name(i) + field + " cannot change (the context holds " + std::to_string(h) + ", the call gives " + std::to_string(w) + ")");
    };
    if (want.type != have.type) return fixed("type", have.type, want.type);
    if (want.masked_material != have.masked_material) return fixed("masked_material", have.masked_material, want.masked_material);
    const struct { const char* name; int32_t h, w; } slots[6] = {{"tex_color", have.tex_color, want.tex_color},          {"tex_color2", have.tex_color2, want.tex_color2},
                                                                 {"tex_exponent", have.tex_exponent, want.tex_exponent}, {"tex_color3", have.tex_color3, want.tex_color3},
                                                                 {"tex_bump", have.tex_bump, want.tex_bump},             {"tex_normal", have.tex_normal, want.tex_normal}};
    for (const auto& s : slots)
        if ((s.h >= 0) != (s.w >= 0))
            return fail(ctx, GBL_ERR_INVALID, material_name(i) + s.name + ": a texture slot cannot be occupied or vacated (the context holds " + std::to_string(s.h) +
                                              ", the call gives " + std::to_string(s.w) + ")");
    return GBL_OK;
}

gbl_status check_fixed_fields(gbl_ctx* ctx, uint32_t i, const gbl_texture& have, const gbl_texture& want) {
    const auto fixed = [&](const char* field, long long h, long long w) {
        return fail(ctx, GBL_ERR_INVALID, texture_name(i) + field + " cannot change (the context holds " + std::to_string(h) + ", the call gives " + std::to_string(w) + ")");
    };
    if (want.type != have.type) return fixed("type", have.type, want.type);
    if (want.is_float != have.is_float) return fixed("is_float", have.is_float, want.is_float);
    if (want.child[0] != have.child[0]) return fixed("child[0]", have.child[0], want.child[0]);
    if (want.child[1] != have.child[1]) return fixed("child[1]", have.child[1], want.child[1]);
    if (want.mapping != have.mapping) return fixed("mapping", have.mapping, want.mapping);
    if (want.image != have.image) return fixed("image", have.image, want.image);
    if (want.filter != have.filter) return fixed("filter", have.filter, want.filter);
    if (want.image_filter != have.image_filter) return fixed("image_filter", have.image_filter, want.image_filter);
    if (want.address != have.address) return fixed("address", have.address, want.address);
    return GBL_OK;
}

gbl_status check_values(gbl_ctx* ctx, uint32_t i, const gbl_material& want) {
    const auto not_finite = [&](const char* field) { return fail(ctx, GBL_ERR_INVALID, material_name(i) + field + " is not finite"); };
    if (!all_finite(want.color, 3)) return not_finite("color");
    if (!all_finite(want.color2, 3)) return not_finite("color2");
    if (want.type == GBL_MAT_SUBSURFACE && !all_finite(want.color3, 3)) return not_finite("color3");
    if (!std::isfinite(want.index)) return not_finite("index");
    if (!std::isfinite(want.k)) return not_finite("k");
    if (!std::isfinite(want.exponent)) return not_finite("exponent");
    return GBL_OK;
}

gbl_status check_values(gbl_ctx* ctx, uint32_t i, const gbl_texture& want) {
    const auto not_finite = [&](const char* field) { return fail(ctx, GBL_ERR_INVALID, texture_name(i) + field + " is not finite"); };
    if (!all_finite(want.value, 3)) return not_finite("value");
    if (!all_finite(want.uv_scale, 2)) return not_finite("uv_scale");
    if (!all_finite(want.uv_offset, 2)) return not_finite("uv_offset");
    if (!(all_finite(want.to_tex.position, 3) && all_finite(want.to_tex.orientation, 4) && all_finite(want.to_tex.scale, 3))) return not_finite("to_tex");
    if (!std::isfinite(want.max_anisotropy)) return not_finite("max_anisotropy");
    if ((want.type == GBL_TEX_CHECKERBOARD || want.type == GBL_TEX_IMAGE) && want.mapping == GBL_MAP_SPHERICAL) {
        float m[12], inv[12];
        std::string why;
        if (!pack_transform(want.to_tex, i, m, inv, &why)) return fail(ctx, GBL_ERR_INVALID, texture_name(i) + "to_tex: " + why);
    }
    return GBL_OK;
}

// A slot pointed at another texture keeps its kind: a float texture in tex_exponent and tex_bump, a colour texture in the others
gbl_status check_slot_kinds(gbl_ctx* ctx, uint32_t i, const gbl_material& have, const gbl_material& want) {
    const struct { const char* name; int32_t h, w; uint32_t is_float; } slots[6] = {
        {"tex_color", have.tex_color, want.tex_color, 0u},          {"tex_color2", have.tex_color2, want.tex_color2, 0u}, {"tex_exponent", have.tex_exponent, want.tex_exponent, 1u},
        {"tex_color3", have.tex_color3, want.tex_color3, 0u},       {"tex_bump", have.tex_bump, want.tex_bump, 1u},       {"tex_normal", have.tex_normal, want.tex_normal, 0u}};
    for (const auto& s : slots) {
        if (s.w < 0 || s.w == s.h || static_cast<size_t>(s.w) >= ctx->h_textures.size()) continue;   // (a slot this type does not read may hold anything)
        if ((ctx->h_textures[s.w].is_float != 0u) != (s.is_float != 0u))
            return fail(ctx, GBL_ERR_INVALID, material_name(i) + s.name + ": texture " + std::to_string(s.w) + " is a " + (s.is_float ? "colour" : "float") + " texture, the slot takes a " +
                                              (s.is_float ? "float" : "colour") + " texture");
    }
    return GBL_OK;
}

// ---------------------------------------------------------------- staging and uploads
// A slot of the pinned staging holds the table's records, then its raw rows
template <class T>
struct StageLayout {
    size_t rows, slot;
    explicit StageLayout(size_t n) {
        const auto pad = [](size_t b) { return (b + 255) & ~static_cast<size_t>(255); };
        rows = pad(std::max<size_t>(1, n) * sizeof(typename T::Record));
        slot = rows + pad(std::max<size_t>(1, n) * T::kRow * sizeof(float));
    }
};

// The next staging slot, free to write: a slot is written again only after the uploads that last read it (queue_tables' rule)
template <class T>
gbl_status claim_slot(gbl_ctx* ctx, const char* who, int* slot_out, unsigned char** base) {
    gbl_ctx::EditTable& e = T::edit(ctx);
    const StageLayout<T> at(T::desc(ctx).size());
    if (!e.stage) {
        void* p = nullptr;
        if (hipHostMalloc(&p, at.slot * gbl_ctx::kLightSlots, hipHostMallocDefault) != hipSuccess) return fail(ctx, GBL_ERR_OOM, std::string(who) + ": hipHostMalloc(staging) failed");
        e.stage = static_cast<unsigned char*>(p);
    }
    const int slot = static_cast<int>(e.edits % gbl_ctx::kLightSlots);
    if (!e.ev[slot]) HIP_TRY(ctx, hipEventCreateWithFlags(&e.ev[slot], hipEventDisableTiming));
    else HIP_TRY(ctx, hipEventSynchronize(e.ev[slot]));
    *slot_out = slot;
    *base = e.stage + at.slot * slot;
    return GBL_OK;
}

// Records `touched` (ascending) of `records` and the raw rows of [first, first + count) go to the device in the stream's order
template <class T>
gbl_status queue_records(gbl_ctx* ctx, const char* who, const std::vector<typename T::Record>& records, const std::vector<uint32_t>& touched, uint32_t first, uint32_t count,
                         hipStream_t stream) {
    typedef typename T::Record Record;
    gbl_ctx::EditTable& e = T::edit(ctx);
    int slot = 0;
    unsigned char* s = nullptr;
    const gbl_status st = claim_slot<T>(ctx, who, &slot, &s);
    if (st != GBL_OK) return st;
    Record* const staged = reinterpret_cast<Record*>(s);
    for (size_t a = 0; a < touched.size();) {
        size_t b = a + 1;
        while (b < touched.size() && touched[b] == touched[b - 1] + 1) ++b;   // one upload per run of neighbours
        const uint32_t at = touched[a];
        memcpy(staged + at, &records[at], (b - a) * sizeof(Record));
        HIP_TRY(ctx, hipMemcpyAsync(T::device(ctx) + at, staged + at, (b - a) * sizeof(Record), hipMemcpyHostToDevice, stream));
        a = b;
    }
    if (e.d_rows) {   // a device edit has made the row table: it follows every edit
        float* const rows = reinterpret_cast<float*>(s + StageLayout<T>(T::desc(ctx).size()).rows) + static_cast<size_t>(first) * T::kRow;
        for (uint32_t i = 0; i < count; ++i) T::row_of(T::desc(ctx)[first + i], rows + static_cast<size_t>(i) * T::kRow);
        if (e.rows_uploaded) HIP_TRY(ctx, hipStreamWaitEvent(stream, e.rows_uploaded, 0));
        HIP_TRY(ctx, hipMemcpyAsync(e.d_rows + static_cast<size_t>(first) * T::kRow, rows, static_cast<size_t>(count) * T::kRow * sizeof(float), hipMemcpyHostToDevice, stream));
    }
    HIP_TRY(ctx, hipEventRecord(e.ev[slot], stream));
    ++e.edits;
    return GBL_OK;
}

// ---------------------------------------------------------------- the host forms
gbl_status gbl_update_materials_impl(gbl_ctx* ctx, uint32_t first, uint32_t count, const gbl_material* materials, void* stream) {
    if (!ctx) return GBL_ERR_INVALID;
    // arguments, range, the fields that cannot change, values, references: nothing is written before the last of them
    if (!materials) return fail(ctx, GBL_ERR_INVALID, std::string(kWhoMat) + ": materials is NULL");
    const size_t n = ctx->h_materials.size();
    if (static_cast<uint64_t>(first) + count > n) return fail(ctx, GBL_ERR_INVALID, std::string(kWhoMat) + ": material range out of bounds");
    if (count == 0) return GBL_OK;
    gbl_status st = GBL_OK;
    if ((st = refresh_table_mirror<MatTable>(ctx)) != GBL_OK) return st;   // (the checks below read the mirror)
    for (uint32_t i = 0; i < count; ++i)
        if ((st = check_fixed_fields(ctx, first + i, ctx->h_materials[first + i], materials[i])) != GBL_OK) return st;
    for (uint32_t i = 0; i < count; ++i)
        if ((st = check_values(ctx, first + i, materials[i])) != GBL_OK) return st;
    for (uint32_t i = 0; i < count; ++i)
        if ((st = check_slot_kinds(ctx, first + i, ctx->h_materials[first + i], materials[i])) != GBL_OK) return st;
    // validate_desc's slot checks on the patched table; a refusal puts the held records back
    const std::vector<gbl_material> held(ctx->h_materials.begin() + first, ctx->h_materials.begin() + first + count);
    std::copy(materials, materials + count, ctx->h_materials.begin() + first);
    std::string why;
    st = check_material_slots(ctx->h_materials.data(), static_cast<uint32_t>(n), ctx->h_textures.data(), static_cast<uint32_t>(ctx->h_textures.size()), first, count, &why);
    if (st != GBL_OK) {
        std::copy(held.begin(), held.end(), ctx->h_materials.begin() + first);
        return fail(ctx, st, std::string(kWhoMat) + ": " + why);
    }
    std::vector<uint32_t> touched;
    repack_materials(ctx->h_materials.data(), static_cast<uint32_t>(n), first, count, &ctx->mat_records, &touched);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((st = queue_records<MatTable>(ctx, kWhoMat, ctx->mat_records, touched, first, count, static_cast<hipStream_t>(stream))) != GBL_OK) return st;
    ctx->auto_rays_per_path.clear();   // the pilot's rays per path belong to the old surfaces: AUTO measures again
    return GBL_OK;
}

gbl_status gbl_update_textures_impl(gbl_ctx* ctx, uint32_t first, uint32_t count, const gbl_texture* textures, void* stream) {
    if (!ctx) return GBL_ERR_INVALID;
    if (!textures) return fail(ctx, GBL_ERR_INVALID, std::string(kWhoTex) + ": textures is NULL");
    const size_t n = ctx->h_textures.size();
    if (static_cast<uint64_t>(first) + count > n) return fail(ctx, GBL_ERR_INVALID, std::string(kWhoTex) + ": texture range out of bounds");
    if (count == 0) return GBL_OK;
    gbl_status st = GBL_OK;
    if ((st = refresh_table_mirror<TexTable>(ctx)) != GBL_OK) return st;
    for (uint32_t i = 0; i < count; ++i)
        if ((st = check_fixed_fields(ctx, first + i, ctx->h_textures[first + i], textures[i])) != GBL_OK) return st;
    for (uint32_t i = 0; i < count; ++i)
        if ((st = check_values(ctx, first + i, textures[i])) != GBL_OK) return st;
    // (children are fixed: a texture edit cannot change the graph, so there is no reference to check)
    repack_textures(textures, first, count, &ctx->tex_records);
    std::copy(textures, textures + count, ctx->h_textures.begin() + first);
    std::vector<uint32_t> touched(count);
    for (uint32_t i = 0; i < count; ++i) touched[i] = first + i;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((st = queue_records<TexTable>(ctx, kWhoTex, ctx->tex_records, touched, first, count, static_cast<hipStream_t>(stream))) != GBL_OK) return st;
    ctx->auto_rays_per_path.clear();
    return GBL_OK;
}

template <class T>
gbl_status get_records(gbl_ctx* ctx, uint32_t first, uint32_t count, typename T::Desc* out) {
    if (!ctx || !out || static_cast<uint64_t>(first) + count > T::desc(ctx).size()) return GBL_ERR_INVALID;
    const gbl_status st = refresh_table_mirror<T>(ctx);
    if (st != GBL_OK) return st;
    std::copy(T::desc(ctx).begin() + first, T::desc(ctx).begin() + first + count, out);
    return GBL_OK;
}

// ---------------------------------------------------------------- the device forms
template <class T>
gbl_status update_device(gbl_ctx* ctx, const char* who, const char* what, uint32_t first, uint32_t count, const float* rows, void* stream_) {
    if (!ctx) return GBL_ERR_INVALID;
    // arguments, range, the pointer: nothing is launched on any of them
    if (!rows) return fail(ctx, GBL_ERR_INVALID, std::string(who) + ": rows is NULL");
    const size_t n = T::desc(ctx).size();
    if (static_cast<uint64_t>(first) + count > n) return fail(ctx, GBL_ERR_INVALID, std::string(who) + ": " + what + " range out of bounds");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t bytes = static_cast<size_t>(count) * T::kRow * sizeof(float);
    const gbl_status st = check_device_pointer(ctx, rows, bytes, who, "rows");
    if (st != GBL_OK) return st;
    if (count == 0) return GBL_OK;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    gbl_ctx::EditTable& e = T::edit(ctx);
    if (!e.d_rows) {   // the row table, made from the host copy (which no device edit has left stale yet) and uploaded once
        void* p = nullptr;
        const gbl_status sa = device_alloc(ctx, n * T::kRow * sizeof(float), who, &p);
        if (sa != GBL_OK) return sa;
        e.h_rows.resize(n * T::kRow);
        for (size_t i = 0; i < n; ++i) T::row_of(T::desc(ctx)[i], &e.h_rows[i * T::kRow]);
        HIP_TRY(ctx, hipEventCreateWithFlags(&e.rows_uploaded, hipEventDisableTiming));
        HIP_TRY(ctx, hipMemcpyAsync(p, e.h_rows.data(), e.h_rows.size() * sizeof(float), hipMemcpyHostToDevice, stream));
        HIP_TRY(ctx, hipEventRecord(e.rows_uploaded, stream));
        e.d_rows = static_cast<float*>(p);
    } else {
        HIP_TRY(ctx, hipStreamWaitEvent(stream, e.rows_uploaded, 0));
    }
    HIP_TRY(ctx, hipMemcpyAsync(e.d_rows + static_cast<size_t>(first) * T::kRow, rows, bytes, hipMemcpyDeviceToDevice, stream));
    T::launch(ctx, rows, first, count, stream);
    HIP_TRY(ctx, hipGetLastError());
    if (e.stale_end <= e.stale_first) e.stale_first = first, e.stale_end = first + count;
    else e.stale_first = std::min(e.stale_first, first), e.stale_end = std::max(e.stale_end, first + count);
    ctx->auto_rays_per_path.clear();
    return GBL_OK;
}

gbl_status gbl_selftest_materials_impl(gbl_ctx* ctx, void* materials_out, void* textures_out, uint64_t* num_materials, uint64_t* num_textures) {
    if (!ctx) return GBL_ERR_INVALID;
    const size_t nm = ctx->h_materials.size(), nt = ctx->h_textures.size();
    if (num_materials) *num_materials = nm;
    if (num_textures) *num_textures = nt;
    if (!materials_out && !textures_out) return GBL_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipDeviceSynchronize());
    if (materials_out && nm > 0) HIP_TRY(ctx, hipMemcpy(materials_out, ctx->scene.materials, nm * sizeof(DevMaterial), hipMemcpyDeviceToHost));
    if (textures_out && nt > 0) HIP_TRY(ctx, hipMemcpy(textures_out, ctx->scene.textures, nt * sizeof(DevTexture), hipMemcpyDeviceToHost));
    return GBL_OK;
}

}   // namespace

extern "C" {

gbl_status gbl_update_materials(gbl_ctx* ctx, uint32_t first, uint32_t count, const gbl_material* materials, void* stream) {
    return gbl_guard([&] { return gbl_update_materials_impl(ctx, first, count, materials, stream); }, [&](const std::string& what) { if (ctx) ctx->error = what; });
}

gbl_status gbl_get_materials(gbl_ctx* ctx, uint32_t first, uint32_t count, gbl_material* out) {
    return gbl_guard([&] { return get_records<MatTable>(ctx, first, count, out); }, [&](const std::string& what) { if (ctx) ctx->error = what; });
}

gbl_status gbl_update_textures(gbl_ctx* ctx, uint32_t first, uint32_t count, const gbl_texture* textures, void* stream) {
    return gbl_guard([&] { return gbl_update_textures_impl(ctx, first, count, textures, stream); }, [&](const std::string& what) { if (ctx) ctx->error = what; });
}

gbl_status gbl_get_textures(gbl_ctx* ctx, uint32_t first, uint32_t count, gbl_texture* out) {
    return gbl_guard([&] { return get_records<TexTable>(ctx, first, count, out); }, [&](const std::string& what) { if (ctx) ctx->error = what; });
}

gbl_status gbl_update_materials_device(gbl_ctx* ctx, uint32_t first, uint32_t count, const float* d_rows, void* stream) {
    return gbl_guard([&] { return update_device<MatTable>(ctx, kWhoMatDev, "material", first, count, d_rows, stream); }, [&](const std::string& what) { if (ctx) ctx->error = what; });
}

gbl_status gbl_update_textures_device(gbl_ctx* ctx, uint32_t first, uint32_t count, const float* d_rows, void* stream) {
    return gbl_guard([&] { return update_device<TexTable>(ctx, kWhoTexDev, "texture", first, count, d_rows, stream); }, [&](const std::string& what) { if (ctx) ctx->error = what; });
}

gbl_status gbl_selftest_materials(gbl_ctx* ctx, void* materials_out, void* textures_out, uint64_t* num_materials, uint64_t* num_textures) {
    return gbl_guard([&] { return gbl_selftest_materials_impl(ctx, materials_out, textures_out, num_materials, num_textures); }, [&](const std::string& what) { if (ctx) ctx->error = what; });
}

}   // extern "C"
