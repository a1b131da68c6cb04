// The previous poses of gbl_render_motion_deform, checked and packed: see motion_stage.h.
#include "motion_stage.h"

#include <cmath>
#include <cstring>

bool check_motion_mesh(const gbl_mesh* meshes, size_t num_meshes, const gbl_motion_mesh& pm, uint32_t k, std::vector<bool>* listed, const char* who, std::string* err) {
    const std::string at = std::string(who) + ": prev_meshes[" + std::to_string(k) + "]";
    if (pm.mesh >= num_meshes) {
        *err = at + ": mesh " + std::to_string(pm.mesh) + " is out of range";
        return false;
    }
    const gbl_mesh& gm = meshes[pm.mesh];
    if (gm.shape != GBL_SHAPE_MESH) {
        *err = at + ": mesh " + std::to_string(pm.mesh) + " is a sphere or a disk: it has no vertices";
        return false;
    }
    if ((*listed)[pm.mesh]) {
        *err = at + ": mesh " + std::to_string(pm.mesh) + " is listed twice";
        return false;
    }
    (*listed)[pm.mesh] = true;
    if (pm.reserved != 0) {
        *err = at + ": reserved must be 0";
        return false;
    }
    if (!pm.positions) {
        *err = at + ": positions is NULL";
        return false;
    }
    return true;
}

std::string motion_mesh_not_finite(const char* who, uint32_t k, size_t i) {
    return std::string(who) + ": prev_meshes[" + std::to_string(k) + "]: a position of vertex " + std::to_string(i / 3) + " is not finite";
}

bool place_motion_mesh(const gbl_mesh& gm, uint32_t mesh, uint64_t* total, std::vector<int32_t>* table, const char* who, std::string* err) {
    // the table's difference and every packed index must be exact in an int32
    if (static_cast<uint64_t>(gm.vertex_offset) + gm.vertex_count > static_cast<uint64_t>(INT32_MAX) || *total + gm.vertex_count > static_cast<uint64_t>(INT32_MAX)) {
        *err = std::string(who) + ": prev_meshes: vertex numbers beyond 2^31 - 1";
        return false;
    }
    (*table)[mesh] = static_cast<int32_t>(static_cast<int64_t>(*total) - static_cast<int64_t>(gm.vertex_offset));
    *total += gm.vertex_count;
    return true;
}

bool stage_motion_meshes(const gbl_mesh* meshes, size_t num_meshes, const float* positions, const gbl_motion_mesh* prev, uint32_t num_prev,
                         const char* who, MotionStage* out, std::string* err) {
    const std::string head = std::string(who) + ": prev_meshes";
    out->table.assign(num_meshes, GBL_MOTION_NOT_DEFORMED);
    out->packed.clear();
    if (num_prev == 0) return true;
    if (!prev) {
        *err = head + " is NULL with num_prev_meshes > 0";
        return false;
    }
    // every entry is checked before any is packed: a refusal does not depend on which meshes happen to be unchanged
    std::vector<bool> listed(num_meshes, false);
    for (uint32_t k = 0; k < num_prev; ++k) {
        const gbl_motion_mesh& pm = prev[k];
        if (!check_motion_mesh(meshes, num_meshes, pm, k, &listed, who, err)) return false;
        const gbl_mesh& gm = meshes[pm.mesh];
        for (size_t i = 0; i < 3 * static_cast<size_t>(gm.vertex_count); ++i)
            if (!std::isfinite(pm.positions[i])) {
                *err = motion_mesh_not_finite(who, k, i);
                return false;
            }
    }
    uint64_t total = 0;
    for (uint32_t k = 0; k < num_prev; ++k) {
        const gbl_mesh& gm = meshes[prev[k].mesh];
        const size_t floats = 3 * static_cast<size_t>(gm.vertex_count);
        if (floats == 0 || memcmp(prev[k].positions, positions + 3 * static_cast<size_t>(gm.vertex_offset), floats * sizeof(float)) == 0) continue;   // bitwise: unchanged
        if (!place_motion_mesh(gm, prev[k].mesh, &total, &out->table, who, err)) return false;
        out->packed.insert(out->packed.end(), prev[k].positions, prev[k].positions + floats);
    }
    return true;
}
