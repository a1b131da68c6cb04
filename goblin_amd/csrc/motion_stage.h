// The host side of gbl_render_motion_deform's previous poses: the list of gbl_motion_mesh checked against the
// context's meshes, the deformed ones told from the unchanged, and their previous positions packed for the device.  Host only
// and free of HIP, as scene_refit.h is: tests/deform_stage.cpp builds it stand-alone with g++.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/goblin_hip.h"

#define GBL_MOTION_NOT_DEFORMED INT32_MIN   // MotionStage::table's entry of a mesh the kernels treat as static

struct MotionStage {
    std::vector<int32_t> table;   // per mesh of the scene: packed_first_vertex - vertex_offset, or GBL_MOTION_NOT_DEFORMED
    std::vector<float> packed;    // 3 per vertex: the previous positions of the deformed meshes, one mesh after the other as listed
    bool any() const { return !packed.empty(); }
};

// `meshes` (num_meshes records) and `positions` (3 floats per vertex of the scene) are the context's.  A listed mesh is deformed
// iff its previous positions differ bitwise from its slice of `positions`; an unchanged one is dropped.  false with *err set
// (naming `who`) and *out unspecified for: a NULL list with num_prev > 0, a NULL positions pointer, a mesh index out of range, a
// sphere or a disk, a mesh listed twice, reserved != 0 and a non-finite coordinate.  Nothing but *out and *err is written.
bool stage_motion_meshes(const gbl_mesh* meshes, size_t num_meshes, const float* positions, const gbl_motion_mesh* prev, uint32_t num_prev,
                         const char* who, MotionStage* out, std::string* err);

// The pieces of stage_motion_meshes that do not read a coordinate, for gbl_render_motion_deform_device, whose positions lie in
// device memory (api_motion.hip): entry k's checks in stage_motion_meshes' order and words (`listed`: one flag per mesh of the
// scene, set for the meshes of the entries before k); the message of a non-finite float i of entry k; and a deformed mesh's entry
// of the table, its packed positions beginning at vertex *total, which moves on by the mesh's vertex count.
bool check_motion_mesh(const gbl_mesh* meshes, size_t num_meshes, const gbl_motion_mesh& pm, uint32_t k, std::vector<bool>* listed, const char* who, std::string* err);
std::string motion_mesh_not_finite(const char* who, uint32_t k, size_t i);
bool place_motion_mesh(const gbl_mesh& gm, uint32_t mesh, uint64_t* total, std::vector<int32_t>* table, const char* who, std::string* err);
