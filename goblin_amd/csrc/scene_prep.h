// Host-side packing of a gbl_scene_desc into the device layout of device_scene.h.
#pragma once
#include <string>
#include <vector>

#include "../../include/goblin_hip.h"
#include "device_scene.h"

struct PackedScene {
    std::vector<DevNode> nodes;
    std::vector<DevTri> tris;
    std::vector<DevTriShade> tri_shade;
    std::vector<DevTriBound> tri_bounds;        // per original triangle (DevTri::shade)
    std::vector<DevTriBound> tri_bounds_leaf;   // ... and in the order of `tris` (host-built trees)
    std::vector<DevInstanceBound> instance_bounds;
    std::vector<DevTriOrder> tri_order;
    std::vector<float> positions;         // 3 per vertex
    std::vector<float> normals, uvs;
    std::vector<DevInstance> instances;
    std::vector<DevMaterial> materials;
    std::vector<DevTexture> textures;
    std::vector<DevImage> images;
    std::vector<float> ewa_lut, ibl_dist, vol_density;
    int32_t has_ibl = 0;
    std::vector<DevLight> lights;
    std::vector<DevLightTri> light_tris;
    std::vector<float> light_cdf, light_pick_pdf;
    std::vector<float> light_power;       // per light: what light_cdf and light_pick_pdf are made of (pack_light_distribution)
    float bound_lo[3], bound_hi[3];       // the scene bound the lights and the medium were packed with
    float filter_table[256];
    int32_t tlas_root = 0;
    int32_t stack_entries = 0;
    int32_t extended = 0;   // DevScene::extended
    int32_t scene_extended = 0;   // ... without the camera's part (camera_extended)
    int32_t has_masks = 0;  // DevScene::has_masks
    int32_t has_bssrdf = 0; // DevScene::has_bssrdf
    int32_t wh_slots = 0;   // DevScene::wh_slots
    DevVolume volume = {};
    uint64_t blas_nodes = 0, tlas_nodes = 0;
    int blas_max_depth = 0, tlas_depth = 0;
    std::vector<int> mesh_stack_need;      // per mesh: most entries a ray can have on its stack inside its BLAS (exact for host-built trees)
    std::vector<float> mesh_lo, mesh_hi;   // 3 per mesh: object bounds
    std::vector<int32_t> mesh_root;        // per mesh: BLAS root reference
    int32_t tlas_base = 0;                 // device index of TLAS node 0
    uint32_t tlas_capacity = 0;            // nodes reserved at tlas_base (any TLAS over the instances fits)
    uint32_t hot_nodes = 0;                // nodes[0 .. hot_nodes): the top of the two-level tree in breadth-first order (hot_prefix)
    DevCamera camera;
    DevFilm film;
};

// Returns GBL_OK or an error with *err set; every refusal is made before anything is written to *out.
// device_blas: leave the triangle BLASes to the device builder (kernels/lbvh.h): `nodes` then holds the TLAS only
// (at indices 0..), `tris` stays empty, mesh instances get root = 0 (patched after the device build) and
// `mesh_lo/hi` carry the object bounds the Morton codes are scaled by.
gbl_status pack_scene(const gbl_scene_desc* desc, PackedScene* out, std::string* err, bool device_blas = false);

// The device camera of a description under a film's resolution: what gbl_create, gbl_update_camera and gbl_film_accumulate (for
// its previous camera) share.  The type is the caller's to check.
void pack_camera(const gbl_camera& camera, const gbl_film& film, DevCamera* out);
// The camera's part of DevScene::extended: a thin lens or an orthographic camera needs the EXT kernels
bool camera_extended(const gbl_camera& camera);

// The instance records and the TLAS over them (pack_scene; gbl_update_instances rebuilds with it after transform edits).
struct TlasInput {
    const gbl_instance* instances;
    uint32_t count;
    const gbl_mesh* meshes;
    const gbl_material* materials;
    const float *mesh_lo, *mesh_hi;   // 3 per mesh: object bounds
    const int32_t* mesh_root;         // per mesh: BLAS root reference
    int32_t tlas_base;                // device index of TLAS node 0
};
struct TlasResult {
    std::vector<DevInstance> instances;
    std::vector<DevNode> nodes;
    std::vector<DevInstanceBound> instance_bounds;
    int32_t root = 0;
    int depth = 0;
    float bound_lo[3], bound_hi[3];   // the scene bound: the union of the instance boxes
};
// Refuses (GBL_ERR_INVALID, *err set, *out unspecified) an instance whose transform the reference cannot invert.
gbl_status build_tlas(const TlasInput& in, TlasResult* out, std::string* err);
// build_tlas's tree alone, over instance world boxes composed elsewhere (gbl_update_instances_device composes them on the
// device): fed the boxes build_tlas stores, it returns build_tlas's nodes, root and depth.  Cannot fail.
void build_tlas_nodes(const DevInstanceBound* bounds, uint32_t count, int32_t tlas_base, std::vector<DevNode>* nodes, int32_t* root, int* depth);

// The 3x4 rows of a transform and of its inverse as build_tlas composes them for DevInstance::m / inv (gbl_render_motion's
// previous transforms).  false, *err set to build_tlas's refusal for instance i, when the reference cannot invert it.
bool pack_transform(const gbl_trs& to_world, uint32_t i, float m[12], float inv[12], std::string* err);

// The part of a light's record that its gbl_light and the scene bound decide -- type, colour, position, cone, axis, m / inv --
// and the light's power: what pack_scene writes per light and gbl_update_lights writes again.  `dl` arrives with the part the
// scene's geometry decides already in place (pack_scene attaches it; an edit keeps it): tri_first, tri_count, sum_area, shape,
// radius, wh_n, wh_prefix, image, dist_*.  An image based light's power is that of its texels over the scene bound, neither of
// which an edit can change: `kept_power` is returned for it (pack_scene passes what it has just worked out).
float pack_light(const gbl_light& gl, const float bound_lo[3], const float bound_hi[3], float kept_power, DevLight* dl);
// The power distribution over the lights (Scene ctor, CDF1D::init): cdf gets power.size() + 1 floats, pick_pdf
// max(1, power.size()).
void pack_light_distribution(const std::vector<float>& power, std::vector<float>* cdf, std::vector<float>* pick_pdf);
// Both over a context's tables: lights [first, first + count) replaced by `edited`, their records and powers packed again,
// then the distribution.  The other lights' records and powers stay as they are.
void repack_lights(const gbl_light* edited, uint32_t first, uint32_t count, const float bound_lo[3], const float bound_hi[3], std::vector<DevLight>* lights,
                   std::vector<float>* power, std::vector<float>* cdf, std::vector<float>* pick_pdf);

// A material's and a texture's record as pack_scene writes them, over a context's tables (gbl_update_materials,
// gbl_update_textures).  `all` is the whole patched description of `num` materials: records [first, first + count) are packed
// again, and so is every mask that wraps one of them (its record carries the wrapped material's has_tex, tex_bump and
// tex_normal); *touched lists the records written, ascending.  The editable values go through kernels/materials.h's mat_compose /
// tex_compose, which the device forms of the edits run as well.
void repack_materials(const gbl_material* all, uint32_t num, uint32_t first, uint32_t count, std::vector<DevMaterial>* records, std::vector<uint32_t>* touched);
void repack_textures(const gbl_texture* edited, uint32_t first, uint32_t count, std::vector<DevTexture>* records);
// validate_desc's checks on the occupied texture slots of materials [first, first + count) of a patched description -- in range,
// no cyclic graph, no deeper than GBL_TEX_MAX_DEPTH -- with its statuses and messages.
gbl_status check_material_slots(const gbl_material* materials, uint32_t num_materials, const gbl_texture* textures, uint32_t num_textures, uint32_t first, uint32_t count,
                                std::string* err);

// What an image based light's tables take from the host besides its texels, stated once for pack_scene and for
// gbl_update_environment: sin(theta) at the centre of each of the distribution's dist_h rows (ImageBasedLight's constructor,
// with the loader's sinf), and the area 4 pi r^2 of the scene bound's sphere that its power is taken over.
void ibl_sin_theta(uint32_t dist_h, std::vector<float>* table);
float ibl_sphere_area(const float bound_lo[3], const float bound_hi[3]);

// One mesh's DevTriOrder records (the reference's visiting order, per mesh-local triangle number) and its object bound (the
// bound of ALL its vertices), as pack_scene makes them: gbl_update_vertices makes them again over edited positions.
// `positions` is the mesh's first vertex, `indices` its first (mesh-local) index.
void mesh_reference_order(const float* positions, const uint32_t* indices, uint32_t tri_count, DevTriOrder* out);
void mesh_object_bound(const float* positions, uint32_t vertex_count, float lo[3], float hi[3]);

// Traversal stack entries a scene needs (kernels/trace.h): exit marker + the worst root-to-leaf sum over the TLAS nodes
// (tlas[0..] are the nodes at absolute indices tlas_base + i) of (children - 1), + per instance its sentinel and what its
// mesh's BLAS needs, + one spare.
int scene_stack_entries(const std::vector<DevNode>& tlas, int32_t tlas_base, int32_t tlas_root, const std::vector<DevInstance>& instances,
                        const std::vector<int>& mesh_stack_need);
