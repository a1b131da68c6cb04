// Internal to libgoblin_hip.so: the context behind the C ABI's opaque handle and the table of device kernels.
//
// The kernels live in translation units of their own (kernels_*.hip), compiled side by side; the host side of the ABI
// (api_*.hip, gbl_host.h) picks an instantiation through the selectors below and launches it by pointer.  A selector returns
// nullptr for a combination that is not built.
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/goblin_hip.h"
#include "device_scene.h"
#include "kernels/wf_args.h"
#include "kernels/aov_args.h"
#include "kernels/denoise_args.h"
#include "kernels/temporal_args.h"
#include "kernels/motion_args.h"
#include "kernels/refit_args.h"
#include "kernels/vertices_args.h"
#include "kernels/query_args.h"
#include "kernels/query_filtered_args.h"
#include "kernels/radiance_args.h"
#include "kernels/pyramid_args.h"
#include "kernels/environment_args.h"
#include "kernels/materials_args.h"

// A device buffer of the context, grown on demand (gbl_host.h grow()) and freed by gbl_destroy
struct gbl_buf {
    void* p = nullptr;
    uint64_t bytes = 0;
};

struct gbl_ctx {
    int device = 0;
    std::string error;
    std::vector<void*> allocations;
    DevScene scene;
    gbl_info info;
    uint32_t* work_counter = nullptr;
    unsigned long long* stats = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int num_cus = 256;
    void* rccl = nullptr;
    void* rccl_allreduce = nullptr;
    // wavefront pool (allocated on first use)
    uint32_t wf_pool = 0;
    hipStream_t wf_aux = nullptr;   // shadow rays of iteration k trace here while the main stream traces extension rays k+1
    hipEvent_t wf_ev_shade = nullptr, wf_ev_shadow = nullptr;
    WfArgs wf;
    uint64_t li_budget = 0;   // li_budget_bytes()
    uint32_t* stream_seeds = nullptr;   // GBL_SAMPLES_STREAM: per-tile mt19937 seeds of the full sample window
    // buffers of the render in flight
    gbl_buf li;               // per-sample radiance (float4) when the caller passes no li_out
    gbl_buf prim_hits;        // the primary pass's hits: entries x (float4 + int32)
    gbl_buf prim_items;       // ... and its word per work item of the path kernel (RenderArgs::prim_items)
    gbl_buf vol;              // per-sample {transmittance, Lv} (scenes with a participating medium)
    gbl_buf sss;              // per-sample Lsubsurface (scenes with subsurface materials)
    gbl_buf aov;              // gbl_render_aov: a chunk's per-sample feature planes (float4 each, up to three)
    gbl_buf stream_scratch;   // GBL_SAMPLES_STREAM: the workgroups' sample-generation scratch ...
    gbl_buf stream_xy;        // ... and the image position of every camera sample of the call (for the splat)
    gbl_buf wf_spill;         // the wavefront trace stacks' levels beyond LDS (wf_ensure_spill) ...
    int wf_spill_levels = 0;  // ... how many it holds
    // gbl_film_develop's scratch (kernels/develop.h)
    gbl_buf dev_rgb1;         // the normalised image as {r, g, b, 1} per pixel: what the bloom's windows and its blend read
    gbl_buf dev_rgb;          // the developed image when the caller asks for bytes only
    gbl_buf dev_logs;         // the tone map's logf(1e4 + luminance) per pixel, then 1 / Ywa^2 in one float after them
    gbl_buf dev_filter;       // the bloom's filter table ...
    int dev_filter_fw = 0;    // ... and the filter width it was built for (0: none yet)
    gbl_buf denoise;          // gbl_film_denoise's four float4 planes (kernels/denoise.h): cv ping, cv pong, nz, af
    bool denoise_lds_allowed = false;   // ... its staging level kernel may be launched with more than 64 KB of LDS on this device
    gbl_buf temporal;         // gbl_film_accumulate's prepared frame (kernels/temporal.h): cl, nz (float4 each) and the flags
    gbl_buf motion;           // gbl_render_motion's previous-transform table and moved flags (kernels/motion_args.h) ...
    std::vector<unsigned char> h_motion;   // ... and the host copy they are uploaded from
    gbl_buf motion_deform;    // gbl_render_motion_deform's per-mesh table, then the deformed meshes' previous positions (motion_stage.h) ...
    std::vector<unsigned char> h_motion_deform;   // ... and the host copy they are uploaded from
    std::map<int, float> auto_rays_per_path;   // GBL_SCHEDULE_AUTO's pilot: rays per camera path by 2 * max_ray_depth + russian_roulette (gbl_render)
    double build_ms = 0.0;    // pack_scene + BVH construction + node / triangle upload
    // what gbl_update_camera and gbl_film_accumulate need to pack a camera (scene_prep.h pack_camera)
    gbl_camera h_camera;      // the description last set: gbl_create's at first (gbl_get_camera)
    gbl_film h_film;
    gbl_render_setting h_setting;   // gbl_create's render_setting block: its bssrdf_sample_num sizes a replay record (gbl_radiance_rays)
    int32_t scene_extended = 0;   // DevScene::extended without the camera's part
    // what gbl_update_instances needs to rebuild the TLAS
    std::vector<gbl_instance> h_instances;
    std::vector<uint32_t> h_light_slots;   // DevLight::wh_n per light (the Whitted quota, host copy for the stream sampler's layout)
    std::vector<gbl_mesh> h_meshes;
    std::vector<gbl_material> h_materials;
    std::vector<float> mesh_lo, mesh_hi;
    std::vector<int32_t> mesh_root;
    int32_t tlas_base = 0;
    uint32_t tlas_capacity = 0;
    int blas_depth = 0;
    std::vector<int> mesh_stack_need;   // scene_prep.h PackedScene::mesh_stack_need
    bool has_directional = false;
    // what gbl_update_vertices needs to refit a mesh's BLAS (api_geometry.hip)
    std::vector<float> h_positions;          // 3 per vertex: gbl_create's at first, the edited ones after (gbl_get_vertices)
    std::vector<uint32_t> h_indices;         // 3 per triangle, mesh-local
    std::vector<uint32_t> mesh_tri_first;    // per mesh: its first record of `tris` (triangle meshes; either builder)
    std::vector<unsigned char> mesh_emits;   // per mesh: an area light emits from it
    uint64_t num_nodes = 0;                  // records of the node array
    std::vector<DevNode> h_nodes;            // the node array as downloaded at the first vertex edit: the plans read its child references
    struct MeshRefit {
        bool built = false;
        std::vector<uint32_t> level_first;   // scene_refit.h RefitPlan::level_first
        uint32_t leaves = 0;                 // leaf slots of the plan's nodes; 1 when the root itself is a leaf (gbl_mesh_tree_stats)
        RefitRecord* plan = nullptr;         // device: the plan's records ...
        RefitBox* node_box = nullptr;        // ... and a box per record
    };
    std::vector<MeshRefit> refit;            // per mesh, built at its first edit
    // what the device-pointer entries add (gbl_update_vertices_device, gbl_render_motion_deform_device; kernels/vertices.h)
    std::vector<unsigned char> mirror_stale;    // per mesh: the device positions are newer than the mesh's slice of h_positions (refresh_mirror)
    std::vector<unsigned char> order_pending;   // per mesh: its tri_order slice waits for its first reader (make_pending_orders)
    uint32_t orders_pending = 0;                // ... how many are set
    gbl_buf vertex_words;     // six 64-bit keys and the check word (64 bytes, all ones before a call's launches), then the bound's six floats
    gbl_buf pose_words;       // gbl_render_motion_deform_device: per listed mesh a check word, a differs flag and its PoseList record
    // what gbl_rebuild_mesh and gbl_mesh_tree_stats keep (api_geometry.hip)
    gbl_buf lbvh_scratch;                    // gbl_build_blas_device's scratch, one allocation carved up per build (kernels_aux.hip)
    std::vector<int32_t> rebuild_slot;       // per mesh: the first of the tri_count node records its rebuilt trees are written to; -1: none yet
    std::vector<uint32_t*> rebuild_idx;      // per mesh: its slice of h_indices on the device, uploaded at its first rebuild
    gbl_buf tree_stats;                      // three sums (root, node and triangle area), then two partial sums per workgroup (kernels/treestats.h)
    // what the device-pointer instance entries keep (api_instances.hip, kernels/instances.h)
    gbl_trs* d_trs = nullptr;                // the raw transforms per instance on the device: made from h_instances at the first device edit or
                                             // gbl_get_instances_device, written by every instance edit after that
    uint32_t trs_stale_first = 0, trs_stale_end = 0;   // h_instances[first .. end).to_world is older than d_trs (refresh_instance_mirror)
    float* d_mesh_bounds = nullptr;          // mesh_lo / mesh_hi on the device, 6 floats per mesh ...
    std::vector<float> mesh_bounds_sent;     // ... and the values last uploaded: a vertex edit or a rebuild changes mesh_lo / mesh_hi, the next
                                             // device instance edit sees the difference and uploads again
    gbl_buf inst_stage;                      // the refusal word, the edited instances' staged records and bounds, the merged bounds of a device TLAS
    std::vector<DevInstance> need_instances; // shape and mesh per instance (transform edits change neither): what scene_stack_entries reads
    // what gbl_trace_rays keeps (api_query.hip, kernels/query.h)
    uint32_t* d_mesh_tri_offset = nullptr;   // gbl_mesh::tri_offset per mesh on the device, made at the first query: a hit's primitive number
    gbl_buf query_spill;                     // the query kernels' stack levels beyond LDS, one column per thread of the largest grid
    std::map<std::pair<const void*, size_t>, int> query_occupancy;   // resident workgroups per CU by (kernel, dynamic LDS bytes), asked once each
    gbl_buf query_any;                       // a transmittance query of a scene without masks: the any-hit bytes it is rewritten from
    // what gbl_update_lights needs to pack the light tables again (api_lights.hip, scene_prep.h repack_lights)
    std::vector<gbl_light> h_lights;         // the description last set: gbl_create's at first (gbl_get_lights)
    std::vector<DevLight> h_dev_lights;      // the device's light records, light_cdf and light_pick_pdf as last queued ...
    std::vector<float> h_light_power, h_light_cdf, h_light_pick_pdf;   // ... and the powers the two distributions are made of
    float bound_lo[3] = {}, bound_hi[3] = {};   // gbl_create's scene bound: read for a directional light's power only, and every edit that
                                             // could change the bound is refused in a scene with such a light
    std::vector<std::vector<uint32_t>> light_instances;   // per light: the instances whose area_light names it
    // ... and its pinned staging: kLightSlots copies of the three tables, each with the event of the upload that last read it
    static const int kLightSlots = 4;
    unsigned char* light_stage = nullptr;
    hipEvent_t light_ev[4] = {};
    unsigned light_edits = 0;
    // what gbl_update_materials* and gbl_update_textures* keep beside h_materials (api_materials.hip, scene_prep.h repack_materials /
    // repack_textures, kernels/materials.h)
    std::vector<gbl_texture> h_textures;     // the description last set: gbl_create's at first (gbl_get_textures)
    std::vector<DevMaterial> mat_records;    // what repack_materials / repack_textures pack into: only the records an edit has just
    std::vector<DevTexture> tex_records;     // packed are read, the others may be older than the device's (a device edit writes none)
    struct EditTable {                       // per table (0 materials, 1 textures):
        unsigned char* stage = nullptr;      // pinned staging, kLightSlots copies of the table's records and raw rows ...
        hipEvent_t ev[4] = {};               // ... each with the event of the upload that last read it
        unsigned edits = 0;
        float* d_rows = nullptr;             // the raw rows (materials_args.h) per record on the device: made from the host copy at the
                                             // first device edit, written by every edit after that
        std::vector<float> h_rows;           // ... that first upload's source
        hipEvent_t rows_uploaded = nullptr;  // ... recorded behind it: an edit on another stream waits for it
        uint32_t stale_first = 0, stale_end = 0;   // the host description of [first .. end) is older than d_rows (refresh_table_mirror)
    };
    EditTable mat_edit, tex_edit;
    bool has_images = false;     // the scene holds MIP pyramids (image textures / image based lights)
    // what gbl_update_image* needs to build an image's pyramid again (api_images.hip, kernels/pyramid.h)
    std::vector<gbl_image> h_images;         // gbl_create's records: an edit changes texels only (gbl_get_image)
    struct ImageTaps {                       // per image, built at its first edit: resizeImage's taps of every level >= 1 ...
        bool built = false;
        std::vector<uint32_t> h_words;       // ... on the host: per level s_weight, t_weight (floats), s_index, t_index (int32) ...
        uint32_t* d_words = nullptr;         // ... and on the device, uploaded once on the first edit's stream
        hipEvent_t uploaded = nullptr;       // ... recorded behind that upload: an edit on another stream waits for it
        struct Level { uint32_t s_weight, t_weight, s_index, t_index; int32_t n; };   // offsets into the words
        std::vector<Level> levels;           // [l - 1] for level l
    };
    std::vector<ImageTaps> image_taps;
    // what gbl_update_environment* needs to make an image based light's tables again (api_environment.hip, kernels/environment.h)
    struct Environment {                     // per light, built at an image based light's first edit: sin(theta) per row of its
        bool built = false;                  // distribution (scene_prep.h ibl_sin_theta) ...
        std::vector<float> h_sin_theta;      // ... on the host, the upload's source ...
        float* d_sin_theta = nullptr;        // ... and on the device, uploaded once on the first edit's stream
        hipEvent_t uploaded = nullptr;       // ... recorded behind that upload: an edit on another stream waits for it
        hipEvent_t power_read = nullptr;     // recorded behind the last edit's copy of the light's new power into env_pinned
        bool power_pending = false;          // h_light_power's entry is older than the device's (settle_environment_power)
    };
    std::vector<Environment> environment;
    float* d_light_power = nullptr;          // the lights' powers on the device, made from h_light_power at the first environment edit and
                                             // kept by every environment edit (its kernel) and light edit (an upload) after that
    float* env_pinned = nullptr;             // pinned, 2 floats per light: that first upload's source, then the powers read back
    hipEvent_t env_power_uploaded = nullptr; // recorded behind d_light_power's first upload
    uint32_t* wf_host_flags = nullptr;   // pinned
    // ring of event triples for gbl_get_timings
    static const int kTimingRing = 64;
    hipEvent_t t_ev[64][3] = {};
    unsigned long long t_calls = 0;
};

#define HIP_TRY(ctx, expr)                                                                     \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) {                                                                \
            (ctx)->error = std::string(#expr) + ": " + hipGetErrorString(e_);                  \
            return GBL_ERR_DEVICE;                                                             \
        }                                                                                      \
    } while (0)

// ---- kernel table ----------------------------------------------------------------------------------------------
typedef void (*gbl_render_kernel)(DevScene, RenderArgs);
typedef void (*gbl_wf_kernel)(DevScene, RenderArgs, WfArgs);
typedef void (*gbl_li_kernel)(DevScene, RenderArgs, float4*);
typedef void (*gbl_aov_kernel)(DevScene, RenderArgs, AovArgs);
typedef void (*gbl_motion_kernel)(DevScene, MotionArgs);
typedef void (*gbl_query_kernel)(DevScene, QueryArgs);
typedef void (*gbl_query_filtered_kernel)(DevScene, FilteredQueryArgs);
typedef void (*gbl_radiance_kernel)(DevScene, RadianceArgs);

// kernels_path.hip: the persistent megakernel and the AO kernel (kernels/render_kernels.h), native / replay samplers
gbl_render_kernel gbl_kernel_path(bool replay, bool stats, bool ext, bool exact_ties = false);
gbl_render_kernel gbl_kernel_ao(bool replay, bool stats, bool ext, bool exact_ties = false);
// kernels_quad.hip: the megakernel whose sparse interior steps put four lanes on each ray (kernels/quadtrace.h)
gbl_render_kernel gbl_kernel_path_quad(bool exact_ties);
gbl_render_kernel gbl_kernel_path_quad_primary(bool exact_ties);   // ... its paths starting at RenderArgs::prim_hit (primary_kernel's output)
gbl_render_kernel gbl_kernel_path_stream_quad(void);
gbl_render_kernel gbl_kernel_ao_quad(bool exact_ties);
void gbl_launch_primary(const DevScene& sc, const RenderArgs& ra, bool exact_ties, float4* prim_hit, int32_t* prim_inst, unsigned blocks, hipStream_t stream);   // kernels/packet.h
uint32_t gbl_quad_lds_words(void);          // LDS words of the quads' records, in the film tile's place
bool gbl_quad_wave_units(void);             // the quad path kernels take wave-owned work units (not in a -DGBL_WG_ITEMS build)
// kernels_stream.hip: the same two under GBL_SAMPLES_STREAM (kernels/stream.h)
gbl_render_kernel gbl_kernel_path_stream(bool stats, bool ext);
gbl_render_kernel gbl_kernel_ao_stream(bool ext);
// kernels_wavefront.hip (kernels/wavefront.h)
gbl_wf_kernel gbl_kernel_wf_trace(bool any, bool stats, bool ext, bool masks, bool ties);
gbl_wf_kernel gbl_kernel_wf_shade(bool replay, bool stats, bool ext);
gbl_wf_kernel gbl_kernel_wf_splat(bool replay, bool stats);
// kernels_whitted.hip (kernels/whitted.h)
gbl_li_kernel gbl_kernel_whitted(bool replay);
gbl_li_kernel gbl_kernel_whitted_stream(void);
// kernels_aux.hip: first-hit passes (kernels/subsurface.h, kernels/volume.h), film resolve, device BLAS build, self tests
gbl_li_kernel gbl_kernel_sss(bool replay);
gbl_render_kernel gbl_kernel_vol(bool replay);
void gbl_launch_vol_combine(float4* li, const float4* vol, uint64_t n, hipStream_t stream);
void gbl_launch_tri_bounds_gather(const DevTri* tris, const DevTriBound* by_id, DevTriBound* out, uint32_t n);
void gbl_launch_film_resolve(const float* accum, float* rgb, int n, hipStream_t stream);
// ... and the passes of gbl_film_develop (kernels/develop.h)
void gbl_launch_develop_resolve(const float* accum, float* rgb1, int n, hipStream_t stream);
void gbl_launch_bloom_filter(float* filter, int fw, int fwx, int fwy, hipStream_t stream);
void gbl_launch_bloom(const float* rgb1, const float* filter, float* out, int width, int height, int fw, int fwx, float weight, hipStream_t stream);
void gbl_launch_tone_map(float* rgb, float* logs, float* inv, int n, hipStream_t stream);
void gbl_launch_quantize(const float* rgb, uint8_t* rgb8, int n, hipStream_t stream);
// kernels_aov.hip: the first-hit feature pass of gbl_render_aov (kernels/aov.h), one lane per camera sample or, for the lean
// scenes under the native sampler, one packet per pixel; and the depth film's resolve
gbl_aov_kernel gbl_kernel_aov(bool replay, bool stats, bool ext, bool exact_ties);
gbl_aov_kernel gbl_kernel_aov_packet(bool exact_ties);
void gbl_launch_aov_resolve_depth(const float* accum, float* depth, float* coverage, int n, hipStream_t stream);
// kernels_denoise.hip: gbl_film_variance and the passes of gbl_film_denoise (kernels/denoise.h)
void gbl_launch_film_variance(const float* li, float* variance, const int32_t window[4], int spp, int width, int height, hipStream_t stream);
void gbl_launch_denoise_prepare(const float* film, const float* variance, const float* albedo, const float* normal, const float* depth, float4* cv,
                                float4* nz, float4* af, int n, uint32_t demodulate, hipStream_t stream);
size_t gbl_denoise_lds_bytes(int stride);   // of the staging level kernel; 0 where a workgroup cannot have that much
hipError_t gbl_launch_denoise_level(bool lds, const float4* cv_in, const float4* nz, const float4* af, float4* cv_out, const DenoiseArgs& a, hipStream_t stream,
                                    bool* lds_allowed);
void gbl_launch_denoise_finish(const float4* cv, const float4* af, float* film_out, int n, uint32_t demodulate, hipStream_t stream);
// kernels_temporal.hip: the passes of gbl_film_accumulate (kernels/temporal.h)
void gbl_launch_temporal_prepare(const float* film, const float* variance, const float* normal, const float* depth, float4* cl, float4* nz, uint32_t* fl,
                                 int n, hipStream_t stream);
void gbl_launch_temporal_accumulate(bool spatial, const float4* cl, const float4* nz, const uint32_t* fl, const float* variance, const float* history_in,
                                    float* history_out, float* film_out, float* variance_out, const TemporalArgs& a, hipStream_t stream);
// kernels_motion.hip: gbl_render_motion's kernels (kernels/motion.h) -- the packet kernel, or one ray per lane, lean or EXT -- and
// gbl_film_accumulate_motion's accumulate pass (kernels/temporal.h with the reprojection read from the motion planes).
// deform: the flavours of gbl_render_motion_deform that follow a deformed mesh's hit through its previous pose
gbl_motion_kernel gbl_kernel_motion(bool packet, bool ext, bool deform = false);
void gbl_launch_temporal_accumulate_motion(bool spatial, const float4* cl, const float4* nz, const uint32_t* fl, const float* variance,
                                           const float* history_in, float* history_out, float* film_out, float* variance_out, const float* motion,
                                           const TemporalArgs& a, hipStream_t stream);
// kernels_query.hip: gbl_trace_rays' kernels (kernels/query.h) -- any-hit or closest-hit, lean or EXT, with or without the tie rule,
// with or without the shading normal (closest-hit only: nullptr for any && normal).  gbl_query_plain: the unit was built as the
// one-ray-per-lane measurement form (-DGBL_QUERY_PLAIN), which takes the whole stack in LDS and no hot prefix.
gbl_query_kernel gbl_kernel_query(bool any, bool ext, bool ties, bool normal);
bool gbl_query_plain(void);
// kernels_query_filtered.hip: gbl_trace_rays_filtered's kernels (kernels/query_filtered.h), EXT builds all -- closest-hit (with or
// without the normal), any-hit or transmittance, each with or without the tie rule (nullptr for the normal with anything but
// closest-hit) -- and the two fills that answer a scene without masks
gbl_query_filtered_kernel gbl_kernel_query_filtered(uint32_t kind, bool ties, bool normal);
void gbl_launch_query_fill_miss(float4* hits, uint32_t n, hipStream_t stream);
void gbl_launch_query_any_to_transmittance(const uint8_t* occluded, float4* out, uint32_t n, hipStream_t stream);
// kernels_radiance.hip: gbl_radiance_rays' kernels (kernels/radiance.h) -- native or replay draws, lean or EXT; exact_ties picks the
// lean native build with the tie rule (the replay and EXT builds follow it always)
gbl_radiance_kernel gbl_kernel_radiance(bool replay, bool ext, bool exact_ties);
// kernels_pyramid.hip: one level of an edited image's MIP pyramid from the level above it (kernels/pyramid.h)
void gbl_launch_pyramid_level(const PyramidArgs& a, hipStream_t stream);
// kernels_environment.hip: an image based light's distribution, power and the pick distribution from its image's pyramid
// (kernels/environment.h).  parts: 2 func and the rows' CDFs, 4 the tail (api_environment.hip parts_asked)
void gbl_launch_environment(const EnvironmentArgs& a, unsigned parts, hipStream_t stream);
// kernels_materials.hip: gbl_update_materials_device / gbl_update_textures_device (kernels/materials.h), one lane per edited record
void gbl_launch_mat_compose(const MatComposeArgs& a, hipStream_t stream);
void gbl_launch_tex_compose(const TexComposeArgs& a, hipStream_t stream);
// kernels_refit.hip: the passes of gbl_update_vertices (kernels/refit.h)
void gbl_launch_refit_tris(DevTri* tris, DevTriBound* bounds, const DevTriShade* tri_shade, const float* pos, uint32_t num_vertices, uint32_t first,
                           uint32_t count, hipStream_t stream);
void gbl_launch_refit_level(DevNode* nodes, const DevTriBound* bounds, const RefitRecord* plan, RefitBox* node_box, uint32_t begin, uint32_t end,
                            hipStream_t stream);
// ... and of gbl_mesh_tree_stats (kernels/treestats.h): sums[0..3) = {root_area, node_area, tri_area}, partial holds two
// doubles per workgroup of GBL_BLOCK plan records
void gbl_launch_tree_stats(const DevNode* nodes, uint64_t num_nodes, const RefitRecord* plan, uint32_t num_records, double* sums, double* partial,
                           hipStream_t stream);
// kernels_vertices.hip: the passes of the device-pointer vertex entries (kernels/vertices.h).  first_bad, keys and differs are
// set by the caller before the launch (all ones, all ones, zero); `list` holds num_listed PoseList records on the device
void gbl_launch_vertices_check(const float* positions, const float* normals, uint32_t n, uint32_t* first_bad, hipStream_t stream);
void gbl_launch_mesh_bound(const float* positions, uint32_t vertex_count, unsigned long long* keys, float* bound, hipStream_t stream);
void gbl_launch_pose_differs(const PoseList* list, uint32_t num_listed, uint32_t max_floats, const float* positions, uint32_t num_floats_total, uint32_t* differs,
                             hipStream_t stream);
// kernels_instances.hip: the passes of the device-pointer instance entries (kernels/instances.h).  *refusal is all ones before the
// launch; the staged records are written for the instances that are not refused.  gbl_build_tlas_device builds the TLAS over n >= 2
// instance boxes into the context's builder scratch (ctx->lbvh_scratch) and writes nothing of the scene.
void gbl_launch_inst_compose(const gbl_trs* d_trs, uint32_t first, uint32_t count, const DevInstance* live, const float* mesh_bounds, uint32_t num_meshes,
                             bool refuse_box, DevInstance* out_inst, DevInstanceBound* out_bound, unsigned long long* refusal, hipStream_t stream);
gbl_status gbl_build_tlas_device(gbl_ctx* ctx, const DevInstanceBound* d_bounds, uint32_t n, int32_t tlas_base, uint32_t capacity, const DevNode** d_nodes_out,
                                 uint32_t* nodes_out, int* depth_out);
gbl_status gbl_build_blas_device(gbl_ctx* ctx, const float* d_pos, const uint32_t* d_idx, uint32_t n, const float* lo, const float* hi,
                                 DevNode* d_nodes, int32_t node_base, DevTri* d_tris, uint32_t tri_base, uint32_t shade_base, uint32_t tri_flags,
                                 int32_t* root_out, uint32_t* nodes_out, int* depth_out);   // (its scratch is ctx->lbvh_scratch, grown on demand)
