// Internal to libgoblin_hip.so, host side only: what the units behind the C ABI (api_context.hip, api_render.hip, api_aov.hip,
// api_film.hip, api_motion.hip, api_geometry.hip, api_instances.hip, api_lights.hip, api_query.hip, api_radiance.hip, api_images.hip, api_environment.hip, api_materials.hip) share.  No kernel header is needed to read it.
#pragma once
#include <chrono>
#include <cstdlib>
#include <string>
#include <utility>

#include "abi_guard.h"
#include "gbl_internal.h"

// Sets the context's error text and returns the status (api_context.hip)
gbl_status fail(gbl_ctx* ctx, gbl_status st, std::string what);

// Device memory that lives as long as the context (gbl_destroy frees ctx->allocations): GBL_ERR_OOM when the device is out of
// memory, GBL_ERR_DEVICE for any other failure, the error text naming `what`.  device_free gives it back sooner (api_context.hip)
gbl_status device_alloc(gbl_ctx* ctx, size_t bytes, const char* what, void** out);
void device_free(gbl_ctx* ctx, void* p);

// Grow a device buffer of the context to at least `bytes`; what it held is not kept (api_context.hip)
gbl_status grow(gbl_ctx* ctx, gbl_buf& b, uint64_t bytes, const char* what);

// GBL_PROBE is set: asked at every probe line and never kept, tests and tools set the variable between calls
inline bool probing() { return getenv("GBL_PROBE") != nullptr; }

// The clock of the probe lines' phases and of build_ms: the milliseconds since the last lap, or since it was made
struct LapClock {
    std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now();
    double lap_ms() {
        const std::chrono::steady_clock::time_point then = std::exchange(last, std::chrono::steady_clock::now());
        return std::chrono::duration<double, std::milli>(last - then).count();
    }
};

// GBL_ERR_UNSUPPORTED with "`who`: a directional or image based light's power ..." in a scene with a light sized by the scene
// bound, GBL_OK otherwise: what every edit that can move the bound asks first.  (api_instances.hip)
gbl_status refuse_scene_bound_edit(gbl_ctx* ctx, const char* who);
// Instances which[0 .. count) take to_world[0 .. count), the tail of every scene edit: the host mirror refreshed, build_tlas over
// the edited list with the context's mesh bounds and roots, records, bounds and TLAS uploaded into their reserved regions behind
// a device synchronisation, commit_tlas, the raw transform table where the context has one.  `who` starts the error messages; a
// refusal (build_tlas's, or a TLAS beyond the reserved nodes) leaves the context untouched.  It makes none of its own:
// gbl_update_instances keeps an instance that carries an area light out of it, gbl_update_lights moves exactly those.
// retlas_after_geometry_edit moves none -- a mesh's bound or root has changed -- and waits for the uploads.  (api_instances.hip)
gbl_status move_instances(gbl_ctx* ctx, const uint32_t* which, uint32_t count, const gbl_trs* to_world, const char* who);
gbl_status retlas_after_geometry_edit(gbl_ctx* ctx, const char* who);
// A new TLAS stands in the node array: what the kernels and gbl_info read of it, and the AUTO pilot's reset.  (api_instances.hip)
void commit_tlas(gbl_ctx* ctx, int32_t root, int depth, size_t nodes, int stack_entries);

// The tie order of every mesh a deferred device edit left pending (gbl_update_vertices_device with GBL_VERTICES_DEFER_ORDER):
// mirror refreshed, mesh_reference_order on the host, the mesh's tri_order slice uploaded, behind a device synchronisation.
// Every entry point calls it where it has chosen a kernel compiled with the tie rule, before it queues anything, and no
// other: a lean launch leaves the orders pending.  Nothing to do (and nothing synchronised) when none is.  (api_geometry.hip)
gbl_status make_pending_orders(gbl_ctx* ctx);
inline gbl_status make_orders_if(gbl_ctx* ctx, bool follows_ties) { return follows_ties && ctx->orders_pending > 0 ? make_pending_orders(ctx) : GBL_OK; }

// The mesh's slice of h_positions brought up to the device's, if a device edit left it stale: one device-to-host copy.  The
// caller has synchronised the device or knows it idle.  (api_geometry.hip)
gbl_status refresh_mirror(gbl_ctx* ctx, uint32_t mesh);

// h_instances' transforms brought up to the device's raw table, if a device instance edit left a range of them stale: one
// device-to-host copy of that range (it waits for the device).  Every reader of h_instances[i].to_world calls it first:
// gbl_get_instances, gbl_update_instances, the TLAS tail of the geometry edits, gbl_render_motion*.  (api_instances.hip)
gbl_status refresh_instance_mirror(gbl_ctx* ctx);
// ... and the other direction: h_instances[first .. first + count).to_world into the raw table, if the context has one yet
// (a host instance edit after a device one).  (api_instances.hip)
gbl_status write_instance_table(gbl_ctx* ctx, uint32_t first, uint32_t count);

// GBL_OK when `p` is device or managed memory of the context's device whose allocation holds `bytes` from p on; GBL_ERR_INVALID
// with "`who`: `what` ..." otherwise, the sticky error a plain host pointer leaves cleared.  Touches no device memory.  (api_geometry.hip)
gbl_status check_device_pointer(gbl_ctx* ctx, const void* p, uint64_t bytes, const std::string& who, const char* what);

// Image `image` takes level 0 from `level0` (device memory, or the caller's pageable host memory) and the levels above it are
// launched, all on `stream`: the image's tap tables made and uploaded at its first edit, the copy, one pyramid launch per level.
// The caller has validated everything; `who` names it in an allocation failure.  (api_images.hip)
gbl_status queue_image_pyramid(gbl_ctx* ctx, uint32_t image, const float* level0, bool on_device, hipStream_t stream, const char* who);

// h_light_power, h_light_cdf and h_light_pick_pdf brought up to the device's after environment edits, whose powers are worked out
// on the device: waits for each pending 4-byte read-back's event, then packs the distribution again on the host.  Nothing to do
// (and nothing waited for) when no light's power is pending.  gbl_update_lights calls it before it packs.  (api_environment.hip)
gbl_status settle_environment_power(gbl_ctx* ctx);

// A kernel launched with more than 64 KiB of dynamic LDS has to be allowed it first
template <class K>
gbl_status allow_lds(gbl_ctx* ctx, K kernel, size_t bytes) {
    if (bytes > 64 * 1024)
        HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(bytes)));
    return GBL_OK;
}

// Two byte ranges share a byte; false when either pointer is NULL
inline bool overlaps(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a && b && a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// LDS of a workgroup's traversal stacks
inline size_t stack_lds_bytes(const DevScene& sc) { return static_cast<size_t>(sc.stack_entries) * GBL_BLOCK * sizeof(uint32_t); }

// Budget for the per-sample buffers of a call, read once per context (api_render.hip)
uint64_t li_budget_bytes(gbl_ctx* ctx);

// Which camera samples a call draws, worked out by plan_samples before anything is queued: what gbl_render and
// gbl_render_aov have in common
struct SamplePlan {
    RenderArgs ra;              // sample layout, window, tiling, shard, seed, replay records and the context's counters; the rest zero
    uint64_t npix = 0;          // pixels of the window
    uint64_t entries = 0;       // ... times spp: the camera samples of the window, the per-sample buffers' length
    int total_tiles = 0;
    bool replay = false;        // the kernels read sample records: replay and stream
    bool want_stats = false;    // collect_stats: instrumented builds
};

// Checks the integrator, sample counts, window, sample mode and shard of a call, in the order gbl_render always met them (a
// call failing several gets the first one's status), and fills the plan.  gbl_render also checks its schedule field, between
// the sample counts and the window; gbl_render_aov ignores that field.  A shard that owns no tile leaves with
// ra.local_tiles == 0.  Nothing is launched or allocated.  (api_render.hip)
gbl_status plan_samples(gbl_ctx* ctx, const gbl_render_params* p, bool check_schedule, SamplePlan* pl);

// The sample quota of a camera sample of `p`'s integrator: ra.spp / root, max_depth, the replay record's dims and off2_base and the
// BSSRDF block's offsets.  RenderArgs::seed_key of a caller's seed.  gbl_radiance_rays takes both as gbl_render does.  (api_render.hip)
void sample_layout(const DevScene& sc, const gbl_render_params* p, RenderArgs& ra);
uint32_t native_seed_key(uint64_t seed);

// The buffers of a query call with n > 0 rays: null pointers, 2^32 rays or more, memory that is not the device's or ends early, an
// output of n records of out_stride bytes that overlaps the rays.  Sets the device.  (api_query.hip)
gbl_status check_query_buffers(gbl_ctx* ctx, const std::string& who, const gbl_ray* d_rays, uint64_t n, void* d_out, uint64_t out_stride);
// A persistent ray kernel's launch: the stack backing and the LDS layout (stacks' first levels, then the top of the tree) into
// qa's stack_spill / hot_word / hot_count, the resident workgroups from the context's occupancy cache into *wgs, the LDS bytes into
// *lds.  max_workgroups: 0 for the grid the device holds.  (api_query.hip)
gbl_status persistent_layout(gbl_ctx* ctx, const void* kernel, uint64_t n, uint32_t max_workgroups, QueryArgs& qa, size_t* lds_out, uint64_t* wgs_out);

// The register-accumulating splat (kernels/wavefront.h wf_splat) of per-sample values into ra.film: samples pass_k0 ..
// pass_k0 + pass_spp of every pixel of the shard's tiles, `li` holding pass_spp values per pixel of the window.  (api_render.hip)
gbl_status launch_splat(gbl_ctx* ctx, const RenderArgs& ra, float4* li, int pass_k0, int pass_spp, bool replay, bool stats, hipStream_t stream);

// Closes a call that reports gbl_stats: the time since ev0, the shard's camera samples as `paths`, every other field zero;
// an instrumented call (want_stats) also copies the 32 device counters into `counters`, unless that is NULL.  (api_render.hip)
gbl_status close_call(gbl_ctx* ctx, const SamplePlan& pl, hipStream_t stream, gbl_stats* stats, unsigned long long* counters);
