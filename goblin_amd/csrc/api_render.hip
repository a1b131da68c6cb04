// libgoblin_hip.so -- C ABI of the device integrator (include/goblin_hip.h): the render path.
//
// gbl_render   launches the persistent render kernel over a sample sub-window and
//              accumulates into the caller's device film.
// plan_samples, launch_splat and close_call are what gbl_render_aov (api_aov.hip) shares with it.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gbl_host.h"
#include "kernels/stream.h"     // StreamLayout: the host sizes the stream sampler's scratch
#include "kernels/trace.h"      // GBL_WF_STACK_LDS

namespace {

int round_to_square(int n, int* root) {
    int s = static_cast<int>(std::ceil(std::sqrt(static_cast<float>(n))));
    *root = s;
    return s * s;
}

uint32_t host_mix(uint32_t a, uint32_t b) {   // same integer hash as kernels/sampler.h nat_mix
    uint32_t h = (a ^ 0x9E3779B9u) * 0x85EBCA6Bu;
    h ^= b + 0x7F4A7C15u + (h << 6) + (h >> 2);
    h ^= h >> 16;
    h *= 0x7FEB352Du;
    h ^= h >> 15;
    h *= 0x846CA68Bu;
    h ^= h >> 16;
    return h;
}


// ---------------------------------------------------------------------------
// Render path: environment switches, device buffers, and the wavefront schedule (host side of kernels/wavefront.h)
// ---------------------------------------------------------------------------
#ifndef GBL_WF_POOL_LOG2
#define GBL_WF_POOL_LOG2 23   // 8 Mi path slots in flight (1.9 GB of path state): 2^21 -> 2^23 is -9 % on config 3, -10 % on config 4
#endif
#ifndef GBL_WF_SHADOW_WGS
#define GBL_WF_SHADOW_WGS 1   // workgroups per CU of the concurrent shadow-ray trace launch
#endif

// The environment switches of the render path, read once per gbl_render call: the tests toggle
// some of them between renders of one process.  GBL_LI_BUDGET_MB is read once per context (li_budget_bytes).
struct RenderKnobs {
    bool mk_quad;            // GBL_MK_QUAD=0: the lean kernels of the native sampler run one ray per lane (bit-identity tests, A/B)
    bool primary;            // GBL_PRIMARY=0: the quad path kernels trace their camera rays themselves (A/B, bit-identity test)
    bool wf_overlap;         // GBL_WF_NO_OVERLAP: the wavefront's shadow and extension traces take turns on one stream
    uint32_t wf_hot;         // GBL_WF_HOT: nodes of the tree's top the wavefront trace kernels keep in LDS
    int hot_lds;             // GBL_HOT_LDS: ... and the quad kernels (measurement aid: any size; -1 = what fits)
    bool stream_tail_set;    // GBL_STREAM_TAIL: a pixel's tail in the stream sampler's scratch (tests: force the medium phase's
    uint64_t stream_tail;    // chunked walk)
    bool phase_clock;        // GBL_PHASE_CLOCK: print the phase shares of a measurement build (-DGBL_PHASE_CLOCK, tools/phase_clock.py)
    bool probe;              // GBL_PROBE: print the instrumented build's probes with collect_stats
};

RenderKnobs read_knobs() {
    RenderKnobs k;
    const char* e = getenv("GBL_MK_QUAD");
    k.mk_quad = e == nullptr || e[0] != '0';
    e = getenv("GBL_PRIMARY");
    k.primary = e == nullptr || e[0] != '0';
    k.wf_overlap = getenv("GBL_WF_NO_OVERLAP") == nullptr;
    e = getenv("GBL_WF_HOT");
    k.wf_hot = e ? static_cast<uint32_t>(std::max(0, atoi(e))) : GBL_WF_HOT_NODES;
    e = getenv("GBL_HOT_LDS");
    k.hot_lds = e ? std::max(0, atoi(e)) : -1;
    e = getenv("GBL_STREAM_TAIL");
    k.stream_tail_set = e != nullptr;
    k.stream_tail = e ? strtoull(e, nullptr, 10) : 0;
    k.phase_clock = getenv("GBL_PHASE_CLOCK") != nullptr;
    k.probe = probing();
    return k;
}

// What one gbl_render call does, worked out by plan_render (and choose_schedule) before anything is queued
struct Plan : SamplePlan {
    uint64_t call_paths = 0;    // camera samples of this rank's shard (AUTO goes by them)
    uint64_t n_items = 0;       // the megakernel's work items: the shard's tiles x chunks of their samples
    bool stream_mode = false;   // GBL_SAMPLES_STREAM
    bool whitted = false;
    size_t lds = 0;             // dynamic LDS of the one-ray-per-lane megakernel ...
    int per_cu = 1;             // ... and the workgroups per CU it leaves room for
    bool defer = false;         // megakernel: per-sample radiance kept and splatted afterwards
    StreamLayout layout;        // GBL_SAMPLES_STREAM: the sample quota of a pixel
    bool wavefront = false;     // choose_schedule
    int pass_spp = 0;           // ... wavefront: samples per pixel of one pass
    // choose_flavours: which builds the call launches, decided once
    bool vol_pass = false, sss_pass = false;   // the first-hit passes (first_hit_passes)
    bool lean_native = false;   // the integrator's kernels are the native sampler's lean builds: no tie rule (trace.h)
    bool follows_ties = false;  // some kernel of the call is compiled with the tie rule and reads tri_order (make_orders_if)
};

// LDS of the film tile the splat accumulates into
size_t tile_lds_bytes(const DevScene& sc) {
    const int tp = GBL_TILE + 2 * sc.film.halo;
    return sizeof(float) * (4 * tp * tp + 256);
}

gbl_status wf_ensure_pool(gbl_ctx* ctx) {
    if (ctx->wf_pool) return GBL_OK;
    const uint32_t pool = 1u << GBL_WF_POOL_LOG2;   // path slots (~160 B each)
    WfArgs& w = ctx->wf;
    memset(&w, 0, sizeof(w));
    gbl_status st;
#define WF_A(field, n) \
    if ((st = device_alloc(ctx, (n) * sizeof(*w.field), "wavefront pool", reinterpret_cast<void**>(&w.field))) != GBL_OK) return st
    WF_A(ray_o, pool); WF_A(ray_d, pool); WF_A(hit, pool); WF_A(hit_inst, pool);
    WF_A(s_thr, pool); WF_A(s_li, pool); WF_A(s_ld, pool); WF_A(s_f, pool); WF_A(s_id, pool); WF_A(s_vis, pool);
    WF_A(ext_q, pool); WF_A(ext_count, pool / 64);
    WF_A(sh_d, pool); WF_A(sh_slot, pool); WF_A(sh_count, pool / 64);
    WF_A(live_flags, 8);
    WF_A(wave_next, 2 * (pool / 64)); WF_A(steal_next, 1);
    if (ctx->scene.has_masks) {   // see WfArgs
        WF_A(hit2, pool); WF_A(hit2_inst, pool); WF_A(mis_tr, pool); WF_A(sh_f, pool); WF_A(sh_L, pool); WF_A(sh_c, pool);
    }
#undef WF_A
    if (hipHostMalloc(reinterpret_cast<void**>(&ctx->wf_host_flags), 8 * sizeof(uint32_t)) != hipSuccess) {
        ctx->error = "hipHostMalloc(wavefront flags) failed";
        return GBL_ERR_OOM;
    }
    ctx->wf_pool = pool;
    return GBL_OK;
}

// Random numbers one camera sample's transmittance + Lv may draw (GBL_SAMPLES_STREAM sizes a pixel's tail with it): 9 per light
// sample and the pick for the homogeneous region; for a heterogeneous one the jitters and up to 5 per point of the march,
// whose length is bounded by the region's longest world-space diagonal over the step (kernels/render_kernels.h
// stream_medium_phase) -- plus room for the generator state that phase sets aside.
static uint64_t medium_draws_per_sample(const DevScene& sc) {
    if (sc.volume.on == 0u) return 0;
    if (sc.volume.hetero == 0u) return 9ull * static_cast<uint64_t>(std::max(0, sc.volume.sample_num)) + 1;
    const DevVolume& v = sc.volume;
    double diag = 0.0;
    for (int s = 0; s < 4; ++s) {
        const double e[3] = {double(v.hi[0] - v.lo[0]), (s & 1 ? -1.0 : 1.0) * double(v.hi[1] - v.lo[1]), (s & 2 ? -1.0 : 1.0) * double(v.hi[2] - v.lo[2])};
        double w[3];
        for (int r = 0; r < 3; ++r) w[r] = v.m[4 * r] * e[0] + v.m[4 * r + 1] * e[1] + v.m[4 * r + 2] * e[2];
        diag = std::max(diag, std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]));
    }
    const double steps = std::floor(diag / std::max(1e-6, double(v.step))) + 3.0;
    return 2ull + 5ull * static_cast<uint64_t>(std::min(steps, 1.0e6)) + 700ull;
}
// GBL_STREAM_TAIL: the tail per sample the knob asks for, raised to the least with which stream_medium_phase can still walk a
// pixel's S samples one per chunk.  Homogeneous: one sample's draws.  Heterogeneous: a sample's share of ONE sample's budget --
// that budget already holds the generator state's room, which the phase takes off the pixel's whole tail, not off every
// sample's, so S times the budget (what the knob used to be raised to) left no pixel with more than one chunk.
static uint32_t knob_stream_tail(const DevScene& sc, uint64_t knob, uint32_t S) {
    const uint64_t med = medium_draws_per_sample(sc);
    const uint64_t least = sc.volume.hetero != 0u ? (med + S - 1) / std::max(1u, S) : med;
    return static_cast<uint32_t>(std::max<uint64_t>(least, knob));
}

// Stack levels of the wavefront trace kernels beyond the LDS part: one column per thread of the largest persistent
// trace grid (8 workgroups per CU).  Re-made when an instance edit deepens the TLAS.
gbl_status wf_ensure_spill(gbl_ctx* ctx) {
    const int deep = ctx->scene.stack_entries > GBL_WF_STACK_LDS ? ctx->scene.stack_entries - GBL_WF_STACK_LDS : 1;
    const uint64_t level_bytes = static_cast<uint64_t>(ctx->num_cus) * 8 * GBL_BLOCK * sizeof(uint32_t);
    gbl_status st = grow(ctx, ctx->wf_spill, static_cast<uint64_t>(deep) * level_bytes, "trace stack backing");
    if (st != GBL_OK) return st;
    ctx->wf_spill_levels = static_cast<int>(ctx->wf_spill.bytes / level_bytes);
    return GBL_OK;
}

// GBL_SAMPLES_STREAM: per-workgroup sample-generation scratch and the per-sample image positions the splat reads
gbl_status ensure_stream_buffers(gbl_ctx* ctx, uint64_t words_per_wg, uint64_t workgroups, uint64_t samples, RenderArgs* ra) {
    ra->stream_stride = words_per_wg;
    gbl_status st = grow(ctx, ctx->stream_scratch, words_per_wg * sizeof(uint32_t) * workgroups, "stream scratch");
    if (st != GBL_OK) return st;
    ra->stream_scratch = static_cast<uint32_t*>(ctx->stream_scratch.p);
    if ((st = grow(ctx, ctx->stream_xy, samples * 2 * sizeof(float), "stream image positions")) != GBL_OK) return st;
    ra->image_xy = static_cast<float*>(ctx->stream_xy.p);
    return GBL_OK;
}

// The path tracer on the wavefront schedule, in passes of pass_spp samples per pixel (choose_schedule)
gbl_status render_wavefront(gbl_ctx* ctx, const gbl_render_params* p, const Plan& pl, const RenderKnobs& knobs, hipEvent_t main_done,
                            hipStream_t stream) {
    const DevScene& sc = ctx->scene;
    const RenderArgs& ra = pl.ra;
    const bool want_stats = pl.want_stats, replay = pl.replay;
    gbl_status st = wf_ensure_pool(ctx);
    if (st != GBL_OK) return st;
    if ((st = wf_ensure_spill(ctx)) != GBL_OK) return st;
    const int pass_spp = pl.pass_spp;
    uint32_t* const spill = static_cast<uint32_t*>(ctx->wf_spill.p);
    WfArgs wa = ctx->wf;
    wa.stack_spill = spill;
    if (ra.li_out) {
        wa.li_buf = reinterpret_cast<float4*>(ra.li_out);   // single pass: li_buf is the caller's buffer, in its order
    } else {
        if ((st = grow(ctx, ctx->li, pl.npix * pass_spp * sizeof(float4), "per-sample radiance")) != GBL_OK) return st;
        wa.li_buf = static_cast<float4*>(ctx->li.p);
    }
    const uint32_t total = static_cast<uint32_t>(static_cast<uint64_t>(ra.local_tiles) * 64 * pass_spp);
    uint32_t pool = std::min<uint32_t>(ctx->wf_pool, (total + GBL_BLOCK - 1) / GBL_BLOCK * GBL_BLOCK);
    wa.pool_size = pool;
    wa.total_paths = total;
    wa.pass_spp = pass_spp;
    {   // ids are dealt in blocks of 64, round-robin over the pool/64 shade-waves
        // ... three quarters of them up front; the rest is the reserve the waves that finish early draw on (wf_shade; round 3 dealt
        // everything up front)
        const uint32_t reserve_pct = 25;
        const uint32_t waves = pool / 64, blocks = (total + 63) / 64;
        wa.static_blocks = static_cast<uint32_t>(static_cast<uint64_t>(blocks / waves) * (100 - reserve_pct) / 100);
        wa.total_blocks = blocks;
    }
    size_t lds_stack = static_cast<size_t>(std::min<int>(sc.stack_entries, GBL_WF_STACK_LDS)) * GBL_BLOCK * sizeof(uint32_t);
    // the trace kernels keep the top of the tree in LDS behind their stacks (trace.h HotSplitStack): GBL_WF_HOT nodes
    RenderArgs ra_trace = ra;
    ra_trace.hot_word = static_cast<uint32_t>(lds_stack / sizeof(uint32_t));
    ra_trace.hot_count = std::min<uint32_t>(knobs.wf_hot, sc.hot_nodes);
    lds_stack += ra_trace.hot_count * sizeof(DevNode);
    // EXT kernels carry the analytic shapes / directional light / non-pinhole cameras; plain scenes run the lean
    // build.  Instrumented launches always use the EXT build (same work, same counters).
    const bool ext = sc.extended != 0;
    const bool masks = sc.has_masks != 0;
    const bool lean_native = pl.lean_native;   // native sampler, lean build: no tie rule (choose_flavours)
    gbl_wf_kernel k_ext = gbl_kernel_wf_trace(false, want_stats, ext || masks || want_stats, masks, !lean_native);
    gbl_wf_kernel k_shd = gbl_kernel_wf_trace(true, want_stats, ext || masks || want_stats, masks, !lean_native);
    // persistent trace grids: exactly the resident workgroups (regions are assigned statically, so a
    // workgroup that has to wait for a free CU would serialise its share), never more waves than regions
    int occ_ext = 0, occ_shd = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ_ext, reinterpret_cast<const void*>(k_ext), GBL_BLOCK, lds_stack) != hipSuccess || occ_ext < 1) occ_ext = 1;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ_shd, reinterpret_cast<const void*>(k_shd), GBL_BLOCK, lds_stack) != hipSuccess || occ_shd < 1) occ_shd = 1;
    occ_ext = std::min(occ_ext, 8);   // stack_spill is sized for 8 workgroups per CU
    occ_shd = std::min(occ_shd, 8);
    // The shadow rays of iteration k and the extension rays of iteration k+1 are both known once wf_shade(k) has run
    // and do not depend on each other, so they trace CONCURRENTLY: the shadow launch goes to a second stream with
    // GBL_WF_SHADOW_WGS workgroups per CU, the extension launch keeps the rest of the occupancy (both grids are
    // persistent, so together they must not exceed what is resident).  One launch tail per iteration instead of two.
    const bool overlap = occ_ext > GBL_WF_SHADOW_WGS && knobs.wf_overlap;
    if (overlap) {
        occ_ext -= GBL_WF_SHADOW_WGS;
        occ_shd = GBL_WF_SHADOW_WGS;
        if (!ctx->wf_aux) {
            HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->wf_aux, hipStreamNonBlocking));
            HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->wf_ev_shade, hipEventDisableTiming));
            HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->wf_ev_shadow, hipEventDisableTiming));
        }
    }
    const uint64_t max_wgs = (pool / 64 + 3) / 4;
    unsigned ext_wgs = static_cast<unsigned>(std::max<uint64_t>(1, std::min<uint64_t>(static_cast<uint64_t>(ctx->num_cus) * occ_ext, max_wgs)));
    unsigned shd_wgs = static_cast<unsigned>(std::max<uint64_t>(1, std::min<uint64_t>(static_cast<uint64_t>(ctx->num_cus) * occ_shd, max_wgs)));
    // the two trace launches may run at the same time: disjoint columns of the stack backing (ext <= 7 and shd = 1
    // workgroups per CU of the 8 the backing is sized for).  Without the overlap they are serialised on one stream and
    // each may take up to 8 per CU, so they share the columns.
    uint32_t* const spill_ext = spill;
    uint32_t* const spill_shd = overlap ? spill + static_cast<size_t>(ctx->wf_spill_levels) * ext_wgs * GBL_BLOCK : spill;
    if (static_cast<uint64_t>(overlap ? ext_wgs + shd_wgs : std::max(ext_wgs, shd_wgs)) > static_cast<uint64_t>(ctx->num_cus) * 8)
        return fail(ctx, GBL_ERR_DEVICE, "wavefront trace grids exceed the stack backing");
    dim3 block(GBL_BLOCK), grid_ext(ext_wgs), grid_shd(shd_wgs), grid_shade(pool / GBL_BLOCK);
    gbl_wf_kernel k_shade = gbl_kernel_wf_shade(replay, want_stats, ext || want_stats);
    if (!k_ext || !k_shd || !k_shade) return fail(ctx, GBL_ERR_UNSUPPORTED, "wavefront kernel variant not built");
    if ((st = allow_lds(ctx, k_ext, lds_stack)) != GBL_OK || (st = allow_lds(ctx, k_shd, lds_stack)) != GBL_OK) return st;
    for (int k0 = 0; k0 < ra.spp; k0 += pass_spp) {
        wa.pass_k0 = k0;
        HIP_TRY(ctx, hipMemsetAsync(wa.wave_next, 0, 2 * (pool / 64) * sizeof(uint32_t), stream));
        HIP_TRY(ctx, hipMemsetAsync(wa.steal_next, 0, sizeof(uint32_t), stream));
        wa.init = 1;
        wa.flag_index = 7;
        hipLaunchKernelGGL(k_shade, grid_shade, block, 0, stream, sc, ra, wa);
        wa.init = 0;
        // slot s traces ceil((total - s) / pool) paths, each at least one iteration
        uint64_t iter = 0, min_iters = total / pool;
        bool done = false, shadow_pending = false;
        while (!done) {
            HIP_TRY(ctx, hipMemsetAsync(wa.live_flags, 0, 8 * sizeof(uint32_t), stream));
            int batch = iter + 4 <= min_iters ? static_cast<int>(std::min<uint64_t>(min_iters - iter, 64)) : 4;
            for (int b = 0; b < batch; ++b) {
                wa.flag_index = b & 7;
                wa.stack_spill = spill_ext;
                hipLaunchKernelGGL(k_ext, grid_ext, block, lds_stack, stream, sc, ra_trace, wa);
                if (overlap && shadow_pending) HIP_TRY(ctx, hipStreamWaitEvent(stream, ctx->wf_ev_shadow, 0));   // wf_shade reads s_ld, rewrites the shadow queue
                hipLaunchKernelGGL(k_shade, grid_shade, block, 0, stream, sc, ra, wa);
                wa.stack_spill = spill_shd;
                if (overlap) {
                    HIP_TRY(ctx, hipEventRecord(ctx->wf_ev_shade, stream));
                    HIP_TRY(ctx, hipStreamWaitEvent(ctx->wf_aux, ctx->wf_ev_shade, 0));
                    hipLaunchKernelGGL(k_shd, grid_shd, block, lds_stack, ctx->wf_aux, sc, ra_trace, wa);
                    HIP_TRY(ctx, hipEventRecord(ctx->wf_ev_shadow, ctx->wf_aux));
                    shadow_pending = true;
                } else {
                    hipLaunchKernelGGL(k_shd, grid_shd, block, lds_stack, stream, sc, ra_trace, wa);
                }
                ++iter;
            }
            if (iter >= min_iters) {
                HIP_TRY(ctx, hipMemcpyAsync(ctx->wf_host_flags, wa.live_flags, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
                HIP_TRY(ctx, hipStreamSynchronize(stream));
                if (ctx->wf_host_flags[(batch - 1) & 7] == 0) done = true;
            }
            if (iter > (1u << 20)) return fail(ctx, GBL_ERR_DEVICE, "wavefront loop did not terminate");
        }
        if (overlap && shadow_pending) HIP_TRY(ctx, hipStreamWaitEvent(stream, ctx->wf_ev_shadow, 0));   // rejoin before the pool is reused
        if ((st = launch_splat(ctx, ra, wa.li_buf, k0, pass_spp, replay, want_stats, stream)) != GBL_OK) return st;
    }
    HIP_TRY(ctx, hipEventRecord(main_done, stream));
    return GBL_OK;
}

// The first n values of libc rand() in a process that never called srand() -- what the reference seeds its per-tile
// generators with (RNGImp::RNGImp, GoblinUtils.cpp:19-20).  glibc's default is the TYPE_3 additive feedback generator
// over 31 words, r[i] = r[i-3] + r[i-31], seeded with 1 through the Park-Miller step and run 310 times before the
// first output, which drops the low bit.
std::vector<uint32_t> glibc_rand_sequence(size_t n) {
    std::vector<uint32_t> st(344 + n);
    int32_t r = 1;
    st[0] = 1u;
    for (int i = 1; i < 31; ++i) {
        const int64_t hi = r / 127773, lo = r % 127773;
        int64_t w = 16807 * lo - 2836 * hi;
        if (w < 0) w += 2147483647;
        r = static_cast<int32_t>(w);
        st[i] = static_cast<uint32_t>(r);
    }
    for (int i = 31; i < 34; ++i) st[i] = st[i - 31];
    for (size_t i = 34; i < st.size(); ++i) st[i] = st[i - 31] + st[i - 3];
    std::vector<uint32_t> out(n);
    for (size_t i = 0; i < n; ++i) out[i] = st[344 + i] >> 1;
    return out;
}

}   // namespace

// The sample quota of a camera sample: record dimensions and pattern offsets of the integrator (RenderArgs; gbl_host.h)
void sample_layout(const DevScene& sc, const gbl_render_params* p, RenderArgs& ra) {
    ra.integrator = static_cast<int32_t>(p->integrator);
    ra.spp = round_to_square(p->sample_per_pixel, &ra.root);
    ra.max_depth = p->max_ray_depth;
    int tmp;
    int ao_n = round_to_square(std::max(1, p->ao_sample_num), &tmp);
    ra.ao_n = ao_n;
    if (p->integrator == GBL_INTEGRATOR_AO) {
        int r2;
        ra.dims = 4 + 2 * round_to_square(ao_n, &r2);
        ra.off2_base = 4;
    } else {
        int r1, r2;
        int n1 = round_to_square(std::max(1, p->bssrdf_sample_num), &r1);
        int n2 = round_to_square(n1, &r2);
        ra.dims = 4 + 7 * ra.max_depth + 4 * n1 + 4 * n2;
        ra.off2_base = 4 + 3 * ra.max_depth + 4 * n1;
        ra.bssrdf_n = n1;
        ra.bssrdf_n2 = n2;
        ra.sss_off1 = static_cast<uint32_t>(4 + 3 * ra.max_depth);
        ra.sss_off2 = static_cast<uint32_t>(ra.off2_base + 4 * ra.max_depth);
        ra.sss_pat1 = 3u * static_cast<uint32_t>(ra.max_depth);
        ra.sss_pat2 = 2u * static_cast<uint32_t>(ra.max_depth);
        if (p->integrator == GBL_INTEGRATOR_WHITTED) {   // per-light patterns instead of per-bounce ones (kernels/whitted.h)
            ra.dims = 4 + 6 * sc.wh_slots + 1 + 4 * n1 + 4 * n2;
            ra.off2_base = 4 + 2 * sc.wh_slots + 1 + 4 * n1;
            ra.sss_off1 = static_cast<uint32_t>(4 + 2 * sc.wh_slots + 1);
            ra.sss_off2 = static_cast<uint32_t>(ra.off2_base + 4 * sc.wh_slots);
            ra.sss_pat1 = 2u * static_cast<uint32_t>(sc.num_lights) + 1u;   // after the per-light ls / bs patterns and pickLight
            ra.sss_pat2 = 2u * static_cast<uint32_t>(sc.num_lights);
        }
    }
}

uint32_t native_seed_key(uint64_t seed) { return host_mix(static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32)); }

// ---------------------------------------------------------------------------
// What gbl_render shares with gbl_render_aov (gbl_host.h)
// ---------------------------------------------------------------------------
// Budget for the per-sample radiance buffer: a quarter of the device's memory (72 GB of the MI355X's 288 GB), so that
// BASELINE's largest frame (config 3: 1028^2 px x 1024 spp x 16 B = 17.3 GB) is one pass.  GBL_LI_BUDGET_MB overrides it.
uint64_t li_budget_bytes(gbl_ctx* ctx) {
    if (ctx->li_budget == 0) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || total_b == 0) total_b = 8ull << 30;
        ctx->li_budget = std::max<uint64_t>(1ull << 30, static_cast<uint64_t>(total_b) / 4);
        if (const char* e = getenv("GBL_LI_BUDGET_MB")) ctx->li_budget = std::max<uint64_t>(1ull << 20, strtoull(e, nullptr, 10) << 20);
    }
    return ctx->li_budget;
}

gbl_status plan_samples(gbl_ctx* ctx, const gbl_render_params* p, bool check_schedule, SamplePlan* pl) {
    const DevScene& sc = ctx->scene;
    RenderArgs& ra = pl->ra;
    memset(&ra, 0, sizeof(ra));
    ra.unit_rows = GBL_TILE;   // work items are whole tiles (plan_wave_units: the lean quad path kernels' are not)
    if (p->integrator != GBL_INTEGRATOR_PATH && p->integrator != GBL_INTEGRATOR_AO && p->integrator != GBL_INTEGRATOR_WHITTED)
        return fail(ctx, GBL_ERR_INVALID, "unknown integrator");
    if (p->sample_per_pixel < 1 || p->max_ray_depth < 1) return fail(ctx, GBL_ERR_INVALID, "sample_per_pixel and max_ray_depth must be >= 1");
    if (check_schedule && p->schedule > GBL_SCHEDULE_WAVEFRONT) return fail(ctx, GBL_ERR_INVALID, "unknown schedule " + std::to_string(p->schedule));
    sample_layout(sc, p, ra);
    const int32_t* full = sc.film.window;
    const bool whole = p->window[0] == 0 && p->window[1] == 0 && p->window[2] == 0 && p->window[3] == 0;
    for (int i = 0; i < 4; ++i) ra.window[i] = whole ? full[i] : p->window[i];
    if (ra.window[0] < full[0] || ra.window[1] > full[1] || ra.window[2] < full[2] || ra.window[3] > full[3] ||
        ra.window[0] > ra.window[1] || ra.window[2] > ra.window[3])
        return fail(ctx, GBL_ERR_INVALID, "render window lies outside the film's sample window");
    if (p->sample_mode == GBL_SAMPLES_REPLAY && !p->replay_samples) return fail(ctx, GBL_ERR_INVALID, "replay mode needs replay_samples");
    if (p->sample_mode != GBL_SAMPLES_REPLAY && p->sample_mode != GBL_SAMPLES_NATIVE && p->sample_mode != GBL_SAMPLES_STREAM)
        return fail(ctx, GBL_ERR_INVALID, "unknown sample_mode");
    pl->npix = static_cast<uint64_t>(ra.window[1] - ra.window[0]) * (ra.window[3] - ra.window[2]);
    if (pl->npix * ra.spp >= (1ull << 32)) return fail(ctx, GBL_ERR_INVALID, "more than 2^32 camera samples in one call: split the window");
    pl->entries = pl->npix * ra.spp;
    ra.tiles_x = (ra.window[1] - ra.window[0] + GBL_TILE - 1) / GBL_TILE;
    ra.tiles_y = (ra.window[3] - ra.window[2] + GBL_TILE - 1) / GBL_TILE;
    ra.shard_count = std::max(1, p->tile_shard_count);
    ra.shard_index = p->tile_shard_count > 1 ? p->tile_shard_index : 0;
    if (ra.shard_index < 0 || ra.shard_index >= ra.shard_count) return fail(ctx, GBL_ERR_INVALID, "tile_shard_index out of range");
    pl->total_tiles = ra.tiles_x * ra.tiles_y;
    ra.local_tiles = pl->total_tiles > ra.shard_index ? (pl->total_tiles - ra.shard_index + ra.shard_count - 1) / ra.shard_count : 0;
    ra.seed_key = native_seed_key(p->seed);
    ra.replay = p->replay_samples;
    ra.work_counter = ctx->work_counter;
    ra.stats = ctx->stats;
    pl->replay = p->sample_mode != GBL_SAMPLES_NATIVE;
    pl->want_stats = p->collect_stats != 0;
    return GBL_OK;
}

gbl_status launch_splat(gbl_ctx* ctx, const RenderArgs& ra, float4* li, int pass_k0, int pass_spp, bool replay, bool stats, hipStream_t stream) {
    WfArgs wa;
    memset(&wa, 0, sizeof(wa));
    wa.li_buf = li;
    wa.pass_k0 = pass_k0;
    wa.pass_spp = pass_spp;
    gbl_wf_kernel k_splat = gbl_kernel_wf_splat(replay, stats);
    if (!k_splat) return fail(ctx, GBL_ERR_UNSUPPORTED, "splat kernel variant not built");
    hipLaunchKernelGGL(k_splat, dim3(ra.local_tiles), dim3(GBL_BLOCK), tile_lds_bytes(ctx->scene), stream, ctx->scene, ra, wa);
    HIP_TRY(ctx, hipGetLastError());
    return GBL_OK;
}

// Pixels of the window in the tiles of the call's shard
static uint64_t shard_pixels(const RenderArgs& ra, int total_tiles) {
    uint64_t n = 0;
    for (int t = ra.shard_index; t < total_tiles; t += ra.shard_count) {
        const int tx = t % ra.tiles_x, ty = t / ra.tiles_x;
        n += static_cast<uint64_t>(std::min(GBL_TILE, ra.window[1] - (ra.window[0] + GBL_TILE * tx))) *
             std::min(GBL_TILE, ra.window[3] - (ra.window[2] + GBL_TILE * ty));
    }
    return n;
}

gbl_status close_call(gbl_ctx* ctx, const SamplePlan& pl, hipStream_t stream, gbl_stats* stats, unsigned long long* counters) {
    HIP_TRY(ctx, hipEventRecord(ctx->ev1, stream));
    HIP_TRY(ctx, hipEventSynchronize(ctx->ev1));
    float ms = 0.0f;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    memset(stats, 0, sizeof(*stats));
    stats->kernel_ms = ms;
    stats->paths = shard_pixels(pl.ra, pl.total_tiles) * pl.ra.spp;
    if (pl.want_stats && counters) HIP_TRY(ctx, hipMemcpy(counters, ctx->stats, 32 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return GBL_OK;
}

namespace {

// GBL_SAMPLES_STREAM: the checks of plan_render that concern the stream sampler, its layout, and the LDS it adds
gbl_status plan_stream(gbl_ctx* ctx, const gbl_render_params* p, Plan* pl, size_t& lds) {
    const DevScene& sc = ctx->scene;
    const int32_t* full = sc.film.window;
    RenderArgs& ra = pl->ra;
    if (p->schedule == GBL_SCHEDULE_WAVEFRONT) return fail(ctx, GBL_ERR_UNSUPPORTED, "GBL_SAMPLES_STREAM runs on the megakernel schedule");
    // the tiles rendered must be tiles of the reference's own tiling of the full sample window
    if ((ra.window[0] - full[0]) % GBL_TILE != 0 || (ra.window[2] - full[2]) % GBL_TILE != 0 ||
        (ra.window[1] != full[1] && (ra.window[1] - full[0]) % GBL_TILE != 0) ||
        (ra.window[3] != full[3] && (ra.window[3] - full[2]) % GBL_TILE != 0)) {
        ctx->error = "GBL_SAMPLES_STREAM: the window must consist of whole 8x8 tiles of the full sample window";
        return GBL_ERR_INVALID;
    }
    StreamLayout& L = pl->layout;
    L = stream_layout(ra.spp, ra.root, ra.max_depth, ra.bssrdf_n, ra.bssrdf_n2, p->integrator == GBL_INTEGRATOR_AO ? ra.ao_n : 0);
    if (pl->whitted &&
        !stream_layout_whitted(L, ra.spp, ra.root, ra.bssrdf_n, ra.bssrdf_n2, sc.num_lights, [&](int i) { return ctx->h_light_slots[i]; })) {
        ctx->error = "GBL_SAMPLES_STREAM under the Whitted integrator covers up to " + std::to_string(GBL_STREAM_MAX_RUNS - 2) + " lights";
        return GBL_ERR_UNSUPPORTED;
    }
    if (static_cast<uint64_t>(sc.stack_entries) * GBL_BLOCK < L.S)
        return fail(ctx, GBL_ERR_UNSUPPORTED, "GBL_SAMPLES_STREAM: sample_per_pixel too large for the shuffle scratch");
    lds += GBL_STREAM_LDS_WORDS * sizeof(uint32_t);
    // the shuffles run one column per lane in the LDS region of the (idle) traversal stacks; widening that region to 40 KB
    // lets 40 columns of 256 samples go at once (65 columns at config 2: two rounds instead of three) and still leaves three
    // workgroups per CU.  (The Whitted kernel sizes its own: render_whitted.)
    const size_t stack_bytes = stack_lds_bytes(sc);
    const size_t want = std::max<size_t>(stack_bytes, 40 * 1024);
    if (lds - stack_bytes + want <= 52 * 1024) {
        lds += want - stack_bytes;
        ra.stream_lperm_words = static_cast<uint32_t>(want / sizeof(uint32_t));
    } else {
        ra.stream_lperm_words = static_cast<uint32_t>(stack_bytes / sizeof(uint32_t));
    }
    ra.full_tiles_x = (full[1] - full[0] + GBL_TILE - 1) / GBL_TILE;
    return GBL_OK;
}

// Checks the call's arguments and works out everything about it that needs no device work: its camera samples (plan_samples),
// the work items, the stream sampler's layout, the megakernel's LDS and whether it keeps the per-sample radiance, and every
// budget.  The checks keep the order in which the render path used to meet them, so a call failing several gets the first
// one's status.  Nothing is launched or allocated.  A call with no tiles in its shard leaves here with pl->n_items == 0.
gbl_status plan_render(gbl_ctx* ctx, const gbl_render_params* p, float* film_accum, Plan* pl) {
    const DevScene& sc = ctx->scene;
    RenderArgs& ra = pl->ra;
    gbl_status st = plan_samples(ctx, p, true, pl);
    if (st != GBL_OK) return st;
    // Work granularity: a work item is one tile x one chunk of its samples.  Start
    // at <= 64 samples per item (4096 paths) and keep halving while the launch
    // would have fewer than ~16 items per resident workgroup (tail effect),
    // down to 4 samples (256 paths) per item.
    int chunks = 1;
    while (ra.spp / chunks > 64 && ra.spp % (chunks * 2) == 0) chunks *= 2;
    const uint64_t want_items = 16ull * ctx->num_cus * 4;
    while (static_cast<uint64_t>(ra.local_tiles) * chunks < want_items && ra.spp / chunks > 4 && ra.spp % (chunks * 2) == 0)
        chunks *= 2;
    pl->stream_mode = p->sample_mode == GBL_SAMPLES_STREAM;
    if (pl->stream_mode) chunks = 1;   // a work item is a whole tile, walked pixel by pixel (kernels/stream.h)
    ra.chunks = chunks;
    ra.chunk_spp = ra.spp / chunks;
    ra.russian_roulette = p->russian_roulette;
    ra.li_out = p->li_out;
    ra.film = film_accum;
    pl->n_items = static_cast<uint64_t>(ra.local_tiles) * ra.chunks;
    if (pl->n_items == 0) return GBL_OK;
    pl->call_paths = pl->entries / static_cast<uint64_t>(ra.shard_count);
    pl->whitted = p->integrator == GBL_INTEGRATOR_WHITTED;
    size_t lds = tile_lds_bytes(sc) + 4 * sizeof(uint32_t) + stack_lds_bytes(sc);
    if (lds > 160 * 1024) return fail(ctx, GBL_ERR_UNSUPPORTED, "scene needs " + std::to_string(lds) + " bytes of LDS per workgroup (BVH too deep)");
    if (pl->stream_mode && (st = plan_stream(ctx, p, pl, lds)) != GBL_OK) return st;
    // (plan_stream turns the stream sampler away from GBL_SCHEDULE_WAVEFRONT)
    if (p->schedule == GBL_SCHEDULE_WAVEFRONT && p->integrator != GBL_INTEGRATOR_PATH)
        return fail(ctx, GBL_ERR_UNSUPPORTED, "the wavefront schedule covers the path tracer only");
    pl->lds = lds;
    pl->per_cu = std::max(1, static_cast<int>(std::min<size_t>(8, (160 * 1024) / lds)));
    if (sc.volume.on != 0u && !pl->stream_mode && pl->entries * 32 > li_budget_bytes(ctx))
        return fail(ctx, GBL_ERR_UNSUPPORTED, "a scene with a participating medium keeps 32 bytes per camera sample: render this window in smaller pieces");
    if (pl->whitted) {
        if (ra.max_depth > GBL_WHITTED_MAX_DEPTH)
            return fail(ctx, GBL_ERR_UNSUPPORTED, "max_ray_depth above " + std::to_string(GBL_WHITTED_MAX_DEPTH) + " is outside the Whitted kernel's frame stack");
        if (!ra.li_out && pl->entries * 16 > li_budget_bytes(ctx))
            return fail(ctx, GBL_ERR_UNSUPPORTED, "the Whitted integrator keeps 16 bytes per camera sample of the call: render this window in smaller pieces");
        return GBL_OK;
    }
    if (sc.has_bssrdf != 0 && p->integrator == GBL_INTEGRATOR_PATH && !pl->stream_mode && pl->entries * 16 > li_budget_bytes(ctx))
        return fail(ctx, GBL_ERR_UNSUPPORTED, "a scene with subsurface materials keeps 16 bytes per camera sample: render this window in smaller pieces");
    // Keep the per-sample radiance (16 B each) and filter it into the film with the register-accumulating splat kernel
    // afterwards, unless that buffer would not fit the budget (then the megakernel splats through its LDS tile as it goes).
    // 64.6 -> ~53 ms on the 68 M-path frame.  Both checks below can only fail under the stream sampler, which never takes
    // the wavefront: otherwise a medium's 32 bytes per sample, checked above, leave room for these 16.
    pl->defer = ra.li_out != nullptr || pl->entries * 16 <= li_budget_bytes(ctx);
    if (sc.volume.on != 0u && !pl->defer)
        return fail(ctx, GBL_ERR_UNSUPPORTED, "a scene with a participating medium needs the per-sample radiance buffer: render this window in smaller pieces");
    if (pl->stream_mode && !pl->defer)
        return fail(ctx, GBL_ERR_UNSUPPORTED, "GBL_SAMPLES_STREAM keeps 16 bytes per camera sample of the call: render this window in smaller pieces");
    return GBL_OK;
}

// The lean quad path kernels of the native sampler take their work wave by wave (render_kernels.h wave_take), so their launch
// is planned in units per resident WAVE where plan_render plans items per resident workgroup: a unit is a band of rows of a
// tile x a chunk of samples, at most 512 paths (8 per lane) -- one row of 64-sample chunks on the headline frame.  A wave no
// longer shares an item's tail with three others, so the unit is what balances the launch: measured on configs[1] 4096 /
// 2048 / 1024 / 512 / 256 / 128 paths -> 56.0 / 44.5 / 38.2 / 37.3 / 37.5 / 38.2 ms (DESIGN_HISTORY, "Wave-owned work units").  Chunks stay at <= 64
// samples as before (64 consecutive path ids of a unit are then the consecutive samples of one pixel: a wave's rays leave
// one pixel); a launch with fewer than ~16 units per resident wave halves the band down to one row first and the chunk,
// down to 4 samples, after.
void plan_wave_units(const gbl_ctx* ctx, Plan* pl) {
    RenderArgs& ra = pl->ra;
    int chunks = 1, rows = GBL_TILE;
    while (ra.spp / chunks > 64 && ra.spp % (chunks * 2) == 0) chunks *= 2;
    while (rows > 1 && GBL_TILE * rows * (ra.spp / chunks) > 512) rows /= 2;
    const uint64_t want_units = 16ull * ctx->num_cus * GBL_PT_WAVES * 4;
    while (static_cast<uint64_t>(ra.local_tiles) * chunks * (GBL_TILE / rows) < want_units) {
        if (rows > 1)
            rows /= 2;
        else if (ra.spp / chunks > 4 && ra.spp % (chunks * 2) == 0)
            chunks *= 2;
        else
            break;
    }
    ra.chunks = chunks;
    ra.chunk_spp = ra.spp / chunks;
    ra.unit_rows = rows;
    pl->n_items = static_cast<uint64_t>(ra.local_tiles) * chunks * (GBL_TILE / rows);
}

gbl_status gbl_render_impl(gbl_ctx* ctx, const gbl_render_params* p, float* film_accum, gbl_stats* stats, const RenderKnobs& knobs);

// GBL_SCHEDULE_AUTO for the path tracer goes by how long the scene's paths are (choose_schedule): measured once per context,
// max_ray_depth and Russian-roulette setting by a pilot -- one instrumented sample per pixel over every 4th tile, native
// sampler, into a scratch film -- before anything of this call is queued.  A call too small to fill the wavefront pool takes
// the megakernel whatever the pilot would say, so it does not pay for one.  Leaves *rays_per_path at 0 when no pilot applies.
gbl_status auto_pilot(gbl_ctx* ctx, const gbl_render_params* p, const Plan& pl, const RenderKnobs& knobs, float* rays_per_path) {
    *rays_per_path = 0.0f;
    if (p->schedule != GBL_SCHEDULE_AUTO || p->integrator != GBL_INTEGRATOR_PATH || pl.stream_mode || ctx->scene.has_masks != 0 ||
        pl.call_paths < GBL_AUTO_WAVEFRONT_PATHS)
        return GBL_OK;
    const int key = p->max_ray_depth * 2 + (p->russian_roulette != 0 ? 1 : 0);
    auto it = ctx->auto_rays_per_path.find(key);
    if (it == ctx->auto_rays_per_path.end()) {
        float* scratch = nullptr;
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        const hipError_t me = hipMalloc(reinterpret_cast<void**>(&scratch), static_cast<size_t>(ctx->info.xres) * ctx->info.yres * 4 * sizeof(float));
        if (me != hipSuccess) return fail(ctx, GBL_ERR_OOM, std::string("hipMalloc(AUTO pilot film): ") + hipGetErrorString(me));
        gbl_render_params pilot;
        memset(&pilot, 0, sizeof(pilot));
        pilot.integrator = GBL_INTEGRATOR_PATH;
        pilot.sample_per_pixel = 1;
        pilot.max_ray_depth = p->max_ray_depth;
        pilot.ao_sample_num = p->ao_sample_num;
        pilot.bssrdf_sample_num = p->bssrdf_sample_num;
        pilot.tile_shard_index = 0;
        pilot.tile_shard_count = 4;
        pilot.sample_mode = GBL_SAMPLES_NATIVE;
        pilot.seed = 0x9011057ull;
        pilot.russian_roulette = p->russian_roulette;   // roulette shortens the paths AUTO goes by
        pilot.collect_stats = 1;
        pilot.schedule = GBL_SCHEDULE_MEGAKERNEL;
        pilot.stream = p->stream;
        gbl_stats ps;
        const gbl_status pst = gbl_render_impl(ctx, &pilot, scratch, &ps, knobs);
        (void)hipFree(scratch);
        if (pst != GBL_OK) return pst;
        const float rpp = ps.paths ? static_cast<float>(static_cast<double>(ps.extension_rays + ps.shadow_rays) / static_cast<double>(ps.paths)) : 0.0f;
        it = ctx->auto_rays_per_path.emplace(key, rpp).first;
    }
    *rays_per_path = it->second;
    return GBL_OK;
}

// Schedule.  The persistent megakernel keeps the path state in registers and regenerates paths in place; the wavefront
// formulation moves it through a 2^23-slot pool in HBM (~400 B per slot and iteration) to trace at five waves per SIMD with
// compacted queues.  Which pays is a matter of how much of a path is incoherent traversal: measured (tools/auto_check.py,
// 512^2 x 64 spp, wavefront / megakernel time) 1.6 on bunny.json at any depth (3.4 ... 3.5 rays per path), 1.15 ... 1.19 on the
// 15-bunny grid (3.5 ... 3.8), 1.04 / 0.98 / 0.96 / 0.92 / 0.91 on the Cornell box at max_ray_depth 4 / 6 / 8 / 12 / 16 (4.9 / 6.6 /
// 7.9 / 9.6 / 10.7 rays per path: a closed box, its paths never leave), 1.35 ... 1.73 on the feature scenes (2.9 ... 4.0); at full
// size 291 against 280 ms on BASELINE configs[3] and 3.39 against 4.62 s on configs[2], where the pool is refilled 130
// times.  AUTO = wavefront when the pilot sees GBL_AUTO_WAVEFRONT_RAYS_PER_PATH rays per path or more and the call
// (this rank's tiles x spp) holds at least GBL_AUTO_WAVEFRONT_PATHS camera samples to fill the pool with; megakernel
// otherwise, for mask scenes (the wavefront kernels run the filtered MIS query and the attenuation walks inline: 35.3
// against 20.2 ms on masked.json), for AO, Whitted and the stream sampler.  (Until round 3 AUTO went by instanced triangles
// and by whether the megakernel's LDS stacks would leave three workgroups per CU; the megakernel has since gained 6 ... 9 %
// and wins the grid at every size.)
// The wavefront renders in passes whose per-sample radiance buffer (16 B per sample) fits the budget.
gbl_status choose_schedule(gbl_ctx* ctx, const gbl_render_params* p, float pilot_rays_per_path, Plan& pl) {
    const RenderArgs& ra = pl.ra;
    const bool auto_wavefront = pilot_rays_per_path >= GBL_AUTO_WAVEFRONT_RAYS_PER_PATH && pl.call_paths >= GBL_AUTO_WAVEFRONT_PATHS;
    pl.wavefront = p->integrator == GBL_INTEGRATOR_PATH && !pl.stream_mode &&
                   (p->schedule == GBL_SCHEDULE_WAVEFRONT || (p->schedule == GBL_SCHEDULE_AUTO && !ctx->scene.has_masks && auto_wavefront));
    if (!pl.wavefront) return GBL_OK;
    pl.pass_spp = ra.spp;
    if (!ra.li_out) {
        const uint64_t budget = li_budget_bytes(ctx) / 16;
        while (pl.npix * pl.pass_spp > budget && pl.pass_spp % 2 == 0 && pl.pass_spp > 1) pl.pass_spp /= 2;
    }
    if (static_cast<uint64_t>(ra.local_tiles) * 64 * pl.pass_spp >= (1ull << 32) || pl.npix * pl.pass_spp >= (1ull << 32))
        return fail(ctx, GBL_ERR_INVALID, "too many paths per pass for 32-bit path ids: split the window");
    return GBL_OK;
}

// GBL_SAMPLES_STREAM: the reference's per-tile generator seeds of the full sample window, uploaded once per context
gbl_status upload_stream_seeds(gbl_ctx* ctx, RenderArgs& ra) {
    if (!ctx->stream_seeds) {
        const int32_t* full = ctx->scene.film.window;
        const int fty = (full[3] - full[2] + GBL_TILE - 1) / GBL_TILE;
        const std::vector<uint32_t> seeds = glibc_rand_sequence(static_cast<size_t>(ra.full_tiles_x) * fty);
        HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&ctx->stream_seeds), seeds.size() * sizeof(uint32_t)));
        HIP_TRY(ctx, hipMemcpy(ctx->stream_seeds, seeds.data(), seeds.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    ra.tile_seeds = ctx->stream_seeds;
    return GBL_OK;
}

// Opens the call's timing window: tev[0] of the gbl_get_timings ring entry, and ev0 when gbl_stats reports kernel_ms
gbl_status start_timing(gbl_ctx* ctx, hipEvent_t* tev, bool timed, hipStream_t stream) {
    if (timed) HIP_TRY(ctx, hipEventRecord(ctx->ev0, stream));
    HIP_TRY(ctx, hipEventRecord(tev[0], stream));
    return GBL_OK;
}

// The first-hit passes' grid: a thread per camera sample of the shard, at most 8 workgroups per CU (grid-stride)
dim3 sample_grid(const gbl_ctx* ctx, const RenderArgs& ra) {
    const uint64_t total = static_cast<uint64_t>(ra.local_tiles) * 64 * ra.spp;
    return dim3(static_cast<unsigned>(std::min<uint64_t>((total + GBL_BLOCK - 1) / GBL_BLOCK, static_cast<uint64_t>(ctx->num_cus) * 8)));
}

// Which builds the call launches, once the schedule is chosen: the first-hit passes, and whether the integrator's kernels are
// the lean ones of the native sampler.  The lean builds compile the tie rule out; every other build reads tri_order: the EXT,
// replay, stream, instrumented and exact_ties builds of the path tracer and AO (render_kernels.h TIES = REPLAY || STATS || EXACT ||
// EXT, which gbl_kernel_path / gbl_kernel_ao and the quad selectors instantiate from the same four facts), the wavefront trace
// kernels for those and for alpha masks (render_wavefront), the Whitted kernels and both first-hit passes (trace<> with its
// default TIES).  render_wavefront takes lean_native from here and the first-hit passes their conditions, so what gbl_render
// makes a pending tie order for is what it launches.
void choose_flavours(const gbl_ctx* ctx, const gbl_render_params* p, Plan& pl) {
    const DevScene& sc = ctx->scene;
    pl.vol_pass = sc.volume.on != 0u && !pl.stream_mode;
    pl.sss_pass = sc.has_bssrdf != 0 && p->integrator == GBL_INTEGRATOR_PATH && !pl.stream_mode;
    pl.lean_native = sc.extended == 0 && !(pl.wavefront && sc.has_masks != 0) && !pl.want_stats && !pl.replay && p->exact_ties == 0;
    pl.follows_ties = pl.whitted || pl.vol_pass || pl.sss_pass || !pl.lean_native;
}

// Passes over every camera sample's first hit, ahead of the integrator kernel (not under GBL_SAMPLES_STREAM, whose integrator
// kernels do this per pixel: the medium's draws follow each sample's Li draws in the tile's stream, stream_medium_phase):
// - the participating medium's {tr, Lv} (kernels/volume.h); the splat applies them;
// - the path tracer's Lsubsurface (kernels/subsurface.h), which the path kernels add at the first hit.
gbl_status first_hit_passes(gbl_ctx* ctx, const gbl_render_params* p, Plan& pl, hipStream_t stream) {
    const DevScene& sc = ctx->scene;
    RenderArgs& ra = pl.ra;
    const size_t lds = stack_lds_bytes(sc);
    gbl_status st;
    if (pl.vol_pass) {
        if ((st = grow(ctx, ctx->vol, pl.entries * 2 * sizeof(float4), "medium terms")) != GBL_OK) return st;
        ra.vol = static_cast<float*>(ctx->vol.p);
        gbl_render_kernel k_vol = gbl_kernel_vol(pl.replay);
        if ((st = allow_lds(ctx, k_vol, lds)) != GBL_OK) return st;
        hipLaunchKernelGGL(k_vol, sample_grid(ctx, ra), dim3(GBL_BLOCK), lds, stream, sc, ra);
        HIP_TRY(ctx, hipGetLastError());
    }
    if (pl.sss_pass) {
        if ((st = grow(ctx, ctx->sss, pl.entries * sizeof(float4), "subsurface term")) != GBL_OK) return st;
        float4* sss = static_cast<float4*>(ctx->sss.p);
        ra.sss = reinterpret_cast<const float*>(sss);
        gbl_li_kernel k_sss = gbl_kernel_sss(pl.replay);
        if ((st = allow_lds(ctx, k_sss, lds)) != GBL_OK) return st;
        hipLaunchKernelGGL(k_sss, sample_grid(ctx, ra), dim3(GBL_BLOCK), lds, stream, sc, ra, sss);
        HIP_TRY(ctx, hipGetLastError());
    }
    return GBL_OK;
}

// WhittedRenderer: one lane per camera sample with the recursion's frames in scratch (kernels/whitted.h), then the shared
// splat kernel.  Its timing window opens again here, after the medium pass.
gbl_status render_whitted(gbl_ctx* ctx, Plan& pl, const RenderKnobs& knobs, hipEvent_t* tev, bool timed, hipStream_t stream) {
    const DevScene& sc = ctx->scene;
    RenderArgs& ra = pl.ra;
    gbl_status st;
    float4* li = reinterpret_cast<float4*>(ra.li_out);
    if (!li) {
        if ((st = grow(ctx, ctx->li, pl.entries * sizeof(float4), "per-sample radiance")) != GBL_OK) return st;
        li = static_cast<float4*>(ctx->li.p);
    }
    if ((st = start_timing(ctx, tev, timed, stream)) != GBL_OK) return st;
    gbl_li_kernel k_wh = pl.stream_mode ? gbl_kernel_whitted_stream() : gbl_kernel_whitted(pl.replay);
    size_t lds = stack_lds_bytes(sc);
    if (pl.stream_mode) {
        const size_t want = std::max<size_t>(lds, 40 * 1024);
        ra.stream_lperm_words = static_cast<uint32_t>(want / sizeof(uint32_t));
        lds = want + (4 + GBL_STREAM_LDS_WORDS) * sizeof(uint32_t);
    }
    if ((st = allow_lds(ctx, k_wh, lds)) != GBL_OK) return st;
    dim3 grid = sample_grid(ctx, ra);
    if (pl.stream_mode) {   // one workgroup per tile in flight, each with its sample-generation scratch
        grid = dim3(static_cast<unsigned>(std::min<uint64_t>(static_cast<uint64_t>(ra.local_tiles), static_cast<uint64_t>(ctx->num_cus) * 4)));
        // a pixel's tail in the stream when a medium is present: per Li evaluation 6 floats per (light, slot) and 6 for the
        // two specular children, up to 2^(depth+1) - 1 evaluations per sample, then 9 per light sample of the medium.  The
        // phase walks the pixel in chunks, so the scratch only has to hold one sample's medium draws; give it the
        // worst case when that is small, 4 MiB per workgroup otherwise
        uint32_t tail = 0;
        if (sc.volume.on != 0u) {
            uint64_t slots = 0;
            for (int i = 0; i < sc.num_lights; ++i) slots += ctx->h_light_slots[i];
            const uint64_t med = medium_draws_per_sample(sc);
            const uint64_t worst = ((2ull << std::min(ra.max_depth, 20)) - 1) * (6 * slots + 6) + med;
            tail = static_cast<uint32_t>(std::max<uint64_t>(med, std::min<uint64_t>(worst, (1ull << 20) / pl.layout.S)));
            if (knobs.stream_tail_set) tail = knob_stream_tail(sc, knobs.stream_tail, pl.layout.S);
        }
        ra.stream_tail_cap = pl.layout.S * tail;
        if ((st = ensure_stream_buffers(ctx, stream_scratch_words(pl.layout, tail), grid.x, pl.entries, &ra)) != GBL_OK) return st;
    }
    hipLaunchKernelGGL(k_wh, grid, dim3(GBL_BLOCK), lds, stream, sc, ra, li);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(tev[1], stream));
    // replay records of another quota: the splat only reads their image positions, at the Whitted record stride
    return launch_splat(ctx, ra, li, 0, ra.spp, pl.replay, pl.want_stats, stream);
}

// The primary pass (kernels/packet.h): the camera rays of the call traced as packets, one wave per pixel and 64 of its
// samples, ahead of the path kernel, which then starts every path at its first hit (a camera ray whose answer depends on
// the visiting order -- an exact tie; under exact_ties also a hit the reference might not reach -- is flagged and traced by
// the path kernel itself, so the radiance is bit for bit what it is without the pass).  Native sampler's quad path
// kernels; 20 bytes per camera sample, within the per-sample radiance buffer's budget; GBL_PRIMARY=0 turns it off (A/B,
// bit-identity test).  *ran tells whether it did.
gbl_status primary_pass(gbl_ctx* ctx, const gbl_render_params* p, Plan& pl, const RenderKnobs& knobs, hipStream_t stream, bool* ran) {
    const DevScene& sc = ctx->scene;
    RenderArgs& ra = pl.ra;
    *ran = false;
    if (pl.stream_mode || p->integrator != GBL_INTEGRATOR_PATH || sc.num_lights <= 0 || !knobs.primary || sc.stack_entries > 64 ||
        pl.entries * 20 > li_budget_bytes(ctx))
        return GBL_OK;
    gbl_status st = grow(ctx, ctx->prim_hits, pl.entries * 20, "primary hits");
    if (st != GBL_OK) return st;
    // one word per work item of the path kernel (render_megakernel has planned its wave-owned units by now)
    if ((st = grow(ctx, ctx->prim_items, pl.n_items * sizeof(uint32_t), "primary items")) != GBL_OK) return st;
    HIP_TRY(ctx, hipMemsetAsync(ctx->prim_items.p, 0, pl.n_items * sizeof(uint32_t), stream));
    ra.prim_items = static_cast<uint32_t*>(ctx->prim_items.p);
    float4* ph = static_cast<float4*>(ctx->prim_hits.p);
    int32_t* pi = reinterpret_cast<int32_t*>(ph + pl.entries);
    const unsigned prim_wgs = 64u;   // workgroups per CU of the pass's grid-stride launch: 5 / 8 / 16 / 32 / 64 / 128 / 2048 -> 2.92 / 2.76 / 2.54 / 2.45 / 2.43 / 2.42 / 2.53 ms on configs[1]
    gbl_launch_primary(sc, ra, p->exact_ties != 0, ph, pi, static_cast<unsigned>(ctx->num_cus) * prim_wgs, stream);
    HIP_TRY(ctx, hipGetLastError());
    ra.prim_hit = reinterpret_cast<const float*>(ph);
    ra.prim_inst = pi;
    *ran = true;
    return GBL_OK;
}

// The device counters of a measurement build on stderr: with phase_clock the phase shares of a -DGBL_PHASE_CLOCK build
// (tools/phase_clock.py), otherwise the instrumented build's probes (GBL_PROBE with collect_stats)
void print_counters(const unsigned long long* h, bool phase_clock) {
    if (!phase_clock)
        fprintf(stderr, "probe: interior lane-steps %llu wave-steps %llu (util %.3f) | leaf/other lane %llu wave %llu (util %.3f)\n", h[7], h[8],
                h[8] ? h[7] / (64.0 * h[8]) : 0.0, h[9], h[10], h[10] ? h[9] / (64.0 * h[10]) : 0.0);
    if (h[25] + h[26] + h[27] + h[28] + h[29]) {   // the stream sampler's phases (-DGBL_STREAM_TM in an un-instrumented build)
        const double tot = static_cast<double>(h[25] + h[26] + h[27] + h[28] + h[29]);
        fprintf(stderr, "%s (share of the workgroups' time): emit %.1f%% permute %.1f%% assemble %.1f%% paths %.1f%% skip %.1f%%\n",
                phase_clock ? "stream phases" : "probe: stream sampler phases",
                100.0 * h[25] / tot, 100.0 * h[26] / tot, 100.0 * h[27] / tot, 100.0 * h[28] / tot, 100.0 * h[29] / tot);
    }
    if (phase_clock) {
        if (h[8]) {
            const double k = static_cast<double>(h[8]);
            fprintf(stderr, "phase clock (share of the waves' ticks): closest-hit query %.1f%% = dense %.1f%% + migrate %.1f%% + quad %.1f%% | any-hit query %.1f%% = dense "
                    "%.1f%% + migrate %.1f%% + quad %.1f%% | rest (shading, regeneration, item fetch) %.1f%% | dense iterations %llu, quad iterations %llu, "
                    "wave ticks %llu\n", 100 * h[0] / k, 100 * h[1] / k, 100 * h[2] / k, 100 * h[3] / k, 100 * h[4] / k, 100 * h[5] / k, 100 * h[6] / k, 100 * h[7] / k,
                    100 * (k - h[0] - h[4]) / k, h[9], h[10], h[8]);
            fprintf(stderr, "phase clock, item loop: iterations run with lanes that have nothing left to take (drain) %.2f%%, between an item's last iteration and the next "
                    "one's first (barriers, fetch) %.2f%%\n", 100 * h[30] / k, 100 * h[31] / k);
            fprintf(stderr, "phase clock, dense loop: interior blocks %llu (%.0f ticks, %.1f lanes each, %.1f%% of the kernel), leaf / instance blocks %llu (%.0f ticks, %.1f lanes, %.1f%%)\n",
                    h[13], h[13] ? double(h[11]) / h[13] : 0.0, h[13] ? double(h[15]) / h[13] : 0.0, 100 * h[11] / k, h[14], h[14] ? double(h[12]) / h[14] : 0.0,
                    h[14] ? double(h[16]) / h[14] : 0.0, 100 * h[12] / k);
            fprintf(stderr, "phase clock, quad loop: interior iterations %llu (%.0f ticks each, %.1f%%), leaf %llu (%.0f ticks, %.1f%%), transitions / exit %llu (%.0f ticks, %.1f%%); %.2f rays per iteration\n",
                    h[20], h[20] ? double(h[17]) / h[20] : 0.0, 100 * h[17] / k, h[21], h[21] ? double(h[18]) / h[21] : 0.0, 100 * h[18] / k, h[22],
                    h[22] ? double(h[19]) / h[22] : 0.0, 100 * h[19] / k, h[10] ? double(h[23]) / h[10] : 0.0);
        }
        return;
    }
    if (h[11] + h[12] + h[13] + h[14] + h[15] + h[16] + h[17]) {
        const char* names[7] = {"<=3", "4-7", "8-15", "16-31", "32-63", "64-127", ">=128"};
        unsigned long long rays = 0, steps = 0;
        for (int i = 0; i < 7; ++i) {
            rays += h[11 + i];
            steps += h[18 + i];
        }
        fprintf(stderr, "probe: closest-hit rays by interior steps (share of rays / share of steps):");
        for (int i = 0; i < 7; ++i)
            fprintf(stderr, " %s %.1f%%/%.1f%%", names[i], 100.0 * h[11 + i] / rays, 100.0 * h[18 + i] / std::max(1ull, steps));
        fprintf(stderr, "\n");
    }
}

// The persistent megakernel (kernels/render_kernels.h) of the path tracer or AO: picks its build, the quad kernel and the
// primary pass where they apply, sizes the resident grid, launches it and splats the per-sample radiance it kept
gbl_status render_megakernel(gbl_ctx* ctx, const gbl_render_params* p, Plan& pl, const RenderKnobs& knobs, hipEvent_t main_done,
                             hipStream_t stream) {
    const DevScene& sc = ctx->scene;
    RenderArgs& ra = pl.ra;
    const bool stream_mode = pl.stream_mode, want_stats = pl.want_stats, ties = p->exact_ties != 0;
    const bool ao = p->integrator == GBL_INTEGRATOR_AO;
    const bool ext = sc.extended != 0;   // see render_wavefront
    gbl_status st;
    size_t lds = pl.lds;
    // persistent grid: enough workgroups to fill every CU at the occupancy LDS allows, never more than items
    uint64_t grid64 = std::min<uint64_t>(pl.n_items, static_cast<uint64_t>(ctx->num_cus) * pl.per_cu);
    dim3 grid(static_cast<unsigned>(grid64)), block(GBL_BLOCK);
    gbl_render_kernel kernel = nullptr;
    if (stream_mode) {
        kernel = ao ? gbl_kernel_ao_stream(ext || want_stats) : gbl_kernel_path_stream(want_stats, ext || want_stats);
        // a sample's tail in the stream: up to 6 discarded floats per bounce, 9 per light sample of the medium
        const uint32_t med = static_cast<uint32_t>(medium_draws_per_sample(sc));
        uint32_t tail_words = (ao ? 0u : 6u * static_cast<uint32_t>(ra.max_depth)) + med;
        if (knobs.stream_tail_set && sc.volume.on) tail_words = knob_stream_tail(sc, knobs.stream_tail, pl.layout.S);
        ra.stream_tail_cap = pl.layout.S * tail_words;
        if ((st = ensure_stream_buffers(ctx, stream_scratch_words(pl.layout, tail_words), grid64, pl.entries, &ra)) != GBL_OK) return st;
    } else {
        kernel = ao ? gbl_kernel_ao(pl.replay, want_stats, ext || want_stats, ties) : gbl_kernel_path(pl.replay, want_stats, ext || want_stats, ties);
    }
    if ((st = allow_lds(ctx, kernel, lds)) != GBL_OK) return st;
    if (ra.li_out) {   // plan_render: pl.defer
        ra.li_defer = ra.li_out;
    } else if (pl.defer) {
        if ((st = grow(ctx, ctx->li, pl.entries * sizeof(float4), "per-sample radiance")) != GBL_OK) return st;
        ra.li_defer = static_cast<float*>(ctx->li.p);
    }
    // kernels/quadtrace.h: sparse interior steps run four lanes per ray (-9 ... -14 % on the BASELINE scenes); per-sample
    // radiance only, the quads' records take the LDS film tile's place.  Its LDS need differs from the film-tile formula of
    // plan_render: checked again here, and a scene whose stacks only fit the one-ray-per-lane kernel keeps that one.  The lean
    // kernels of the native sampler only (with or without exact_ties): the EXT builds are slower under it, replay and
    // instrumented renders are not timed.
    if (pl.defer && !ext && (stream_mode || !pl.replay) && !want_stats && knobs.mk_quad) {
        // (stream mode: the shuffles' LDS region, at least the stacks', and the generator's state come on top)
        const size_t stack_bytes = stream_mode ? static_cast<size_t>(ra.stream_lperm_words) * sizeof(uint32_t) : stack_lds_bytes(sc);
        size_t lds_quad = (gbl_quad_lds_words() + 4 + (stream_mode ? GBL_STREAM_LDS_WORDS : 0)) * sizeof(uint32_t) + stack_bytes;
        // the top of the tree in LDS (trace.h HotLdsStack): as many nodes of the breadth-first prefix as fit into what the
        // stacks leave of the LDS share of the workgroups per CU they allow anyway (granules of 1280 bytes, 128 per CU)
        ra.hot_count = 0;
        ra.hot_word = static_cast<uint32_t>(lds_quad / sizeof(uint32_t));
        if (!stream_mode && sc.hot_nodes > 0 && lds_quad <= 160 * 1024) {
            const size_t gran = 1280, granules = (lds_quad + gran - 1) / gran;
            const size_t wgs = std::max<size_t>(1, std::min<size_t>(GBL_PT_WAVES * 4 * 64 / GBL_BLOCK, 128 / granules));
            size_t room = (128 / wgs) * gran - lds_quad;
            if (knobs.hot_lds >= 0) room = static_cast<size_t>(knobs.hot_lds) * sizeof(DevNode);
            ra.hot_count = static_cast<uint32_t>(std::min<size_t>(sc.hot_nodes, room / sizeof(DevNode)));
            if (lds_quad + ra.hot_count * sizeof(DevNode) > 160 * 1024) ra.hot_count = 0;
            lds_quad += ra.hot_count * sizeof(DevNode);
        }
        gbl_render_kernel k_quad = stream_mode ? (ao ? nullptr : gbl_kernel_path_stream_quad()) : ao ? gbl_kernel_ao_quad(ties) : gbl_kernel_path_quad(ties);
        if (k_quad && lds_quad <= 160 * 1024) {
            kernel = k_quad;
            lds = lds_quad;
            if ((st = allow_lds(ctx, kernel, lds)) != GBL_OK) return st;
            if (!stream_mode && !ao && gbl_quad_wave_units()) {   // wave-owned units: four waves to a workgroup, never more waves than units
                plan_wave_units(ctx, &pl);
                grid64 = std::min<uint64_t>((pl.n_items + GBL_BLOCK / 64 - 1) / (GBL_BLOCK / 64), static_cast<uint64_t>(ctx->num_cus) * pl.per_cu);
                grid = dim3(static_cast<unsigned>(grid64));
            }
            bool primary = false;
            if ((st = primary_pass(ctx, p, pl, knobs, stream, &primary)) != GBL_OK) return st;
            if (primary) {
                kernel = gbl_kernel_path_quad_primary(ties);   // the same kernel, its paths starting at those hits
                if ((st = allow_lds(ctx, kernel, lds)) != GBL_OK) return st;
            }
        }
    }
    {
        // the persistent grid is what is resident: registers may allow fewer workgroups per CU than LDS does (EXT builds)
        int occ = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, reinterpret_cast<const void*>(kernel), GBL_BLOCK, lds) == hipSuccess && occ >= 1) {
            grid64 = std::max<uint64_t>(1, std::min<uint64_t>(grid64, static_cast<uint64_t>(ctx->num_cus) * occ));
            if (!stream_mode) grid = dim3(static_cast<unsigned>(grid64));   // (stream mode sized its scratch for the original grid)
        }
    }
    const bool phase_clock = knobs.phase_clock && !want_stats;
    if (phase_clock) HIP_TRY(ctx, hipMemsetAsync(ctx->stats, 0, 32 * sizeof(unsigned long long), stream));
    hipLaunchKernelGGL(kernel, grid, block, lds, stream, sc, ra);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(main_done, stream));
    if (phase_clock) {
        unsigned long long h[32];
        HIP_TRY(ctx, hipStreamSynchronize(stream));
        HIP_TRY(ctx, hipMemcpy(h, ctx->stats, sizeof(h), hipMemcpyDeviceToHost));
        print_counters(h, true);
    }
    return pl.defer ? launch_splat(ctx, ra, reinterpret_cast<float4*>(ra.li_defer), 0, ra.spp, pl.replay, want_stats, stream) : GBL_OK;
}

// Closes the call: the medium's terms into the caller's per-sample output, the timing events, and gbl_stats.  The Whitted
// kernel is not instrumented: it reports no ray counters, and the path count of the whole window whatever the shard.
gbl_status finish_render(gbl_ctx* ctx, const Plan& pl, const RenderKnobs& knobs, hipEvent_t* tev, hipStream_t stream, gbl_stats* stats) {
    const RenderArgs& ra = pl.ra;
    if (ra.vol && ra.li_out) {   // the caller's per-sample output carries what the tile received: tr * Li + Lv
        gbl_launch_vol_combine(reinterpret_cast<float4*>(ra.li_out), reinterpret_cast<const float4*>(ra.vol), pl.entries, stream);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipEventRecord(tev[2], stream));
    ctx->t_calls += 1;
    if (!stats) return GBL_OK;
    unsigned long long h[32];
    const gbl_status st = close_call(ctx, pl, stream, stats, pl.whitted ? nullptr : h);
    if (st != GBL_OK) return st;
    stats->schedule = pl.wavefront ? GBL_SCHEDULE_WAVEFRONT : GBL_SCHEDULE_MEGAKERNEL;
    if (pl.whitted) {
        stats->paths = pl.entries;
        return GBL_OK;
    }
    if (!pl.want_stats) return GBL_OK;
    if (knobs.probe) print_counters(h, false);
    // (the AO kernel of the stream sampler has no instrumented build, gbl_kernel_ao_stream: its launch leaves the device
    //  counters at zero -- report the path count computed above and no ray counters rather than zeros for both)
    const bool main_instrumented = !(pl.stream_mode && ra.integrator == GBL_INTEGRATOR_AO);
    if (main_instrumented) stats->paths = h[0];
    stats->extension_rays = h[1];
    stats->shadow_rays = h[2];
    stats->nodes = h[3];
    stats->tris = h[4];
    stats->splats = h[5];
    stats->dims = h[6];
    return GBL_OK;
}

// gbl_render: plan the call, run the AUTO pilot, choose the schedule, then queue the first-hit passes, the integrator and
// the epilogue.  A call that fails a check queues nothing.
gbl_status gbl_render_impl(gbl_ctx* ctx, const gbl_render_params* p, float* film_accum, gbl_stats* stats, const RenderKnobs& knobs) {
    if (!ctx) return GBL_ERR_INVALID;
    if (!p || !film_accum) return fail(ctx, GBL_ERR_INVALID, "null argument");
    Plan pl;
    gbl_status st = plan_render(ctx, p, film_accum, &pl);
    if (st != GBL_OK) return st;
    if (pl.n_items == 0) {
        if (stats) memset(stats, 0, sizeof(*stats));
        return GBL_OK;
    }
    float rays_per_path = 0.0f;
    if ((st = auto_pilot(ctx, p, pl, knobs, &rays_per_path)) != GBL_OK) return st;
    if ((st = choose_schedule(ctx, p, rays_per_path, pl)) != GBL_OK) return st;
    choose_flavours(ctx, p, pl);
    if ((st = make_orders_if(ctx, pl.follows_ties)) != GBL_OK) return st;   // a deferred vertex edit's tie order, for its first reader

    hipStream_t stream = static_cast<hipStream_t>(p->stream);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemsetAsync(ctx->work_counter, 0, sizeof(uint32_t), stream));
    if (pl.want_stats) HIP_TRY(ctx, hipMemsetAsync(ctx->stats, 0, 32 * sizeof(unsigned long long), stream));
    if (pl.stream_mode && (st = upload_stream_seeds(ctx, pl.ra)) != GBL_OK) return st;
    hipEvent_t* tev = ctx->t_ev[ctx->t_calls % gbl_ctx::kTimingRing];   // [0] start, [1] after the integrator kernel, [2] end
    for (int k = 0; k < 3; ++k)
        if (!tev[k]) HIP_TRY(ctx, hipEventCreate(&tev[k]));
    if ((st = start_timing(ctx, tev, stats != nullptr, stream)) != GBL_OK) return st;
    if ((st = first_hit_passes(ctx, p, pl, stream)) != GBL_OK) return st;
    if (pl.whitted)
        st = render_whitted(ctx, pl, knobs, tev, stats != nullptr, stream);
    else if (pl.wavefront)
        st = render_wavefront(ctx, p, pl, knobs, tev[1], stream);
    else
        st = render_megakernel(ctx, p, pl, knobs, tev[1], stream);
    if (st != GBL_OK) return st;
    return finish_render(ctx, pl, knobs, tev, stream, stats);
}

}   // namespace

extern "C" {

gbl_status gbl_render(gbl_ctx* ctx, const gbl_render_params* p, float* film_accum, gbl_stats* stats) {
    return gbl_guard([&] { return gbl_render_impl(ctx, p, film_accum, stats, read_knobs()); }, [&](const std::string& what) { if (ctx) ctx->error = what; });
}

int gbl_get_timings(gbl_ctx* ctx, int n, gbl_timing* out) {
    if (!ctx || !out || n <= 0) return 0;
    int have = static_cast<int>(std::min<unsigned long long>(ctx->t_calls, gbl_ctx::kTimingRing));
    n = std::min(n, have);
    for (int i = 0; i < n; ++i) {
        hipEvent_t* ev = ctx->t_ev[(ctx->t_calls - 1 - i) % gbl_ctx::kTimingRing];
        float a = 0.0f, b = 0.0f;
        if (hipEventSynchronize(ev[2]) != hipSuccess || hipEventElapsedTime(&a, ev[0], ev[1]) != hipSuccess ||
            hipEventElapsedTime(&b, ev[0], ev[2]) != hipSuccess)
            return i;
        out[i].main_kernel_ms = a;
        out[i].total_ms = b;
    }
    return n;
}

}  // extern "C"
