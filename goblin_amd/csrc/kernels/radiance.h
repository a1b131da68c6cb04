// gbl_radiance_rays' kernel: PathTracer::Li (GoblinPathtracer.cpp:50-179) along a flat array of caller rays in device memory, one
// {Li, 1} per ray.
//
//   radiance_trace   persistent workgroups, one path per lane with its PathState in registers.  The SOURCE is query_trace's refill
//                    (kernels/query.h): wave w of W owns the 64-ray regions w, w + W, ... and hands their rays to its idle lanes by
//                    ballot and prefix popcount, the cursor its own, no atomic.  The LOOP is the megakernel's one-ray-per-lane
//                    iteration (kernels/render_kernels.h path_trace_kernel<.., QUAD = false, PRIM = false>): closest-hit query,
//                    close the bounce, shade the vertex, shadow query, BSDF sample -- the same expressions over shade.h's functions
//                    in the same order, so a ray that is a frame's camera ray gets that camera sample's Li bit for bit.  The SINK is
//                    one float4 store per path.
//
// What differs from the megakernel's vertex 0: the ray is the caller's (its own [mint, maxt] for the first query, +inf afterwards)
// and carries no differentials -- RayDifferential(o, d) without auxiliary rays (GoblinRay.h:48-51), which is what every
// continuation ray is -- so hit_differentials runs with primary = false at every vertex.  Lsubsurface and the medium are not
// computed here: the host refuses such scenes.
//
// REPLAY: the draws are the caller's records (gbl_render's replay layout; the first four floats are not read); otherwise the native
// law, ray i being sample i % S of group first_group + i / S.  EXT: the scene is beyond the headline feature set.  TIES: the
// reference's exact-t tie rule (trace.h), REPLAY || EXT || GBL_RADIANCE_EXACT_TIES.
//
// Stacks: HotSplitStack in persistent_layout's form, as the query kernels -- GBL_WF_STACK_LDS levels per lane and the top of the tree
// in LDS, the deeper levels in the context's query backing -- so no tree is too deep for the call.
#pragma once
#include "query.h"   // query_ray_valid, GBL_QUERY_REFILL
#include "radiance_args.h"
#include "render_kernels.h"   // PathState, eval_attenuation, hit_differentials

#define GBL_RADIANCE_UNIT_TOL 1e-4f   // |d.d - 1| beyond it: an invalid ray (every BSDF reads wo = -d)

template <bool REPLAY, bool EXT, bool TIES>
__global__ __launch_bounds__(GBL_BLOCK, EXT ? GBL_EXT_WAVES : GBL_PT_WAVES) void radiance_trace(DevScene sc, RadianceArgs ra) {
    constexpr bool LAST_SKIP = !REPLAY && !EXT;   // the capped vertex traces no ray under a delta light (path_trace_kernel)
    constexpr bool LAZY_DRAWS = LAST_SKIP;        // ... and a vertex's sample dimensions are drawn only where they are read
    extern __shared__ __align__(16) unsigned char smem[];
    HotSplitStack stk;
    stk.p = gbl_as_lds(reinterpret_cast<uint32_t*>(smem) + threadIdx.x);
    stk.g = gbl_as_global(ra.stack_spill + blockIdx.x * GBL_BLOCK + threadIdx.x);
    stk.gstride = gridDim.x * GBL_BLOCK;
    {   // the top of the tree, once per (persistent) workgroup: trace.h HotLdsStack
        uint4* hot = reinterpret_cast<uint4*>(reinterpret_cast<uint32_t*>(smem) + ra.hot_word);
        for (uint32_t i = threadIdx.x; i < 4u * ra.hot_count; i += GBL_BLOCK) hot[i] = reinterpret_cast<const uint4*>(sc.nodes)[i];
        stk.hot = (const gbl_lds_u4*)hot;
        stk.hot_count = ra.hot_count;
        if (ra.hot_count) __syncthreads();
    }
    LaneCounters cnt = {};
    const int lane = threadIdx.x & 63;
    const uint32_t n_regions = (ra.n >> 6) + ((ra.n & 63u) != 0u ? 1u : 0u);   // (n + 63 may not fit 32 bits)
    const uint32_t n_waves = gridDim.x * (GBL_BLOCK / 64);
    // this wave's regions: w, w + n_waves, w + 2 n_waves, ...; the last region of the array may be short
    uint32_t region = blockIdx.x * (GBL_BLOCK / 64) + (threadIdx.x >> 6);
    auto region_count = [&](uint32_t r) { return r < n_regions ? min(64u, ra.n - r * 64u) : 0u; };
    uint32_t r_off = 0, r_cnt = region_count(region);

    PathState ps;
    bool active = false;
    SampleSource src;
    src.spp = ra.spp;
    src.root = ra.root;
    src.rec = nullptr;
    src.pixel_key = 0;
    src.k = 0;
    uint32_t idx = 0;
    float query_maxt = INFINITY;   // of the ray in flight: the caller's for the first query, +inf for every extension ray

    for (;;) {
        // ---- refill idle lanes from this wave's regions (all scalar bookkeeping)
        const unsigned long long idle = __ballot(!active);
        const int n_idle = __popcll(idle);
        if (region < n_regions && n_idle > 0) {
            const int my_rank = __popcll(idle & ((1ull << lane) - 1ull));
            int assigned = 0;
            uint32_t my_entry = 0xffffffffu;   // (no ray has this number: n < 2^32)
            while (assigned < n_idle && region < n_regions) {
                const int avail = static_cast<int>(r_cnt - r_off);
                const int take = min(avail, n_idle - assigned);
                if (!active && my_rank >= assigned && my_rank < assigned + take) my_entry = region * 64u + r_off + static_cast<uint32_t>(my_rank - assigned);
                assigned += take;
                r_off += take;
                if (r_off >= r_cnt) {
                    region += n_waves;
                    r_off = 0;
                    r_cnt = region_count(region);
                }
            }
            if (my_entry != 0xffffffffu) {
                const float4 a = ra.rays[2 * static_cast<size_t>(my_entry)], b = ra.rays[2 * static_cast<size_t>(my_entry) + 1];
                const float dd = b.x * b.x + b.y * b.y + b.z * b.z;
                if (!query_ray_valid(a, b) || !(fabsf(dd - 1.0f) <= GBL_RADIANCE_UNIT_TOL)) {
                    ra.out[my_entry] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);   // an invalid ray: no node fetched, and the lane stays idle
                } else if (sc.num_lights == 0) {
                    ra.out[my_entry] = make_float4(0.0f, 0.0f, 0.0f, 1.0f);   // PathTracer::Li returns Black without lights (:53-56)
                } else {
                    idx = my_entry;
                    if (REPLAY) {
                        src.rec = ra.records + static_cast<size_t>(my_entry) * ra.dims;
                    } else {
                        src.k = my_entry % static_cast<uint32_t>(ra.spp);
                        src.pixel_key = nat_mix(ra.seed_key, ra.first_group + my_entry / static_cast<uint32_t>(ra.spp));
                    }
                    ps.o = f3(a.x, a.y, a.z);
                    ps.d = f3(b.x, b.y, b.z);
                    ps.mint = a.w;
                    query_maxt = b.w;
                    ps.throughput = f3(1.0f, 1.0f, 1.0f);
                    ps.Li = f3(0.0f, 0.0f, 0.0f);
                    ps.bounce = -1;
                    ps.punch = false;
                    ps.first = true;
                    active = true;
                }
            }
        }
        if (__ballot(active) == 0ull) {
            if (region >= n_regions) break;
            continue;
        }

        // ---- closest-hit query
        bool finished = false;
        Hit hit;
        bool got = false;
        if (active) got = trace<false, false, EXT, TIES>(sc, ps.o, ps.d, ps.mint, query_maxt, stk, hit, cnt);
        Frag fr;
        TexFrag tf;
        // ---- close the bounce
        if (active) {
            if (got) {
                make_fragment<EXT>(sc, hit, ps.o, ps.d, fr, &tf);
                if (EXT && sc.materials[sc.instances[hit.inst].material].has_tex != 0u)
                    hit_differentials<REPLAY>(sc, src, false, 0.0f, 0.0f, fr, tf);
            }
            // The MIS query sees opaque surfaces only (isOpaque, GoblinPathtracer.cpp:148) and is attenuated by the masks in front of
            // them; the extension query above sees everything.  They only differ when the closest surface is a mask.
            int mis_inst = got ? hit.inst : -1;
            F3 mis_n = fr.n, mis_tr = f3(1.0f, 1.0f, 1.0f);
            if (EXT && sc.has_masks != 0 && got && ps.bounce >= 0 && !ps.punch && sc.instances[hit.inst].is_mask != 0u) {
                Hit ho;
                const bool go = trace<false, false, EXT>(sc, ps.o, ps.d, ps.mint, INFINITY, stk, ho, cnt, GBL_FILTER_OPAQUE);
                mis_tr = eval_attenuation<false>(sc, ps.o, ps.d, ps.mint, go ? ho.t : INFINITY, stk, cnt);
                mis_inst = go ? ho.inst : -1;
                if (go) {
                    Frag fo;
                    make_fragment<EXT>(sc, ho, ps.o, ps.d, fo);
                    mis_n = fo.n;
                }
            }
            if (ps.bounce < 0) {
                if (!got) {
                    if (EXT) {   // Li += scene->evalEnvironmentLight(ray), GoblinPathtracer.cpp:61-65: Black without an image based light
                        const F3 le = environment_le<EXT>(sc, ps.d);
                        ps.Li = f3(ps.Li.x + le.x, ps.Li.y + le.y, ps.Li.z + le.z);
                    }
                    finished = true;
                } else {
                    F3 le = hit_Le(sc, hit.inst, fr.n, -ps.d);
                    ps.Li = f3(ps.Li.x + le.x, ps.Li.y + le.y, ps.Li.z + le.z);
                    ps.bounce = 0;
                }
            } else if (EXT && ps.punch) {
                // the bounce that punched through a mask contributes no direct light (`continue`, :122-136)
                ps.punch = false;
                ps.bounce += 1;
                if (!got) {
                    if (ps.first) {   // "primary ray need to evaluate image based lighting in this case" (:125-131)
                        const F3 le = ps.throughput * environment_le<EXT>(sc, ps.d);
                        ps.Li = f3(ps.Li.x + le.x, ps.Li.y + le.y, ps.Li.z + le.z);
                    }
                    finished = true;
                }
            } else {
                ps.first = false;
                // close the previous bounce: MIS term for the sampled direction, then Li and throughput
                if (mis_inst >= 0 && sc.instances[mis_inst].area_light == ps.light) {
                    F3 le = hit_Le(sc, mis_inst, mis_n, -ps.d);
                    if (!is_black(le)) {
                        // Ld += f * tr * Li * absdot(wi, n) * fWeight / bsdfPdf   (tr == 1 without masks)
                        F3 term = EXT ? div(ps.f * mis_tr * le * ps.cosw * ps.fw, ps.bsdf_pdf) : div(ps.f * le * ps.cosw * ps.fw, ps.bsdf_pdf);
                        ps.Ld = f3(ps.Ld.x + term.x, ps.Ld.y + term.y, ps.Ld.z + term.z);
                    }
                } else if (EXT && mis_inst < 0 && sc.has_ibl != 0) {
                    // the sampled direction left the scene: Ld += f * tr * light->Le(r) * fWeight / bsdfPdf (:157-161; no cosine there)
                    const F3 le = light_le_escaped<EXT>(sc, sc.lights[ps.light], ps.d);
                    const F3 term = div(ps.f * mis_tr * le * ps.fw, ps.bsdf_pdf);
                    ps.Ld = f3(ps.Ld.x + term.x, ps.Ld.y + term.y, ps.Ld.z + term.z);
                }
                F3 add = div(ps.throughput * ps.Ld, ps.pick_pdf);
                ps.Li = f3(ps.Li.x + add.x, ps.Li.y + add.y, ps.Li.z + add.z);
                F3 scale = div(ps.f * ps.cosw, ps.bsdf_pdf);
                ps.throughput = ps.throughput * scale;
                ps.bounce += 1;
                if (!got) finished = true;
            }
            if (!finished && ps.bounce >= ra.max_depth - 1) finished = true;
        }

        // ---- shade the vertex: light sample (shadow ray below) and BSDF sample
        bool need_shadow = false;
        F3 shadow_d = f3(0, 0, 1), contrib = f3(0, 0, 0);
        float shadow_maxt = 0.0f;
        F3 wo = -ps.d;
        const DevMaterial* mat = nullptr;
        ResolvedMat rmat;       // EXT: the hit material with its textures evaluated / its mask unwrapped
        F3 l_f = f3(0, 0, 0), l_L = f3(0, 0, 0);
        float l_cos = 0.0f, l_w = 1.0f, l_pdf = 1.0f;
        bool l_area = false;
        float u_bsdf_c = 0.0f, u_bsdf_1 = 0.0f, u_bsdf_2 = 0.0f;
        if (active && !finished) {
            const int b = ps.bounce;
            // The vertex's seven sample dimensions: 1D 3b (light component), 3b + 1 (BSDF component), 3b + 2 (light pick); 2D 2b
            // (light), 2b + 1 (BSDF) -- the megakernel's and wf_shade's, LAZY_DRAWS as path_trace_kernel explains it
            float u_light_c = 0.0f, u_light_1 = 0.0f, u_light_2 = 0.0f, u_pick = 0.0f;
            if (REPLAY) {
                const float* r1 = src.rec + 4 + 3 * b;
                const float* r2 = src.rec + ra.off2_base + 4 * b;
                u_light_c = r1[0]; u_bsdf_c = r1[1]; u_pick = r1[2];
                u_light_1 = r2[0]; u_light_2 = r2[1]; u_bsdf_1 = r2[2]; u_bsdf_2 = r2[3];
            } else if constexpr (!LAZY_DRAWS) {
                u_light_c = src.native_1d(3u * b + 0u);
                u_bsdf_c = src.native_1d(3u * b + 1u);
                u_pick = src.native_1d(3u * b + 2u);
                src.native_2d(0x10000u + 2u * b, 1u, 0u, true, &u_light_1, &u_light_2);
                src.native_2d(0x10000u + 2u * b + 1u, 1u, 0u, true, &u_bsdf_1, &u_bsdf_2);
            } else {
                const bool pair = !mat_sample_reads_comp(sc.materials[sc.instances[hit.inst].material]);
                float a0, a1;
                src.native_1d_or_2d(pair, 3u * b + 1u, 0x10000u + 2u * b + 1u, &a0, &a1);
                u_bsdf_c = pair ? 0.0f : a0;
                u_bsdf_1 = pair ? a0 : 0.0f;
                u_bsdf_2 = pair ? a1 : 0.0f;
            }
            // Scene::sampleLight: CDF1D::sampleDiscrete over the power distribution (one light: index 0 for every u)
            if (LAZY_DRAWS && sc.num_lights > 1) u_pick = src.native_1d(3u * b + 2u);
            int li = 0;
            for (int i = 1; i <= sc.num_lights; ++i)
                if (sc.light_cdf[i] < u_pick) li = i;
            if (li >= sc.num_lights) li = sc.num_lights - 1;
            ps.light = li;
            ps.pick_pdf = sc.light_pick_pdf[li];
            ps.Ld = f3(0, 0, 0);
            mat = sc.materials + sc.instances[hit.inst].material;
            if (EXT) resolve_hit_material(sc, sc.instances[hit.inst].material, fr, tf, rmat);
            const DevLight& light = sc.lights[li];
            if (LAZY_DRAWS && light_sample_reads_u<EXT>(light)) {
                u_light_c = src.native_1d(3u * b + 0u);
                src.native_2d(0x10000u + 2u * b, 1u, 0u, true, &u_light_1, &u_light_2);
            }
            LightSampleOut ls;
            light_sample<EXT>(sc, light, fr.p, fr.eps, u_light_c, u_light_1, u_light_2, ls);
            if (!is_black(ls.L) && ls.pdf > 0.0f) {
                F3 f = EXT ? rmat_bsdf(rmat, fr.n, wo, ls.wi) : mat_bsdf(*mat, fr.n, wo, ls.wi);
                if (!is_black(f)) {
                    need_shadow = true;
                    shadow_d = ls.wi;
                    shadow_maxt = ls.maxt;
                    float lw = 1.0f;
                    if (light_is_delta<EXT>(light)) {
                        contrib = div(f * ls.L * absdot(fr.n, ls.wi), ls.pdf);
                    } else {
                        float bp = EXT ? rmat_pdf(rmat, fr.n, wo, ls.wi) : mat_pdf(*mat, fr.n, wo, ls.wi);
                        lw = power_heuristic(ls.pdf, bp);
                        contrib = div(f * ls.L * absdot(fr.n, ls.wi) * lw, ls.pdf);
                    }
                    if (EXT) {   // kept for the attenuated form f * tr * L * |n.wi| (* lWeight) / lightPdf below
                        l_f = f;
                        l_L = ls.L;
                        l_cos = absdot(fr.n, ls.wi);
                        l_w = lw;
                        l_pdf = ls.pdf;
                        l_area = !light_is_delta<EXT>(light);
                    }
                }
            }
        }
        // ---- shadow query (any-hit)
        if (need_shadow) {
            Hit dummy;
            const bool masks = EXT && sc.has_masks != 0;
            const bool occluded = trace<true, false, EXT, TIES>(sc, fr.p, shadow_d, fr.eps, shadow_maxt, stk, dummy, cnt, masks ? GBL_FILTER_OPAQUE : GBL_FILTER_NONE);
            if (!occluded && masks) {
                F3 tr = eval_attenuation<false>(sc, fr.p, shadow_d, fr.eps, shadow_maxt, stk, cnt);
                contrib = l_area ? div(l_f * tr * l_L * l_cos * l_w, l_pdf) : div(l_f * tr * l_L * l_cos, l_pdf);
            }
            if (!occluded) ps.Ld = f3(ps.Ld.x + contrib.x, ps.Ld.y + contrib.y, ps.Ld.z + contrib.z);
        }
        // ---- the last vertex under a delta light: no next ray (path_trace_kernel's LAST_SKIP: the dead-end term, added here)
        if constexpr (LAST_SKIP) {
            if (active && !finished && ps.bounce + 1 >= ra.max_depth - 1 && light_is_delta<EXT>(sc.lights[ps.light])) {
                F3 add = div(ps.throughput * ps.Ld, ps.pick_pdf);
                ps.Li = f3(ps.Li.x + add.x, ps.Li.y + add.y, ps.Li.z + add.z);
                finished = true;
            }
        }
        // ---- BSDF sample: the next ray
        if (active && !finished) {
            F3 wi;
            float pdf;
            bool specular;
            bool null_sampled = false;
            F3 f = EXT ? rmat_sample(rmat, fr, wo, u_bsdf_c, u_bsdf_1, u_bsdf_2, &wi, &pdf, &specular, &null_sampled)
                       : mat_sample(*mat, fr, wo, u_bsdf_c, u_bsdf_1, u_bsdf_2, &wi, &pdf, &specular);
            if (EXT && null_sampled && !is_black(f) && pdf > 0.0f) {
                // punch through the mask: throughput *= f / pdf, no cosine, and this bounce's Ld is dropped (:122-136)
                ps.throughput = ps.throughput * div(f, pdf);
                ps.o = fr.p;
                ps.d = wi;
                ps.mint = fr.eps;
                ps.punch = true;
            } else if (!is_black(f) && pdf > 0.0f) {
                float fw = 1.0f;
                if (!specular) fw = power_heuristic(pdf, light_pdf<EXT>(sc, sc.lights[ps.light], fr.p, wi));
                ps.f = f;
                ps.fw = fw;
                ps.bsdf_pdf = pdf;
                ps.cosw = absdot(wi, fr.n);
                ps.o = fr.p;
                ps.d = wi;
                ps.mint = fr.eps;
                if (ra.russian_roulette && !REPLAY && ps.bounce >= 2) {
                    // build-side extension (path_trace_kernel's, restated in oracle/goblin_oracle.cpp russian_roulette)
                    F3 tn = ps.throughput * div(ps.f * ps.cosw, ps.bsdf_pdf);
                    float q = fminf(0.95f, fmaxf(tn.x, fmaxf(tn.y, tn.z)));
                    float u = nat_u01(nat_mix(nat_mix(src.pixel_key, 0xBADC0DEu + ps.bounce), src.k));
                    if (!(u < q)) {
                        // terminate after accounting this vertex's direct light
                        F3 add = div(ps.throughput * ps.Ld, ps.pick_pdf);
                        ps.Li = f3(ps.Li.x + add.x, ps.Li.y + add.y, ps.Li.z + add.z);
                        finished = true;
                    } else {
                        // survivors carry 1/q on what depends on the extension ray, NOT on this vertex's light-sampled term
                        ps.f = ps.f * (1.0f / q);
                    }
                }
            } else {
                // Li += throughput * Ld / pickLightPdf; break   (:163-167)
                F3 add = div(ps.throughput * ps.Ld, ps.pick_pdf);
                ps.Li = f3(ps.Li.x + add.x, ps.Li.y + add.y, ps.Li.z + add.z);
                finished = true;
            }
            query_maxt = INFINITY;   // RayDifferential(p, wi, epsilon): maxt = +inf
        }
        // ---- path end: store and free the lane (a NaN component is stored as it is: the caller drops it, as ImageTile::addSample does)
        if (active && finished) {
            ra.out[idx] = make_float4(ps.Li.x, ps.Li.y, ps.Li.z, 1.0f);
            active = false;
        }
    }
}
