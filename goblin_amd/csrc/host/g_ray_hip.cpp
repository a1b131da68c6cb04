// g_ray_hip <scene.json> [--device N] [--seed S] [--sampler native|stream] [--out file.{exr,ppm,pfm}] [--aov] [--denoise[=N]]
//
// --denoise[=N] also writes <output stem>.denoised.<ext>: the film filtered by gbl_film_denoise at N levels (default 5), guided
// by the feature films of gbl_render_aov and, where the frame's per-sample radiance (16 bytes per camera sample) fits the
// library's per-sample budget, by gbl_film_variance of it; otherwise without a variance plane, which it says on stderr.  The
// denoised film goes through the same develop and write path as the image; the image itself does not change.  Native sampler only.
//
// --aov also writes the first-hit feature films (gbl_render_aov) of the same camera samples beside the image:
// <output stem>.albedo.pfm, .normal.pfm (both normalised) and .depth.pfm (r = depth, g = coverage, b = 0).  Portable float
// maps are lossless; the EXR writer stores halves and would quantise depth.  Native sampler only.
//
// --sampler stream renders with the reference's own sample stream (GBL_SAMPLES_STREAM): the image is the one the
// reference binary writes for this scene file, up to float summation order; native (default) is the fast sampler.
//
// Stand-alone host with the call shape of the reference's g_ray
// (/root/reference/src/g_ray.cpp:7-27): load the scene, render it, and run
// Film::writeImage's tail (GoblinFilm.cpp:164-198): normalise, bloom, write the
// film's "file" (default <scene>.exr, HALF B/G/R).  The tail runs on the device
// (gbl_film_develop): a .ppm downloads bytes, .exr / .pfm the floats.  Everything
// goes through the C ABI of include/goblin_hip.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/goblin_hip.h"

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "Usage: g_ray_hip scene_file.json [--device N] [--seed S] [--sampler native|stream] [--out image.{exr,ppm,pfm}] [--aov] [--denoise[=N]]\n");
        return 0;
    }
    std::string scene_path = argv[1], out_path;
    int device = 0;
    unsigned long long seed = 0;
    bool stream_sampler = false, aov = false;
    int denoise = 0;   // levels; 0: off
    for (int i = 2; i < argc; i += 2) {
        if (!strcmp(argv[i], "--aov")) {   // (the switches without a separate value)
            aov = true;
            i -= 1;
            continue;
        }
        if (!strncmp(argv[i], "--denoise", 9) && (argv[i][9] == 0 || argv[i][9] == '=')) {
            denoise = argv[i][9] ? atoi(argv[i] + 10) : 5;
            if (denoise < 1 || denoise > 8) {
                fprintf(stderr, "--denoise takes 1..8 levels\n");
                return 1;
            }
            i -= 1;
            continue;
        }
        if (i + 1 >= argc) break;
        if (!strcmp(argv[i], "--device")) device = atoi(argv[i + 1]);
        else if (!strcmp(argv[i], "--seed")) seed = strtoull(argv[i + 1], nullptr, 10);
        else if (!strcmp(argv[i], "--out")) out_path = argv[i + 1];
        else if (!strcmp(argv[i], "--sampler")) stream_sampler = !strcmp(argv[i + 1], "stream");
    }
    if (aov && stream_sampler) {   // (gbl_render_aov refuses GBL_SAMPLES_STREAM: say so before rendering anything)
        fprintf(stderr, "--aov needs the native sampler\n");
        return 1;
    }
    if (denoise && stream_sampler) {
        fprintf(stderr, "--denoise needs the native sampler\n");
        return 1;
    }
    gbl_host_scene* hs = nullptr;
    if (gbl_host_load_file(scene_path.c_str(), &hs) != GBL_OK) {
        fprintf(stderr, "load failed: %s\n", gbl_host_last_error());
        return 1;
    }
    const gbl_scene_desc* desc = gbl_host_desc(hs);
    if (out_path.empty()) out_path = gbl_host_output_path(hs);
    gbl_ctx* ctx = nullptr;
    if (gbl_create(desc, device, &ctx) != GBL_OK) {
        fprintf(stderr, "gbl_create failed: %s\n", gbl_last_error(nullptr));
        return 1;
    }
    gbl_info info;
    gbl_get_info(ctx, &info);
    size_t npix = static_cast<size_t>(info.xres) * info.yres;
    float *accum = nullptr, *rgb = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&accum), npix * 4 * sizeof(float)) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&rgb), npix * 3 * sizeof(float)) != hipSuccess) {
        fprintf(stderr, "hipMalloc failed\n");
        return 1;
    }
    (void)hipMemset(accum, 0, npix * 4 * sizeof(float));
    gbl_render_params p;
    memset(&p, 0, sizeof(p));
    p.integrator = desc->setting.integrator;
    p.sample_per_pixel = desc->setting.sample_per_pixel;
    p.max_ray_depth = desc->setting.max_ray_depth;
    p.ao_sample_num = desc->setting.ao_sample_num;
    p.bssrdf_sample_num = desc->setting.bssrdf_sample_num;
    p.sample_mode = GBL_SAMPLES_NATIVE;
    p.seed = seed;
    // --denoise: keep the per-sample radiance of the one render below where it fits the budget gbl_render itself keeps its
    // per-sample buffer inside.  The rule restated here is li_budget_bytes() of api_render.hip -- a quarter of the device's memory,
    // at least 1 GiB, GBL_LI_BUDGET_MB instead when set -- and has to follow it: inside that budget plan_render defers the splat
    // (`defer`) with or without li_out and choose_schedule does not split the call into passes, so the call runs under the
    // schedule it would run under without li_out (tests/test_gpu_denoise.py holds the two calls to one schedule and one film).
    float* li = nullptr;
    if (denoise) {
        const unsigned long long spp = static_cast<unsigned long long>(gbl_host_round_to_square(p.sample_per_pixel));
        const unsigned long long li_bytes = static_cast<unsigned long long>(info.window[1] - info.window[0]) * (info.window[3] - info.window[2]) * spp * 16ull;
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || total_b == 0) total_b = 8ull << 30;
        unsigned long long budget = std::max<unsigned long long>(1ull << 30, total_b / 4);
        if (const char* e = getenv("GBL_LI_BUDGET_MB")) budget = std::max<unsigned long long>(1ull << 20, strtoull(e, nullptr, 10) << 20);
        if (spp >= 2 && li_bytes <= budget && hipMalloc(reinterpret_cast<void**>(&li), li_bytes) == hipSuccess) {
            (void)hipMemset(li, 0, li_bytes);
            p.li_out = li;
        } else {
            li = nullptr;
            fprintf(stderr, "--denoise: the per-sample radiance (%llu bytes) is not kept: filtering without a variance plane\n", li_bytes);
        }
    }
    gbl_stats st;
    auto t0 = std::chrono::steady_clock::now();
    if (stream_sampler) {
        // bands of whole tile rows, sized so a band's per-sample buffers stay near 1 GiB
        p.sample_mode = GBL_SAMPLES_STREAM;
        const int spp = gbl_host_round_to_square(p.sample_per_pixel);
        const long long row_samples = static_cast<long long>(info.window[1] - info.window[0]) * spp;
        int band = static_cast<int>(std::max<long long>(8, ((1ll << 26) / std::max<long long>(1, row_samples)) / 8 * 8));
        gbl_stats total;
        memset(&total, 0, sizeof(total));
        for (int y = info.window[2]; y < info.window[3]; y += band) {
            p.window[0] = info.window[0];
            p.window[1] = info.window[1];
            p.window[2] = y;
            p.window[3] = std::min(y + band, info.window[3]);
            if (gbl_render(ctx, &p, accum, &st) != GBL_OK) {
                fprintf(stderr, "gbl_render failed: %s\n", gbl_last_error(ctx));
                return 1;
            }
            total.paths += st.paths;
            total.kernel_ms += st.kernel_ms;
        }
        st = total;
    } else if (gbl_render(ctx, &p, accum, &st) != GBL_OK) {
        fprintf(stderr, "gbl_render failed: %s\n", gbl_last_error(ctx));
        return 1;
    }
    (void)hipDeviceSynchronize();
    double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();   // the render; developing the film is not in it
    if (aov) {
        // the three feature films of the very samples rendered above, resolved on the device, written as portable float maps
        float* feat = nullptr;   // 3 accumulators, then depth and coverage
        if (hipMalloc(reinterpret_cast<void**>(&feat), npix * 14 * sizeof(float)) != hipSuccess) {
            fprintf(stderr, "hipMalloc failed\n");
            return 1;
        }
        (void)hipMemset(feat, 0, npix * 12 * sizeof(float));
        gbl_aov_targets tg;
        memset(&tg, 0, sizeof(tg));
        tg.albedo_accum = feat;
        tg.normal_accum = feat + 4 * npix;
        tg.depth_accum = feat + 8 * npix;
        gbl_render_params ap = p;
        ap.li_out = nullptr;
        memset(ap.window, 0, sizeof(ap.window));
        if (gbl_render_aov(ctx, &ap, &tg, nullptr) != GBL_OK) {
            fprintf(stderr, "gbl_render_aov failed: %s\n", gbl_last_error(ctx));
            return 1;
        }
        const size_t dot_a = out_path.rfind("."), slash = out_path.rfind("/");
        const std::string stem = (dot_a == std::string::npos || (slash != std::string::npos && dot_a < slash)) ? out_path : out_path.substr(0, dot_a);
        std::vector<float> host(npix * 3), dc(npix * 2);
        float* const films[2] = {tg.albedo_accum, tg.normal_accum};
        const char* const names[2] = {".albedo.pfm", ".normal.pfm"};
        for (int f = 0; f < 2; ++f) {
            if (gbl_film_resolve(ctx, films[f], rgb, nullptr) != GBL_OK) {
                fprintf(stderr, "gbl_film_resolve failed: %s\n", gbl_last_error(ctx));
                return 1;
            }
            (void)hipMemcpy(host.data(), rgb, host.size() * sizeof(float), hipMemcpyDeviceToHost);
            if (gbl_host_write_pfm((stem + names[f]).c_str(), host.data(), info.xres, info.yres) != GBL_OK) {
                fprintf(stderr, "write failed: %s\n", gbl_host_last_error());
                return 1;
            }
        }
        if (gbl_aov_resolve_depth(ctx, tg.depth_accum, feat + 12 * npix, feat + 13 * npix, nullptr) != GBL_OK) {
            fprintf(stderr, "gbl_aov_resolve_depth failed: %s\n", gbl_last_error(ctx));
            return 1;
        }
        (void)hipMemcpy(dc.data(), feat + 12 * npix, dc.size() * sizeof(float), hipMemcpyDeviceToHost);
        for (size_t i = 0; i < npix; ++i) {
            host[3 * i] = dc[i];
            host[3 * i + 1] = dc[npix + i];
            host[3 * i + 2] = 0.0f;
        }
        if (gbl_host_write_pfm((stem + ".depth.pfm").c_str(), host.data(), info.xres, info.yres) != GBL_OK) {
            fprintf(stderr, "write failed: %s\n", gbl_host_last_error());
            return 1;
        }
        printf("write feature films to : %s.{albedo,normal,depth}.pfm\n", stem.c_str());
        (void)hipFree(feat);
    }
    // Goblin::writeImage's dispatch (GoblinImageIO.cpp:146-167): .ppm is tone-mapped (when the film asks) and quantised,
    // .exr (and .pfm) get the floats as they are, anything else becomes <name>.ppm without tone mapping
    const size_t dot = out_path.rfind(".");
    const std::string ext = dot == std::string::npos ? std::string() : out_path.substr(dot);
    const bool is_ppm = ext == ".ppm" || ext == ".PPM";
    const bool floats = ext == ".exr" || ext == ".EXR" || ext == ".pfm" || ext == ".PFM";
    uint8_t* rgb8 = nullptr;
    if (!floats && hipMalloc(reinterpret_cast<void**>(&rgb8), npix * 3) != hipSuccess) {
        fprintf(stderr, "hipMalloc failed\n");
        return 1;
    }
    // develops a film and writes it: the image, and the denoised film beside it
    const auto develop_and_write = [&](const float* film, const std::string& path) -> bool {
        gbl_develop_params dp;
        memset(&dp, 0, sizeof(dp));
        dp.bloom_radius = desc->film.bloom_radius;
        dp.bloom_weight = desc->film.bloom_weight;
        dp.tone_mapping = is_ppm ? desc->film.tone_mapping : 0u;
        if (gbl_film_develop(ctx, film, &dp, floats ? rgb : nullptr, rgb8) != GBL_OK) {
            fprintf(stderr, "gbl_film_develop failed: %s\n", gbl_last_error(ctx));
            return false;
        }
        (void)hipDeviceSynchronize();
        gbl_status wst;
        if (floats) {
            std::vector<float> host(npix * 3);
            (void)hipMemcpy(host.data(), rgb, host.size() * sizeof(float), hipMemcpyDeviceToHost);
            wst = gbl_host_write_image(path.c_str(), host.data(), info.xres, info.yres, 0);
        } else {
            std::vector<uint8_t> host(npix * 3);
            (void)hipMemcpy(host.data(), rgb8, host.size(), hipMemcpyDeviceToHost);
            wst = gbl_host_write_ppm8((is_ppm ? path : path + ".ppm").c_str(), host.data(), info.xres, info.yres);
        }
        if (wst != GBL_OK) {
            fprintf(stderr, "write failed: %s\n", gbl_host_last_error());
            return false;
        }
        return true;
    };
    if (denoise) {
        // feature films of the very samples rendered above, the variance of the pixel mean where li was kept, the filter
        float* work = nullptr;   // 3 feature accumulators, the denoised film, the variance plane
        if (hipMalloc(reinterpret_cast<void**>(&work), npix * 17 * sizeof(float)) != hipSuccess) {
            fprintf(stderr, "hipMalloc failed\n");
            return 1;
        }
        (void)hipMemset(work, 0, npix * 17 * sizeof(float));
        gbl_aov_targets tg;
        memset(&tg, 0, sizeof(tg));
        tg.albedo_accum = work;
        tg.normal_accum = work + 4 * npix;
        tg.depth_accum = work + 8 * npix;
        float* const denoised = work + 12 * npix;
        float* const variance = li ? work + 16 * npix : nullptr;
        gbl_render_params ap = p;
        ap.li_out = nullptr;
        memset(ap.window, 0, sizeof(ap.window));
        if (gbl_render_aov(ctx, &ap, &tg, nullptr) != GBL_OK) {
            fprintf(stderr, "gbl_render_aov failed: %s\n", gbl_last_error(ctx));
            return 1;
        }
        if (li && gbl_film_variance(ctx, li, ap.window, p.sample_per_pixel, variance, nullptr) != GBL_OK) {
            fprintf(stderr, "gbl_film_variance failed: %s\n", gbl_last_error(ctx));
            return 1;
        }
        gbl_denoise_params np;
        memset(&np, 0, sizeof(np));
        np.iterations = denoise;
        np.sigma_luminance = 4.0f;
        np.sigma_normal = 0.5f;
        np.sigma_albedo = 0.1f;
        np.sigma_depth = 0.1f;
        np.demodulate = 1;
        if (gbl_film_denoise(ctx, accum, variance, tg.albedo_accum, tg.normal_accum, tg.depth_accum, &np, denoised) != GBL_OK) {
            fprintf(stderr, "gbl_film_denoise failed: %s\n", gbl_last_error(ctx));
            return 1;
        }
        const size_t slash = out_path.rfind("/");
        const bool has_ext = dot != std::string::npos && (slash == std::string::npos || dot > slash);
        const std::string dn_path = has_ext ? out_path.substr(0, dot) + ".denoised" + ext : out_path + ".denoised";
        if (!develop_and_write(denoised, dn_path)) return 1;
        printf("write denoised image to : %s\n", dn_path.c_str());
        (void)hipFree(work);
        if (li) (void)hipFree(li);
    }
    if (!develop_and_write(accum, out_path)) return 1;
    printf("Render Complete!\n%llu paths in %.3f s (kernel %.3f ms, %.1f Mpaths/s)\nwrite image to : %s\n",
           static_cast<unsigned long long>(st.paths), sec, st.kernel_ms, st.paths / (st.kernel_ms * 1e3), out_path.c_str());
    (void)hipFree(accum);
    (void)hipFree(rgb);
    if (rgb8) (void)hipFree(rgb8);
    gbl_destroy(ctx);
    gbl_host_free(hs);
    return 0;
}
