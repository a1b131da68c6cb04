// Stand-alone digest of pack_scene's tables (tests/test_scene_prep_cpu.py): for every scene file on the command line and
// for host- and device-built BLASes, one line per PackedScene member -- a vector's element count and the 64-bit FNV-1a of
// its bytes, a scalar's value.  pack_scene's wall time goes to stderr.  Links scene_prep.cpp and libgoblin_host.so.
#include <chrono>
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../goblin_amd/csrc/scene_prep.h"

static uint64_t fnv1a(const void* p, size_t n) {
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ static_cast<const unsigned char*>(p)[i]) * 1099511628211ull;
    return h;
}
template <class T>
static void vec(const char* name, const std::vector<T>& v) {
    printf("%s %zu %016" PRIx64 "\n", name, v.size(), fnv1a(v.data(), v.size() * sizeof(T)));
}
static void num(const char* name, long long v) { printf("%s = %lld\n", name, v); }
#define VEC(m) vec(#m, s.m)
#define NUM(m) num(#m, static_cast<long long>(s.m))
#define RAW(m) printf(#m " 1 %016" PRIx64 "\n", fnv1a(&s.m, sizeof(s.m)))

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        gbl_host_scene* hs = nullptr;
        if (gbl_host_load_file(argv[a], &hs) != GBL_OK) {
            fprintf(stderr, "%s: %s\n", argv[a], gbl_host_last_error());
            return 1;
        }
        const char* base = strrchr(argv[a], '/') ? strrchr(argv[a], '/') + 1 : argv[a];
        for (int device_blas = 0; device_blas < 2; ++device_blas) {
            PackedScene s;
            memset(s.filter_table, 0, sizeof(s.filter_table));
            memset(&s.camera, 0, sizeof(s.camera));
            memset(&s.film, 0, sizeof(s.film));
            std::string err;
            const auto t0 = std::chrono::steady_clock::now();
            const gbl_status st = pack_scene(gbl_host_desc(hs), &s, &err, device_blas != 0);
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            fprintf(stderr, "time %s device_blas=%d %.3f ms\n", base, device_blas, ms);
            if (st != GBL_OK) {
                fprintf(stderr, "%s: pack_scene: %s\n", argv[a], err.c_str());
                return 1;
            }
            printf("scene %s device_blas=%d\n", base, device_blas);
            VEC(nodes); VEC(tris); VEC(tri_shade); VEC(tri_bounds); VEC(tri_bounds_leaf); VEC(instance_bounds); VEC(tri_order);
            VEC(positions); VEC(normals); VEC(uvs); VEC(instances); VEC(materials); VEC(textures); VEC(images);
            VEC(ewa_lut); VEC(ibl_dist); VEC(vol_density); VEC(lights); VEC(light_tris); VEC(light_cdf); VEC(light_pick_pdf);
            VEC(mesh_stack_need); VEC(mesh_lo); VEC(mesh_hi); VEC(mesh_root);
            RAW(filter_table); RAW(volume); RAW(camera); RAW(film);
            NUM(has_ibl); NUM(tlas_root); NUM(stack_entries); NUM(extended); NUM(scene_extended); NUM(has_masks); NUM(has_bssrdf);
            NUM(wh_slots); NUM(blas_nodes); NUM(tlas_nodes); NUM(blas_max_depth); NUM(tlas_depth); NUM(tlas_base);
            NUM(tlas_capacity); NUM(hot_nodes);
        }
        gbl_host_free(hs);
    }
    return 0;
}
