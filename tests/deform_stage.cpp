// TEST INFRASTRUCTURE (tests/test_deform_cpu.py): drives goblin_amd/csrc/motion_stage.cpp, the host side of
// gbl_render_motion_deform's previous poses, stand-alone -- no HIP, no library.  Built with g++ -fsanitize=address,undefined.
//
//   deform_stage JOB      JOB: little-endian words.  u32 num_meshes, then {vertex_offset, vertex_count, shape} per mesh;
//                         u32 num_vertices, then 3 floats per vertex (the context's positions); u32 list_is_null, u32 num_prev,
//                         then per entry {mesh, reserved, positions_is_null, num_floats} and num_floats floats.
//   stdout                "ok 1", "table <int32 per mesh>", "packed <u32 word per float, hex>"; or "ok 0" and "err <message>"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../goblin_amd/csrc/motion_stage.h"

namespace {

bool read_words(FILE* f, void* out, size_t count) { return fread(out, 4, count, f) == count; }

}   // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t num_meshes = 0, num_vertices = 0, list_is_null = 0, num_prev = 0;
    if (!read_words(f, &num_meshes, 1)) return 2;
    std::vector<gbl_mesh> meshes(num_meshes);
    for (gbl_mesh& gm : meshes) {
        uint32_t w[3];
        if (!read_words(f, w, 3)) return 2;
        memset(&gm, 0, sizeof(gm));
        gm.vertex_offset = w[0];
        gm.vertex_count = w[1];
        gm.shape = w[2];
    }
    if (!read_words(f, &num_vertices, 1)) return 2;
    std::vector<float> positions(3 * static_cast<size_t>(num_vertices));
    if (!positions.empty() && !read_words(f, positions.data(), positions.size())) return 2;
    if (!read_words(f, &list_is_null, 1) || !read_words(f, &num_prev, 1)) return 2;
    std::vector<gbl_motion_mesh> prev(list_is_null ? 0 : num_prev);
    std::vector<std::vector<float>> held(prev.size());   // exactly as long as the job says: a read past the end is the sanitizer's to find
    for (size_t k = 0; k < prev.size(); ++k) {
        uint32_t w[4];
        if (!read_words(f, w, 4)) return 2;
        held[k].resize(w[3]);
        if (w[3] > 0 && !read_words(f, held[k].data(), w[3])) return 2;
        prev[k].mesh = w[0];
        prev[k].reserved = w[1];
        prev[k].positions = w[2] ? nullptr : held[k].data();
    }
    fclose(f);
    MotionStage stage;
    std::string err;
    const bool ok = stage_motion_meshes(meshes.data(), meshes.size(), positions.data(), list_is_null ? nullptr : prev.data(), num_prev,
                                        "gbl_render_motion_deform", &stage, &err);
    printf("ok %d\n", ok ? 1 : 0);
    if (!ok) {
        printf("err %s\n", err.c_str());
        return 0;
    }
    printf("table");
    for (int32_t v : stage.table) printf(" %d", v);
    printf("\npacked");
    for (float v : stage.packed) {
        uint32_t w;
        memcpy(&w, &v, 4);
        printf(" %08x", w);
    }
    printf("\n");
    return 0;
}
