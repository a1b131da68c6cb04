// Stand-alone dump for tests/test_refit_cpu.py: packs the scene file argv[2] with the host builder and writes, into the
// directory argv[1], the tables a vertex edit touches -- nodes, tris, tri_bounds_leaf, tri_shade, positions, mesh_root,
// hot_nodes, `meshes` (per mesh: shape, vertex_offset, vertex_count, tri_offset, tri_count, first record of tris) -- and per
// triangle mesh m the plan goblin_amd/csrc/scene_refit.cpp builds: plan_<m> (RefitRecord) and levels_<m> (level_first).
// Links scene_prep.cpp, scene_refit.cpp and libgoblin_host.so.
#include <cstdio>
#include <cstring>
#include <string>

#include "../goblin_amd/csrc/scene_prep.h"
#include "../goblin_amd/csrc/scene_refit.h"

static bool put(const std::string& dir, const std::string& name, const void* p, size_t bytes) {
    FILE* f = fopen((dir + "/" + name).c_str(), "wb");
    if (!f) return false;
    const bool ok = bytes == 0 || fwrite(p, 1, bytes, f) == bytes;
    return fclose(f) == 0 && ok;
}
template <class T>
static bool put(const std::string& dir, const std::string& name, const std::vector<T>& v) {
    return put(dir, name, v.data(), v.size() * sizeof(T));
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: refit_dump OUT_DIR SCENE.json\n");
        return 2;
    }
    const std::string dir = argv[1];
    gbl_host_scene* hs = nullptr;
    if (gbl_host_load_file(argv[2], &hs) != GBL_OK) {
        fprintf(stderr, "%s: %s\n", argv[2], gbl_host_last_error());
        return 1;
    }
    const gbl_scene_desc* d = gbl_host_desc(hs);
    PackedScene s;
    memset(s.filter_table, 0, sizeof(s.filter_table));
    memset(&s.camera, 0, sizeof(s.camera));
    memset(&s.film, 0, sizeof(s.film));
    std::string err;
    if (pack_scene(d, &s, &err, false) != GBL_OK) {
        fprintf(stderr, "%s: pack_scene: %s\n", argv[2], err.c_str());
        return 1;
    }
    bool ok = put(dir, "nodes", s.nodes) && put(dir, "tris", s.tris) && put(dir, "tri_bounds_leaf", s.tri_bounds_leaf) && put(dir, "tri_shade", s.tri_shade) &&
              put(dir, "positions", s.positions) && put(dir, "mesh_root", s.mesh_root) && put(dir, "hot_nodes", &s.hot_nodes, sizeof(s.hot_nodes));
    std::vector<uint32_t> meshes;
    uint32_t tri_first = 0;
    for (uint32_t m = 0; m < d->num_meshes && ok; ++m) {
        const gbl_mesh& gm = d->meshes[m];
        const bool mesh = gm.shape == GBL_SHAPE_MESH;
        const uint32_t row[6] = {gm.shape, gm.vertex_offset, gm.vertex_count, gm.tri_offset, gm.tri_count, mesh ? tri_first : 0u};
        meshes.insert(meshes.end(), row, row + 6);
        if (!mesh) continue;
        RefitPlan plan;
        if (!build_refit_plan(s.nodes.data(), s.nodes.size(), s.mesh_root[m], tri_first, gm.tri_count, &plan, &err)) {
            fprintf(stderr, "%s: mesh %u: %s\n", argv[2], m, err.c_str());
            return 1;
        }
        ok = put(dir, "plan_" + std::to_string(m), plan.records) && put(dir, "levels_" + std::to_string(m), plan.level_first);
        tri_first += gm.tri_count;
    }
    ok = ok && put(dir, "meshes", meshes);
    gbl_host_free(hs);
    if (!ok) fprintf(stderr, "cannot write into %s\n", dir.c_str());
    return ok ? 0 : 1;
}
