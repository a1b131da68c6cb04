// Stand-alone checks of the material and texture edits' host arithmetic (tests/test_materials_cpu.py).
//
// materials_repack cases <scenes> <case file>: for each case of tests/material_edit_cases.py a shipped scene is packed, the case's
// edits are applied to the packed `materials` and `textures` tables through repack_materials / repack_textures, and the edited
// description is packed from scratch.  The two tables must be identical byte for byte, every other table and the flags (extended,
// has_masks, has_bssrdf, every instance's is_mask) must not have moved, the edit must have changed something, and the inverse edit
// must restore the first bytes.  One line per case: "case <scene> <name> ok" or "case <scene> <name> FAIL <what>".  Both packings
// run in this one process, so the machine's libm does not enter.  The BLASes are left to the device builder (pack_scene's
// device_blas): these tables do not depend on the trees.
//
// materials_repack compose: kernels/materials.h's mat_compose / tex_compose, compiled for the host, over 10^5 random rows and the
// edge rows -- each applied to a live record of every material type whose editable fields hold other values -- against (a) the
// record pack_scene makes for the patched description and (b) the expressions pack_materials / pack_textures held before the
// compose functions were split out of them, restated here.  NaN payloads are not compared.  "key value" lines.
// Links scene_prep.cpp and, for the cases, libgoblin_host.so.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <limits>
#include <map>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "../goblin_amd/csrc/kernels/materials.h"
#include "../goblin_amd/csrc/scene_prep.h"

namespace {

template <class T>
bool same(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

struct Edit {
    char table;
    uint32_t index;
    std::string field;
    std::vector<double> values;
};

struct Scene {
    gbl_host_scene* host = nullptr;
    const gbl_scene_desc* desc = nullptr;
    PackedScene packed;
    std::vector<gbl_material> materials;
    std::vector<gbl_texture> textures;
};

bool pack(const gbl_scene_desc& d, PackedScene* out, std::string* err) { return pack_scene(&d, out, err, true) == GBL_OK; }

bool apply(const Edit& e, std::vector<gbl_material>& M, std::vector<gbl_texture>& T, std::string* why) {
    const auto floats = [&](float* f, size_t n) {
        if (e.values.size() != n) return false;
        for (size_t k = 0; k < n; ++k) f[k] = static_cast<float>(e.values[k]);
        return true;
    };
    *why = std::string("the case names no such field: ") + e.table + " " + e.field;
    if (e.table == 'm') {
        if (e.index >= M.size()) return false;
        gbl_material& m = M[e.index];
        if (e.field == "color") return floats(m.color, 3);
        if (e.field == "color2") return floats(m.color2, 3);
        if (e.field == "color3") return floats(m.color3, 3);
        if (e.field == "index") return floats(&m.index, 1);
        if (e.field == "k") return floats(&m.k, 1);
        if (e.field == "exponent") return floats(&m.exponent, 1);
        const std::map<std::string, int32_t*> slots = {{"tex_color", &m.tex_color}, {"tex_color2", &m.tex_color2}, {"tex_exponent", &m.tex_exponent},
                                                       {"tex_color3", &m.tex_color3}, {"tex_bump", &m.tex_bump},   {"tex_normal", &m.tex_normal}};
        const auto it = slots.find(e.field);
        if (it == slots.end() || e.values.size() != 1) return false;
        *it->second = static_cast<int32_t>(e.values[0]);
        return true;
    }
    if (e.table != 't' || e.index >= T.size()) return false;
    gbl_texture& t = T[e.index];
    if (e.field == "value") return floats(t.value, 3);
    if (e.field == "uv_scale") return floats(t.uv_scale, 2);
    if (e.field == "uv_offset") return floats(t.uv_offset, 2);
    if (e.field == "max_anisotropy") return floats(&t.max_anisotropy, 1);
    if (e.field == "to_tex") {
        float f[10];
        if (!floats(f, 10)) return false;
        memcpy(t.to_tex.position, f, 12), memcpy(t.to_tex.orientation, f + 3, 16), memcpy(t.to_tex.scale, f + 7, 12);
        return true;
    }
    return false;
}

std::string others_moved(const PackedScene& a, const PackedScene& b) {
    if (!same(a.nodes, b.nodes) || !same(a.tris, b.tris) || !same(a.tri_shade, b.tri_shade) || !same(a.tri_bounds, b.tri_bounds) || !same(a.tri_order, b.tri_order)) return "geometry tables moved";
    if (!same(a.positions, b.positions) || !same(a.normals, b.normals) || !same(a.uvs, b.uvs)) return "vertex attributes moved";
    if (!same(a.instances, b.instances) || !same(a.instance_bounds, b.instance_bounds)) return "instances moved (is_mask among them)";
    if (!same(a.images, b.images) || !same(a.ewa_lut, b.ewa_lut) || !same(a.ibl_dist, b.ibl_dist) || !same(a.vol_density, b.vol_density)) return "image tables moved";
    if (!same(a.lights, b.lights) || !same(a.light_tris, b.light_tris) || !same(a.light_cdf, b.light_cdf) || !same(a.light_pick_pdf, b.light_pick_pdf)) return "light tables moved";
    if (a.extended != b.extended || a.scene_extended != b.scene_extended || a.has_masks != b.has_masks || a.has_bssrdf != b.has_bssrdf || a.has_ibl != b.has_ibl ||
        a.wh_slots != b.wh_slots || a.stack_entries != b.stack_entries || a.tlas_root != b.tlas_root || a.hot_nodes != b.hot_nodes)
        return "extended / has_masks / has_bssrdf / a scalar moved";
    if (memcmp(&a.volume, &b.volume, sizeof(a.volume)) != 0 || memcmp(&a.camera, &b.camera, sizeof(a.camera)) != 0 || memcmp(&a.film, &b.film, sizeof(a.film)) != 0 ||
        memcmp(a.filter_table, b.filter_table, sizeof(a.filter_table)) != 0)
        return "volume / camera / film moved";
    return "";
}

// The packed tables taken from `from`'s description to `to`'s through the repackers, over the contiguous ranges the edits span
void repack(const std::vector<Edit>& edits, const std::vector<gbl_material>& M, const std::vector<gbl_texture>& T, std::vector<DevMaterial>* dm, std::vector<DevTexture>* dt) {
    for (char table : {'m', 't'}) {
        uint32_t lo = UINT32_MAX, hi = 0;
        for (const Edit& e : edits)
            if (e.table == table) lo = std::min(lo, e.index), hi = std::max(hi, e.index);
        if (lo == UINT32_MAX) continue;
        std::vector<uint32_t> touched;
        if (table == 'm') repack_materials(M.data(), static_cast<uint32_t>(M.size()), lo, hi - lo + 1, dm, &touched);
        else repack_textures(T.data() + lo, lo, hi - lo + 1, dt);
    }
}

std::string run(const Scene& s, const std::vector<Edit>& edits) {
    std::vector<gbl_material> M = s.materials;
    std::vector<gbl_texture> T = s.textures;
    std::string why;
    for (const Edit& e : edits)
        if (!apply(e, M, T, &why)) return why;
    std::vector<DevMaterial> dm = s.packed.materials;
    std::vector<DevTexture> dt = s.packed.textures;
    repack(edits, M, T, &dm, &dt);
    gbl_scene_desc d = *s.desc;
    d.materials = M.data(), d.textures = T.data();
    PackedScene fresh;
    std::string err;
    if (!pack(d, &fresh, &err)) return "pack_scene refused the edited description: " + err;
    if (!same(dm, fresh.materials)) return "materials differ from the fresh packing";
    if (!same(dt, fresh.textures)) return "textures differ from the fresh packing";
    if (!(why = others_moved(fresh, s.packed)).empty()) return why;
    if (same(dm, s.packed.materials) && same(dt, s.packed.textures)) return "the edit changed nothing";
    repack(edits, s.materials, s.textures, &dm, &dt);
    if (!same(dm, s.packed.materials) || !same(dt, s.packed.textures)) return "the inverse edit does not restore the first bytes";
    return "";
}

int run_cases(const char* scenes, const char* case_file) {
    std::ifstream in(case_file);
    std::map<std::string, Scene> open;
    std::string line, scene, name;
    std::vector<Edit> edits;
    int failed = 0;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string word;
        ls >> word;
        if (word == "case") {
            ls >> scene >> name;
            edits.clear();
        } else if (word == "m" || word == "t") {
            Edit e;
            size_t n = 0;
            e.table = word[0];
            ls >> e.index >> e.field >> n;
            for (size_t k = 0; k < n; ++k) {
                std::string v;
                ls >> v;
                e.values.push_back(strtod(v.c_str(), nullptr));
            }
            edits.push_back(e);
        } else if (word == "end") {
            Scene& s = open[scene];
            if (!s.host) {
                const std::string path = std::string(scenes) + "/" + scene + ".json";
                std::string err;
                if (gbl_host_load_file(path.c_str(), &s.host) != GBL_OK) {
                    fprintf(stderr, "%s: %s\n", path.c_str(), gbl_host_last_error());
                    return 1;
                }
                s.desc = gbl_host_desc(s.host);
                s.materials.assign(s.desc->materials, s.desc->materials + s.desc->num_materials);
                s.textures.assign(s.desc->textures, s.desc->textures + s.desc->num_textures);
                if (!pack(*s.desc, &s.packed, &err)) {
                    fprintf(stderr, "%s: pack_scene: %s\n", path.c_str(), err.c_str());
                    return 1;
                }
            }
            const std::string what = run(s, edits);
            printf("case %s %s %s%s\n", scene.c_str(), name.c_str(), what.empty() ? "ok" : "FAIL ", what.c_str());
            failed += !what.empty();
        }
    }
    for (auto& kv : open) gbl_host_free(kv.second.host);
    printf("failed %d\n", failed);
    return 0;
}

// ---------------------------------------------------------------- the compose functions
uint32_t bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
bool same_float(float a, float b) { return (std::isnan(a) && std::isnan(b)) || bits(a) == bits(b); }

// What pack_materials wrote into the editable fields before mat_compose was split out of it
void expected_material(const gbl_material& m, DevMaterial* dm) {
    for (int k = 0; k < 3; ++k) dm->color[k] = m.color[k], dm->color2[k] = m.color2[k];
    dm->index = m.index;
    dm->k = m.k;
    dm->exponent = m.exponent;
    if (m.type == GBL_MAT_SUBSURFACE) {
        for (int k = 0; k < 3; ++k) dm->color3[k] = m.color3[k];
        const float eta = m.index;
        const float fdr = eta < 1.0f ? -0.4399f + 0.7099f / eta - 0.3319f / (eta * eta) + 0.0636f / (eta * eta * eta)
                                     : -1.4399f / (eta * eta) + 0.7099f / eta + 0.6681f + 0.0636f * eta;
        dm->exponent = (1.0f + fdr) / (1.0f - fdr);
    }
}

bool same_material(const DevMaterial& a, const DevMaterial& b) {
    DevMaterial x = a, y = b;
    float* fx[] = {x.color, x.color2, x.color3, &x.index};   // (index, k, exponent lie behind one another)
    float* fy[] = {y.color, y.color2, y.color3, &y.index};
    for (int g = 0; g < 4; ++g)
        for (int k = 0; k < 3; ++k) {
            if (!same_float(fx[g][k], fy[g][k])) return false;
            fx[g][k] = fy[g][k] = 0.0f;
        }
    return memcmp(&x, &y, sizeof(x)) == 0;
}

bool same_texture(const DevTexture& a, const DevTexture& b) {
    DevTexture x = a, y = b;
    for (int k = 0; k < 3; ++k) {
        if (!same_float(x.value[k], y.value[k])) return false;
        x.value[k] = y.value[k] = 0.0f;
    }
    for (int k = 0; k < 2; ++k) {
        if (!same_float(x.uv_scale[k], y.uv_scale[k]) || !same_float(x.uv_offset[k], y.uv_offset[k])) return false;
        x.uv_scale[k] = y.uv_scale[k] = x.uv_offset[k] = y.uv_offset[k] = 0.0f;
    }
    return memcmp(&x, &y, sizeof(x)) == 0;
}

int run_compose() {
    // a description of one material per type (a mask wraps the lambert one, slots of both kinds occupied) and three textures
    std::vector<gbl_material> M(6);
    std::vector<gbl_texture> T(3);
    memset(M.data(), 0, M.size() * sizeof(gbl_material));
    memset(T.data(), 0, T.size() * sizeof(gbl_texture));
    for (uint32_t i = 0; i < 6; ++i) {
        gbl_material& m = M[i];
        m.type = i;
        m.tex_color = m.tex_color2 = m.tex_exponent = m.tex_color3 = m.tex_bump = m.tex_normal = m.masked_material = -1;
        for (int k = 0; k < 3; ++k) m.color[k] = 0.25f, m.color2[k] = 0.5f, m.color3[k] = 0.75f;
        m.index = 1.5f, m.k = 0.125f, m.exponent = 7.0f;
    }
    M[GBL_MAT_MASK].masked_material = GBL_MAT_LAMBERT;
    M[GBL_MAT_LAMBERT].tex_color = 0, M[GBL_MAT_BLINN].tex_exponent = 1, M[GBL_MAT_SUBSURFACE].tex_color3 = 2, M[GBL_MAT_LAMBERT].tex_bump = 1;
    for (gbl_texture& t : T) t.child[0] = t.child[1] = t.image = -1, t.uv_scale[0] = t.uv_scale[1] = 1.0f;
    T[1].is_float = 1u;
    T[2].type = GBL_TEX_CHECKERBOARD, T[2].child[0] = T[2].child[1] = 0, T[2].mapping = GBL_MAP_SPHERICAL;
    T[2].to_tex.orientation[0] = T[2].to_tex.scale[0] = T[2].to_tex.scale[1] = T[2].to_tex.scale[2] = 1.0f;
    std::vector<std::vector<float>> rows;
    std::mt19937 rng(20261021u);
    std::uniform_real_distribution<float> unit(0.0f, 1.0f), wide(-8.0f, 8.0f);
    for (int i = 0; i < 100000; ++i) {
        std::vector<float> r(12);
        for (float& f : r) f = (i & 1) ? unit(rng) * 4.0f : std::exp(wide(rng)) * (unit(rng) < 0.25f ? -1.0f : 1.0f);
        if (i % 3 == 0) r[9] = 0.25f + 2.5f * unit(rng);   // a third of the indices around 1: both branches of the polynomial
        rows.push_back(r);
    }
    const size_t random_rows = rows.size();
    const float denorm = std::numeric_limits<float>::denorm_min(), big = std::numeric_limits<float>::max(), tiny = std::numeric_limits<float>::min();
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (float eta : {1.0f, std::nextafter(1.0f, 0.0f), std::nextafter(1.0f, 2.0f), 0.5f, 0.9f, 1.3f, 1.5f, 3.0f, 0.0f, -0.0f, -1.5f, denorm, -denorm, tiny, 1e-20f, 1e-13f,
                      1e13f, big, -big, inf, -inf, nan})
        for (float fill : {0.0f, -0.0f, denorm, tiny, 1.0f, big, -big}) {
            std::vector<float> r(12, fill);
            r[9] = eta;
            rows.push_back(r);
        }
    long differs_pack = 0, differs_expected = 0, differs_tex = 0, below = 0, above = 0, cases = 0, tex_cases = 0;
    for (size_t n = 0; n < rows.size(); ++n) {
        const std::vector<float>& r = rows[n];
        if (r[9] < 1.0f) ++below;
        if (r[9] > 1.0f) ++above;
        std::vector<gbl_material> P = M;
        for (gbl_material& m : P) {
            memcpy(m.color, &r[0], 12), memcpy(m.color2, &r[3], 12), memcpy(m.color3, &r[6], 12);
            m.index = r[9], m.k = r[10], m.exponent = r[11];
        }
        std::vector<gbl_texture> Q = T;
        for (gbl_texture& t : Q) memcpy(t.value, &r[0], 12), memcpy(t.uv_scale, &r[3], 8), memcpy(t.uv_offset, &r[5], 8);
        // (a) the packer on the patched description, through the functions gbl_create and the host edits use
        std::vector<DevMaterial> live(M.size()), want(M.size());
        std::vector<DevTexture> tlive(T.size()), twant(T.size());
        std::vector<uint32_t> touched;
        repack_materials(M.data(), 6, 0, 6, &live, &touched);
        repack_materials(P.data(), 6, 0, 6, &want, &touched);
        repack_textures(T.data(), 0, 3, &tlive);
        repack_textures(Q.data(), 0, 3, &twant);
        for (uint32_t i = 0; i < 6; ++i, ++cases) {
            DevMaterial got = live[i];   // the kernel's lane: the live record in, the row's editable fields, the record out
            mat_compose(&got, r.data());
            if (!same_material(got, want[i])) ++differs_pack;
            // (b) the packer's expressions as they stood
            DevMaterial exp = live[i];
            expected_material(P[i], &exp);
            if (!same_material(got, exp)) ++differs_expected;
            if (i != GBL_MAT_SUBSURFACE && (got.color3[0] != 0.0f || got.color3[1] != 0.0f || got.color3[2] != 0.0f)) ++differs_expected;
        }
        for (uint32_t i = 0; i < 3; ++i, ++tex_cases) {
            DevTexture got = tlive[i];
            tex_compose(&got, r.data());
            DevTexture exp = tlive[i];
            for (int k = 0; k < 3; ++k) exp.value[k] = Q[i].is_float ? Q[i].value[0] : Q[i].value[k];
            for (int k = 0; k < 2; ++k) exp.uv_scale[k] = Q[i].uv_scale[k], exp.uv_offset[k] = Q[i].uv_offset[k];
            if (!same_texture(got, twant[i]) || !same_texture(got, exp)) ++differs_tex;
        }
    }
    printf("random_rows %zu\nedge_rows %zu\nmaterial_cases %ld\ntexture_cases %ld\nindex_below_one %ld\nindex_above_one %ld\n", random_rows, rows.size() - random_rows, cases,
           tex_cases, below, above);
    printf("differs_from_the_packer %ld\ndiffers_from_the_former_expressions %ld\ntexture_differs %ld\n", differs_pack, differs_expected, differs_tex);
    return 0;
}

}   // namespace

int main(int argc, char** argv) {
    if (argc == 4 && std::string(argv[1]) == "cases") return run_cases(argv[2], argv[3]);
    if (argc == 2 && std::string(argv[1]) == "compose") return run_compose();
    return 2;
}
