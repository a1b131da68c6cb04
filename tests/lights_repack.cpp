// Stand-alone check of repack_lights against pack_scene (tests/test_lights_cpu.py): for each case a shipped scene is packed,
// one edit is applied to the packed light tables through repack_lights, and the edited description is packed from scratch.  The
// two `lights`, `light_cdf` and `light_pick_pdf` tables must be identical byte for byte, light_tris, ibl_dist, wh_slots, extended
// and has_ibl must not have moved, and the inverse edit must restore the first bytes.  One line per case: "case <scene> <name> ok"
// or "case <scene> <name> FAIL <what>".  Both packings run in this one process, so the machine's libm does not enter.  The
// BLASes are left to the device builder (pack_scene's device_blas): the light tables do not depend on the trees.
// argv[1]: the directory of the shipped scenes.  Links scene_prep.cpp and libgoblin_host.so.
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../goblin_amd/csrc/scene_prep.h"

namespace {

template <class T>
bool same(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

struct Tables {
    std::vector<DevLight> lights;
    std::vector<float> power, cdf, pick;
};

typedef std::function<void(std::vector<gbl_light>&)> Edit;

struct Scene {
    std::string name;
    gbl_host_scene* host = nullptr;
    const gbl_scene_desc* desc = nullptr;
    PackedScene packed;
    std::vector<gbl_light> lights;
};

bool pack(const gbl_scene_desc& d, PackedScene* out, std::string* err) { return pack_scene(&d, out, err, true) == GBL_OK; }

// The description with its lights replaced and every instance that emits through a moved area light moved along
bool pack_edited(const Scene& s, const std::vector<gbl_light>& lights, PackedScene* out, std::string* err) {
    gbl_scene_desc d = *s.desc;
    std::vector<gbl_instance> inst(d.instances, d.instances + d.num_instances);
    for (gbl_instance& gi : inst)
        if (gi.area_light >= 0 && memcmp(&gi.to_world, &s.lights[gi.area_light].to_world, sizeof(gbl_trs)) == 0) gi.to_world = lights[gi.area_light].to_world;
    d.lights = lights.data();
    d.instances = inst.data();
    return pack(d, out, err);
}

std::string compare(const Tables& got, const PackedScene& want, const PackedScene& first) {
    if (!same(got.lights, want.lights)) return "lights differ from the fresh packing";
    if (!same(got.cdf, want.light_cdf)) return "light_cdf differs from the fresh packing";
    if (!same(got.pick, want.light_pick_pdf)) return "light_pick_pdf differs from the fresh packing";
    if (!same(got.power, want.light_power)) return "light_power differs from the fresh packing";
    if (!same(want.light_tris, first.light_tris)) return "light_tris moved";
    if (!same(want.ibl_dist, first.ibl_dist)) return "ibl_dist moved";
    if (want.wh_slots != first.wh_slots || want.extended != first.extended || want.has_ibl != first.has_ibl) return "wh_slots / extended / has_ibl moved";
    return "";
}

// first / count: the range handed to repack_lights; `also`: what else the case asks of the edited tables
std::string run(const Scene& s, uint32_t first, uint32_t count, const Edit& edit, const std::function<std::string(const Tables&)>& also) {
    std::vector<gbl_light> edited = s.lights;
    edit(edited);
    for (size_t i = 0; i < edited.size(); ++i)
        if ((i < first || i >= first + count) && memcmp(&edited[i], &s.lights[i], sizeof(gbl_light)) != 0) return "the case edits a light outside its range";
    Tables t = {s.packed.lights, s.packed.light_power, s.packed.light_cdf, s.packed.light_pick_pdf};
    repack_lights(edited.data() + first, first, count, s.packed.bound_lo, s.packed.bound_hi, &t.lights, &t.power, &t.cdf, &t.pick);
    PackedScene fresh;
    std::string err;
    if (!pack_edited(s, edited, &fresh, &err)) return "pack_scene refused the edited description: " + err;
    std::string what = compare(t, fresh, s.packed);
    if (!what.empty()) return what;
    if (same(t.lights, s.packed.lights) && same(t.pick, s.packed.light_pick_pdf)) return "the edit changed nothing";
    if (also && !(what = also(t)).empty()) return what;
    repack_lights(s.lights.data() + first, first, count, s.packed.bound_lo, s.packed.bound_hi, &t.lights, &t.power, &t.cdf, &t.pick);
    what = compare(t, s.packed, s.packed);
    return what.empty() ? "" : "after the inverse edit: " + what;
}

int find(const Scene& s, uint32_t type, int nth = 0) {
    for (size_t i = 0; i < s.lights.size(); ++i)
        if (s.lights[i].type == type && nth-- == 0) return static_cast<int>(i);
    return -1;
}

void set3(float* f, float x, float y, float z) { f[0] = x, f[1] = y, f[2] = z; }

}   // namespace

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    int failed = 0;
    Scene s;
    const auto open = [&](const char* name) {
        if (s.host) gbl_host_free(s.host);
        s = Scene();
        s.name = name;
        const std::string path = std::string(argv[1]) + "/" + name + ".json";
        std::string err;
        if (gbl_host_load_file(path.c_str(), &s.host) != GBL_OK) {
            fprintf(stderr, "%s: %s\n", path.c_str(), gbl_host_last_error());
            return false;
        }
        s.desc = gbl_host_desc(s.host);
        s.lights.assign(s.desc->lights, s.desc->lights + s.desc->num_lights);
        if (!pack(*s.desc, &s.packed, &err)) {
            fprintf(stderr, "%s: pack_scene: %s\n", path.c_str(), err.c_str());
            return false;
        }
        return true;
    };
    const auto check = [&](const char* name, int light, int count, const Edit& edit, const std::function<std::string(const Tables&)>& also = nullptr) {
        const std::string what = light < 0 ? "the scene has no such light" : run(s, static_cast<uint32_t>(light), static_cast<uint32_t>(count), edit, also);
        printf("case %s %s %s%s\n", s.name.c_str(), name, what.empty() ? "ok" : "FAIL ", what.c_str());
        failed += !what.empty();
    };
    const auto direction = [](int l, float x, float y, float z) { return Edit([=](std::vector<gbl_light>& L) { set3(L[l].direction, x, y, z); }); };
    const auto colour = [](int l, float k) { return Edit([=](std::vector<gbl_light>& L) { for (int c = 0; c < 3; ++c) L[l].color[c] *= k; }); };

    // ---- grid: a spot and a point light
    if (!open("grid")) return 1;
    {
        const int spot = find(s, GBL_LIGHT_SPOT), point = find(s, GBL_LIGHT_POINT);
        check("spot_colour", spot, 1, colour(spot, 2.5f));
        check("point_colour", point, 1, colour(point, 0.3f));
        check("spot_position", spot, 1, [=](std::vector<gbl_light>& L) { set3(L[spot].position, 1.25f, 7.5f, -2.0f); });
        check("point_position", point, 1, [=](std::vector<gbl_light>& L) { set3(L[point].position, -3.0f, 2.0f, 0.125f); });
        check("spot_direction_axis_z", spot, 1, direction(spot, 0.0f, 0.0f, 1.0f));
        check("spot_direction_axis_y", spot, 1, direction(spot, 0.0f, -2.0f, 0.0f));
        check("spot_direction_x_over_y", spot, 1, direction(spot, 0.8f, 0.3f, -0.5f));
        check("spot_direction_y_over_x", spot, 1, direction(spot, 0.2f, -0.9f, 0.4f));
        check("spot_direction_x_equals_y", spot, 1, direction(spot, 0.5f, -0.5f, 0.7f));
        check("spot_direction_trace_not_positive", spot, 1, direction(spot, 0.0f, 0.0f, -1.0f));
        check("spot_direction_trace_negative_x", spot, 1, direction(spot, -0.9f, 0.1f, -0.4f));
        check("spot_cos_theta_max", spot, 1, [=](std::vector<gbl_light>& L) { L[spot].cos_theta_max = 0.8125f; });
        check("spot_cos_falloff_start", spot, 1, [=](std::vector<gbl_light>& L) { L[spot].cos_falloff_start = 0.96875f; });
        check("both_lights_at_once", 0, 2, [=](std::vector<gbl_light>& L) {
            set3(L[spot].direction, -0.3f, -1.0f, 0.2f);
            set3(L[point].color, 4.0f, 5.0f, 6.0f);
        });
        check("point_without_power", point, 1, [=](std::vector<gbl_light>& L) { set3(L[point].color, 0.0f, 0.0f, 0.0f); }, [=](const Tables& t) {
            return t.power[point] == 0.0f && t.pick[point] == 0.0f && t.pick[spot] == 1.0f ? "" : "the light without power keeps a pick probability";
        });
    }
    // ---- cornell: one area light over a mesh; the CDF of a one-light scene is {0, 1}
    if (!open("cornell")) return 1;
    {
        const int area = find(s, GBL_LIGHT_AREA);
        const auto one_light = [](const Tables& t) { return t.cdf.size() == 2 && t.cdf[0] == 0.0f && t.cdf[1] == 1.0f ? "" : "a one-light CDF is not {0, 1}"; };
        check("one_light", s.lights.size() == 1 ? area : -1, 1, colour(area, 0.5f), one_light);
        check("area_colour", area, 1, colour(area, 3.0f));
        check("area_translation", area, 1, [=](std::vector<gbl_light>& L) {
            L[area].to_world.position[0] += 0.75f, L[area].to_world.position[1] -= 0.5f, L[area].to_world.position[2] += 0.25f;
        });
        check("area_scale_changes_power", area, 1, [=](std::vector<gbl_light>& L) { L[area].to_world.scale[0] *= 1.5f, L[area].to_world.scale[1] *= 0.5f, L[area].to_world.scale[2] *= 2.0f; },
              [&, area](const Tables& t) { return t.power[area] != s.packed.light_power[area] ? "" : "the scale left the power alone"; });
    }
    // ---- shapes: area lights over a sphere and a disk, and a directional light
    if (!open("shapes")) return 1;
    {
        const int a0 = find(s, GBL_LIGHT_AREA, 0), a1 = find(s, GBL_LIGHT_AREA, 1), sun = find(s, GBL_LIGHT_DIRECTIONAL);
        check("area0_colour", a0, 1, colour(a0, 1.75f));
        check("area1_colour", a1, 1, colour(a1, 0.25f));
        check("directional_colour", sun, 1, colour(sun, 2.0f));
        check("directional_direction", sun, 1, direction(sun, 0.4f, -1.0f, -0.3f));
        check("directional_direction_not_unit", sun, 1, direction(sun, -3.0f, -0.5f, 1.0f));
    }
    // ---- volume: lights in a participating medium, an area light over a sphere
    if (!open("volume")) return 1;
    {
        const int a0 = find(s, GBL_LIGHT_AREA, 0), a1 = find(s, GBL_LIGHT_AREA, 1), spot = find(s, GBL_LIGHT_SPOT);
        check("area0_colour", a0, 1, colour(a0, 0.5f));
        check("area1_colour", a1, 1, colour(a1, 2.0f));
        check("spot_direction", spot, 1, direction(spot, 0.3f, -0.8f, 0.45f));
    }
    // ---- ibl: an image based light and a point light
    if (!open("ibl")) return 1;
    {
        const int ibl = find(s, GBL_LIGHT_IBL), point = find(s, GBL_LIGHT_POINT);
        check("ibl_orientation", ibl, 1, [=](std::vector<gbl_light>& L) {
            float* q = L[ibl].to_world.orientation;
            q[0] = 0.9238795f, q[1] = 0.0f, q[2] = 0.3826834f, q[3] = 0.0f;
        });
        check("ibl_orientation_not_unit", ibl, 1, [=](std::vector<gbl_light>& L) {
            float* q = L[ibl].to_world.orientation;
            q[0] = 0.5f, q[1] = -0.25f, q[2] = 0.125f, q[3] = 1.5f;
        });
        check("point_colour_beside_the_ibl", point, 1, colour(point, 4.0f));
    }
    if (s.host) gbl_host_free(s.host);
    printf("failed %d\n", failed);
    return 0;
}
