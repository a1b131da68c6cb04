// Host program of tests/test_instances_device_cpu.py: the compose functions the device runs (goblin_amd/csrc/kernels/instances.h,
// compiled here for the host) against scene_prep.cpp's own -- pack_transform for m / inv and the invertibility verdict,
// build_tlas over a one-instance TlasInput for the world box -- bit for bit, over seeded random transforms and a list of edge
// cases.  Prints one "name value" line per count; the test asserts on them.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "../goblin_amd/csrc/kernels/instances.h"
#include "../goblin_amd/csrc/scene_prep.h"

namespace {

struct Counts {
    long cases = 0, invertible = 0, singular = 0, verdict = 0, m = 0, inv = 0, box = 0, record = 0, flagged = 0, not_flagged = 0;
};

// Bit for bit.  nan_class (the non-finite inputs only): two NaNs are the same value whatever their sign and payload -- IEEE 754
// leaves both to the implementation, x86 takes them from whichever operand the compiler put first, and the compose kernel
// refuses these inputs before it composes.  Every float that is a number is still compared by its bits.
bool nan_class = false;
bool same_bits(const float* a, const float* b, int n) {
    for (int i = 0; i < n; ++i)
        if (memcmp(a + i, b + i, sizeof(float)) != 0 && !(nan_class && std::isnan(a[i]) && std::isnan(b[i]))) return false;
    return true;
}

// One transform through both; `expect_not_finite`: whether a float of it is NaN or infinite
void one(const float t[10], const float lo[3], const float hi[3], bool expect_not_finite, Counts* c, bool* invertible_out = nullptr) {
    gbl_trs trs;
    memcpy(&trs, t, sizeof(trs));
    float m_h[12], inv_h[12], m_d[12], inv_d[12];
    std::string err;
    const bool ok_h = pack_transform(trs, 7, m_h, inv_h, &err);
    const bool ok_d = inst_compose(t, m_d, inv_d);
    c->cases += 1;
    if (invertible_out) *invertible_out = ok_h;
    if (inst_trs_not_finite(t) != expect_not_finite) c->not_flagged += 1;
    if (inst_trs_not_finite(t)) c->flagged += 1;
    if (ok_h != ok_d) {
        c->verdict += 1;
        return;
    }
    if (!ok_h) {
        c->singular += 1;
        if (err.find("instance 7") == std::string::npos || err.find("1e-5") == std::string::npos) c->verdict += 1;
        return;
    }
    c->invertible += 1;
    if (!same_bits(m_h, m_d, 12)) c->m += 1;
    if (!same_bits(inv_h, inv_d, 12)) c->inv += 1;
    // the box, and the record's m / inv once more, from build_tlas itself
    gbl_instance gi;
    memset(&gi, 0, sizeof(gi));
    gi.to_world = trs;
    gi.area_light = -1;
    gbl_mesh mesh;
    memset(&mesh, 0, sizeof(mesh));
    gbl_material mat;
    memset(&mat, 0, sizeof(mat));
    const int32_t root = 0;
    const TlasInput in = {&gi, 1u, &mesh, &mat, lo, hi, &root, 0};
    TlasResult built;
    if (build_tlas(in, &built, &err) != GBL_OK) {
        c->verdict += 1;
        return;
    }
    float blo[3], bhi[3];
    inst_world_box(m_d, lo, hi, blo, bhi);
    if (!same_bits(built.instance_bounds[0].lo, blo, 3) || !same_bits(built.instance_bounds[0].hi, bhi, 3)) c->box += 1;
    if (!same_bits(built.instances[0].m, m_d, 12) || !same_bits(built.instances[0].inv, inv_d, 12)) c->record += 1;
}

void print(const char* what, const Counts& c) {
    printf("%s_cases %ld\n%s_invertible %ld\n%s_singular %ld\n%s_verdict_differs %ld\n%s_m_differs %ld\n%s_inv_differs %ld\n%s_box_differs %ld\n"
           "%s_record_differs %ld\n%s_flagged_not_finite %ld\n%s_flag_wrong %ld\n",
           what, c.cases, what, c.invertible, what, c.singular, what, c.verdict, what, c.m, what, c.inv, what, c.box, what, c.record, what, c.flagged, what, c.not_flagged);
}

}   // namespace

int main() {
    std::mt19937 rng(20261020u);
    std::uniform_real_distribution<float> u(-1.0f, 1.0f);
    // ---- 10^5 random transforms over random mesh boxes
    Counts r;
    for (int k = 0; k < 100000; ++k) {
        float t[10], lo[3], hi[3];
        for (int a = 0; a < 3; ++a) t[a] = 10.0f * u(rng);
        for (int a = 0; a < 4; ++a) t[3 + a] = u(rng);
        if (k % 3 == 0) {   // a third of them normalised, as scene files hold them
            const float len = std::sqrt(t[3] * t[3] + t[4] * t[4] + t[5] * t[5] + t[6] * t[6]);
            for (int a = 0; a < 4; ++a) t[3 + a] /= len > 0.0f ? len : 1.0f;
        }
        const float size = std::exp(4.0f * u(rng));             // scales over e^-4 .. e^4: some fall below the determinant's threshold
        for (int a = 0; a < 3; ++a) t[7 + a] = (k % 5 == 0 ? size : size * (1.5f + u(rng))) * ((k % 7 == 0 && a == 1) ? -1.0f : 1.0f);
        for (int a = 0; a < 3; ++a) {
            const float c = 3.0f * u(rng), h = k % 11 == 0 && a == 2 ? 0.0f : 0.5f * (1.0f + u(rng));   // (a flat box now and then)
            lo[a] = c - h;
            hi[a] = c + h;
        }
        one(t, lo, hi, false, &r);
    }
    print("random", r);

    // ---- the edge cases
    const float lo[3] = {-0.5f, -0.0f, -1.25f}, hi[3] = {0.75f, 2.0f, 0.0f};
    const float base[10] = {0.3f, -1.7f, 2.9f, 0.9238795f, 0.0f, 0.3826834f, 0.0f, 0.6f, 0.6f, 0.6f};
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    Counts e;
    bool inv_flag = false;
    std::vector<std::vector<float>> valid;
    auto with = [&](std::initializer_list<std::pair<int, float>> changes) {
        std::vector<float> t(base, base + 10);
        for (const auto& ch : changes) t[ch.first] = ch.second;
        return t;
    };
    valid.push_back(with({{7, 0.2f}, {8, 1.5f}, {9, 3.0f}}));                    // non-uniform scale
    valid.push_back(with({{7, -0.6f}}));                                           // one negative scale
    valid.push_back(with({{7, -0.6f}, {8, -1.1f}, {9, -0.4f}}));                   // all negative
    valid.push_back(with({{3, 1.7f}, {4, -0.4f}, {5, 2.2f}, {6, 0.9f}}));          // an unnormalised quaternion
    valid.push_back(with({{0, -0.0f}, {1, -0.0f}, {2, -0.0f}}));                   // -0.0 position
    valid.push_back(with({{4, -0.0f}, {6, -0.0f}}));                               // -0.0 in the quaternion
    valid.push_back(with({{0, 1e6f}, {1, -1e6f}, {2, 1e6f}}));                     // translations of 1e6
    valid.push_back(with({{7, 0.0217f}, {8, 0.0217f}, {9, 0.0217f}}));             // just above |det| = 1e-5
    valid.push_back(with({{3, 1.0f}, {4, 0.0f}, {5, 0.0f}, {6, 0.0f}, {7, 1.0f}, {8, 1.0f}, {9, 1.0f}}));   // the identity rotation and scale
    for (const auto& t : valid) {
        one(t.data(), lo, hi, false, &e, &inv_flag);
        if (!inv_flag) e.verdict += 1000;   // every one of these must be accepted
    }
    printf("edge_list_valid %zu\n", valid.size());
    std::vector<std::vector<float>> singular;
    singular.push_back(with({{7, 0.0215f}, {8, 0.0215f}, {9, 0.0215f}}));          // just below the threshold
    singular.push_back(with({{7, 1e-39f}, {8, 1e-39f}, {9, 1e-39f}}));             // denormal scales
    singular.push_back(with({{7, 1e-39f}}));                                       // one denormal scale
    singular.push_back(with({{7, 0.0f}}));
    singular.push_back(with({{7, -0.0f}, {8, -0.0f}, {9, -0.0f}}));
    singular.push_back(with({{3, 0.0f}, {4, 0.0f}, {5, 0.0f}, {6, 0.0f}, {7, 0.001f}, {8, 0.001f}, {9, 0.001f}}));
    for (const auto& t : singular) {
        one(t.data(), lo, hi, false, &e, &inv_flag);
        if (inv_flag) e.verdict += 1000;    // ... and every one of these refused
    }
    printf("edge_list_singular %zu\n", singular.size());
    print("edge", e);
    // NaN and +-inf in each of the ten slots: the device refuses these before it composes; the flag is what is compared, and the
    // composed bits beside it wherever the host composes numbers
    Counts n;
    nan_class = true;
    for (int slot = 0; slot < 10; ++slot)
        for (float bad : {nan, inf, -inf}) {
            const std::vector<float> t = with({{slot, bad}});
            one(t.data(), lo, hi, true, &n);
        }
    print("nonfinite", n);
    return 0;
}
