// Host-side scene packing for the device integrator: transforms, the two-level
// BVH (our own binned-SAH builder, NOT the reference's median-split tree), the
// packed triangle / instance / material / light tables, camera and film
// constants.  Replaces the constructors the reference runs at load time:
//   Transform::update            GoblinTransform.cpp:182-193
//   Model / Scene BVH build      GoblinModel.cpp:10-26, GoblinScene.cpp:11-27, GoblinBVH.cpp:34-151
//   SpotLight / AreaLight ctors  GoblinLight.cpp:212-223, 345-361
//   PerspectiveCamera ctor       GoblinCamera.cpp:83-95
//   FilterTable ctor             GoblinFilm.cpp:10-27
// Radiance is BVH-independent except for exact t ties, so the tree is built for
// the GPU: both child boxes in the parent (64 B nodes), <= 4 triangles per leaf,
// SAH splits, depth-capped so the LDS traversal stack has a hard bound.
#include "scene_prep.h"
#include "kernels/materials.h"

#include <algorithm>
#include <array>
#include <atomic>
#include <cmath>
#include <cstring>
#include <thread>

namespace {

const float kPi = 3.14159265358979323f;
const float kTwoPi = 6.28318530718f;

// ---------------------------------------------------------------- transforms
struct Mat4 {
    float v[4][4];
};

Mat4 identity() {
    Mat4 r;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) r.v[i][j] = i == j ? 1.0f : 0.0f;
    return r;
}

Mat4 multiply(const Mat4& a, const Mat4& b) {
    Mat4 r;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            float acc = a.v[i][0] * b.v[0][j];
            acc = acc + a.v[i][1] * b.v[1][j];
            acc = acc + a.v[i][2] * b.v[2][j];
            acc = acc + a.v[i][3] * b.v[3][j];
            r.v[i][j] = acc;
        }
    return r;
}

Mat4 rotation_of(const float q[4]) {   // q = w x y z
    const float w = q[0], x = q[1], y = q[2], z = q[3];
    const float tx = 2.0f * x, ty = 2.0f * y, tz = 2.0f * z;
    const float xx = tx * x, xy = tx * y, xz = tx * z, xw = tx * w;
    const float yy = ty * y, yz = ty * z, yw = ty * w;
    const float zz = tz * z, zw = tz * w;
    Mat4 r = identity();
    r.v[0][0] = 1 - yy - zz; r.v[0][1] = xy - zw;     r.v[0][2] = xz + yw;
    r.v[1][0] = xy + zw;     r.v[1][1] = 1 - xx - zz; r.v[1][2] = yz - xw;
    r.v[2][0] = xz - yw;     r.v[2][1] = yz + xw;     r.v[2][2] = 1 - xx - yy;
    return r;
}

// 2x2 minor of rows (r0, r1), columns (c0, c1)
inline float minor2(const Mat4& m, int r0, int r1, int c0, int c1) { return m.v[r0][c0] * m.v[r1][c1] - m.v[r0][c1] * m.v[r1][c0]; }

// General 4x4 inverse by cofactors, expanding each cofactor along the row that
// is NOT in the minor's row pair, in the same association as the reference so
// the float32 result is the same; fails (returns false) when |det| < 1e-5.
bool invert(const Mat4& m, Mat4* out) {
    const int cols[6][2] = {{2, 3}, {1, 3}, {1, 2}, {0, 3}, {0, 2}, {0, 1}};
    float a[6], b[6], c[6];   // minors of row pairs (2,3), (1,3), (1,2)
    for (int k = 0; k < 6; ++k) {
        a[k] = minor2(m, 2, 3, cols[k][0], cols[k][1]);
        b[k] = minor2(m, 1, 3, cols[k][0], cols[k][1]);
        c[k] = minor2(m, 1, 2, cols[k][0], cols[k][1]);
    }
    auto cof = [&](int row, const float s[6], float r[4]) {
        r[0] = m.v[row][1] * s[0] - m.v[row][2] * s[1] + m.v[row][3] * s[2];
        r[1] = m.v[row][0] * s[0] - m.v[row][2] * s[3] + m.v[row][3] * s[4];
        r[2] = m.v[row][0] * s[1] - m.v[row][1] * s[3] + m.v[row][3] * s[5];
        r[3] = m.v[row][0] * s[2] - m.v[row][1] * s[4] + m.v[row][2] * s[5];
    };
    float k0[4], k1[4], k2[4], k3[4];
    cof(1, a, k0);
    cof(0, a, k1);
    cof(0, b, k2);
    cof(0, c, k3);
    const float sgn[4] = {1.0f, -1.0f, 1.0f, -1.0f};
    Mat4& o = *out;
    for (int i = 0; i < 4; ++i) o.v[i][0] = sgn[i] > 0 ? k0[i] : -k0[i];
    float det = m.v[0][0] * o.v[0][0] + m.v[0][1] * o.v[1][0] + m.v[0][2] * o.v[2][0] + m.v[0][3] * o.v[3][0];
    if (std::fabs(det) < 1e-5f) return false;
    float inv_det = 1.0f / det;
    for (int i = 0; i < 4; ++i) {
        o.v[i][1] = sgn[i] > 0 ? -k1[i] : k1[i];
        o.v[i][2] = sgn[i] > 0 ? k2[i] : -k2[i];
        o.v[i][3] = sgn[i] > 0 ? -k3[i] : k3[i];
    }
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) o.v[i][j] *= inv_det;
    return true;
}

struct Trs {
    Mat4 m, inv;
    bool invertible;
};

Trs compose(const float pos[3], const float q[4], const float scale[3]) {
    Mat4 S = identity();
    S.v[0][0] = scale[0]; S.v[1][1] = scale[1]; S.v[2][2] = scale[2];
    Trs t;
    t.m = multiply(rotation_of(q), S);
    t.m.v[0][3] = pos[0]; t.m.v[1][3] = pos[1]; t.m.v[2][3] = pos[2];
    t.inv = identity();
    t.invertible = invert(t.m, &t.inv);
    return t;
}

void store3x4(const Mat4& m, float out[12]) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j) out[4 * i + j] = m.v[i][j];
}

void point_by(const Mat4& m, const float p[3], float out[3]) {
    for (int i = 0; i < 3; ++i) out[i] = m.v[i][0] * p[0] + m.v[i][1] * p[1] + m.v[i][2] * p[2] + m.v[i][3];
}

// ---------------------------------------------------------------------- BVH
struct Aabb {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    void grow(const float p[3]) {
        for (int k = 0; k < 3; ++k) {
            lo[k] = std::min(lo[k], p[k]);
            hi[k] = std::max(hi[k], p[k]);
        }
    }
    void grow(const Aabb& b) {
        for (int k = 0; k < 3; ++k) {
            lo[k] = std::min(lo[k], b.lo[k]);
            hi[k] = std::max(hi[k], b.hi[k]);
        }
    }
    float half_area() const {
        float d[3] = {hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]};
        if (d[0] < 0 || d[1] < 0 || d[2] < 0) return 0.0f;
        return d[0] * d[1] + d[1] * d[2] + d[2] * d[0];
    }
};

struct Prim {
    Aabb box;
    float c[3];
    uint32_t id;
};

struct TmpNode {
    Aabb box;
    int left = -1, right = -1;   // interior
    uint32_t first = 0, count = 0;   // leaf when count > 0
};

int balanced_height(size_t n, int leaf) {
    int h = 1;
    size_t leaves = (n + leaf - 1) / leaf;
    while (leaves > 1) {
        leaves = (leaves + 1) / 2;
        ++h;
    }
    return h;
}

// Most entries a ray can have on its traversal stack while inside the subtree of `ref` (kernels/trace.h trav_interior: a node
// whose k children are all hit leaves k - 1 of them on the stack while the first is visited, and any child can be the first).
// The 3-per-level bound assumes four children at every level of the deepest path; SAH trees of real meshes need about two
// thirds of it, and the megakernel's LDS stacks are sized by this number (api_render.hip: three workgroups per CU or two).
// GBL_STACK_LEVEL_BOUND=1 (a test aid): count three siblings at every node, i.e. the per-level bound the stacks had before.
static bool stack_level_bound() {
    static const bool on = [] { const char* e = getenv("GBL_STACK_LEVEL_BOUND"); return e != nullptr && e[0] != '\0' && e[0] != '0'; }();
    return on;
}
template <class ChildNeed>
static int node_stack_need(const DevNode& n, ChildNeed child_need) {
    int k = 0, deepest = 0;
    for (int c = 0; c < 4; ++c) {
        if (n.child[c] == GBL_REF_NONE) continue;
        ++k;
        deepest = std::max(deepest, child_need(n.child[c]));
    }
    return k > 0 ? (stack_level_bound() ? 3 : k - 1) + deepest : 0;
}
static int blas_stack_need(const std::vector<DevNode>& nodes, int32_t ref) {
    if (ref < 0 || ref >= static_cast<int32_t>(nodes.size())) return 0;   // a leaf (or an analytic shape's root)
    return node_stack_need(nodes[static_cast<size_t>(ref)], [&](int32_t c) { return blas_stack_need(nodes, c); });
}

static int tlas_stack_need(const std::vector<DevNode>& tlas, int32_t tlas_base, int32_t ref, const std::vector<DevInstance>& instances,
                           const std::vector<int>& mesh_need) {
    if (ref == GBL_REF_NONE) return 0;
    if (ref < 0) {   // an instance: its sentinel, then its BLAS (an analytic shape's "root" is a leaf)
        const uint32_t i = (~static_cast<uint32_t>(ref)) >> 2;
        if (i >= instances.size()) return 1;
        const DevInstance& di = instances[i];
        const bool mesh = di.shape == 0u && di.mesh >= 0 && static_cast<size_t>(di.mesh) < mesh_need.size();
        return 1 + (mesh ? mesh_need[static_cast<size_t>(di.mesh)] : 0);
    }
    const size_t local = static_cast<size_t>(ref - tlas_base);
    if (local >= tlas.size()) return 0;
    return node_stack_need(tlas[local], [&](int32_t c) { return tlas_stack_need(tlas, tlas_base, c, instances, mesh_need); });
}

// SAH cost of visiting a node relative to one triangle test (tuning knob: GBL_SAH_CT)
inline float sah_traversal_cost() {
    static const float ct = [] {
        const char* e = getenv("GBL_SAH_CT");
        return e ? static_cast<float>(atof(e)) : 1.0f;
    }();
    return ct;
}

struct Builder {
    std::vector<Prim>& prims;
    std::vector<TmpNode> nodes;
    int max_leaf, depth_cap, height = 0;
    // parallel build: subranges of at most `defer_below` primitives are not descended into but recorded as tasks
    struct Task {
        int node;
        size_t start, end;
        int depth;
    };
    size_t defer_below = 0;
    std::vector<Task> tasks;
    Builder(std::vector<Prim>& p, int leaf, int cap) : prims(p), max_leaf(leaf), depth_cap(cap) {}

    // Same tree as build(0, n, 1), built on several host threads: the top of the tree sequentially, every subtree of
    // <= n/64 primitives as an independent task (the tasks own disjoint ranges of `prims`), merged in task order --
    // so the result does not depend on the number of threads.
    int build_parallel(size_t n) {
        const unsigned hw = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
        if (n < 65536 || hw < 2) return build(0, n, 1);
        defer_below = std::max<size_t>(4096, n / 64);
        int root = build(0, n, 1);
        defer_below = 0;
        std::vector<Builder> subs;
        subs.reserve(tasks.size());
        for (size_t i = 0; i < tasks.size(); ++i) subs.emplace_back(prims, max_leaf, depth_cap);
        std::atomic<size_t> next(0);
        auto work = [&]() {
            for (size_t i = next.fetch_add(1); i < tasks.size(); i = next.fetch_add(1)) subs[i].build(tasks[i].start, tasks[i].end, tasks[i].depth);
        };
        std::vector<std::thread> pool;
        for (unsigned t = 1; t < std::min<size_t>(hw, tasks.size()); ++t) pool.emplace_back(work);
        work();
        for (auto& th : pool) th.join();
        for (size_t i = 0; i < tasks.size(); ++i) {
            const std::vector<TmpNode>& sn = subs[i].nodes;   // sn[0] is the subtree's root
            const int offset = static_cast<int>(nodes.size()) - 1;
            auto remap = [&](TmpNode nd) {
                if (nd.count == 0) {
                    nd.left += offset;
                    nd.right += offset;
                }
                return nd;
            };
            nodes[tasks[i].node] = remap(sn[0]);
            for (size_t k = 1; k < sn.size(); ++k) nodes.push_back(remap(sn[k]));
            height = std::max(height, subs[i].height);
        }
        tasks.clear();
        return root;
    }

    int build(size_t start, size_t end, int depth) {
        int me = static_cast<int>(nodes.size());
        nodes.push_back(TmpNode());
        Aabb box, cbox;
        for (size_t i = start; i < end; ++i) {
            box.grow(prims[i].box);
            cbox.grow(prims[i].c);
        }
        nodes[me].box = box;
        height = std::max(height, depth);
        size_t n = end - start;
        if (defer_below && depth > 1 && n <= defer_below && n > static_cast<size_t>(max_leaf)) {
            tasks.push_back(Task{me, start, end, depth});
            return me;
        }
        int room = depth_cap - depth;   // levels available below this node
        // binned SAH over the centroid bounds, all three axes
        // (tuning knobs like GBL_SAH_CT: GBL_SAH_BINS, and GBL_MAX_LEAF below.  On bunny.json 8 / 16 / 32 bins trace alike --
        //  51.3 / 51.3 / 51.1 ms -- while 64 bins or 2-triangle leaves add a BLAS level and with it the LDS for a third
        //  workgroup per CU: 65.6 / 66.1 ms)
        static const int B = [] { const char* e = getenv("GBL_SAH_BINS"); return e ? std::max(4, std::min(64, atoi(e))) : 16; }();
        float best_cost = INFINITY;
        int best_axis = -1, best_bin = -1;
        float parent_area = box.half_area();
        if (n > 1 && parent_area > 0.0f) {
            for (int axis = 0; axis < 3; ++axis) {
                float lo = cbox.lo[axis], ext = cbox.hi[axis] - cbox.lo[axis];
                if (!(ext > 0.0f)) continue;
                Aabb bb[64];
                size_t bn[64] = {0};
                float scale = B / ext;
                for (size_t i = start; i < end; ++i) {
                    int b = std::min(B - 1, static_cast<int>((prims[i].c[axis] - lo) * scale));
                    bb[b].grow(prims[i].box);
                    bn[b]++;
                }
                Aabb right_acc[64];
                size_t right_n[64];
                Aabb acc;
                size_t cnt = 0;
                for (int b = B - 1; b >= 1; --b) {
                    acc.grow(bb[b]);
                    cnt += bn[b];
                    right_acc[b] = acc;
                    right_n[b] = cnt;
                }
                Aabb left;
                size_t ln = 0;
                for (int b = 0; b < B - 1; ++b) {
                    left.grow(bb[b]);
                    ln += bn[b];
                    size_t rn = right_n[b + 1];
                    if (ln == 0 || rn == 0) continue;
                    if (balanced_height(std::max(ln, rn), max_leaf) > room) continue;   // would break the depth cap
                    float cost = sah_traversal_cost() + (left.half_area() * ln + right_acc[b + 1].half_area() * rn) / parent_area;
                    if (cost < best_cost) {
                        best_cost = cost;
                        best_axis = axis;
                        best_bin = b;
                    }
                }
            }
        }
        bool can_leaf = n <= static_cast<size_t>(max_leaf);
        if (can_leaf && (best_axis < 0 || static_cast<float>(n) <= best_cost)) {
            nodes[me].first = static_cast<uint32_t>(start);
            nodes[me].count = static_cast<uint32_t>(n);
            return me;
        }
        size_t mid;
        if (best_axis >= 0) {
            float lo = cbox.lo[best_axis], scale = B / (cbox.hi[best_axis] - cbox.lo[best_axis]);
            int axis = best_axis, bin = best_bin;
            auto it = std::partition(prims.begin() + start, prims.begin() + end, [&](const Prim& p) {
                return std::min(B - 1, static_cast<int>((p.c[axis] - lo) * scale)) <= bin;
            });
            mid = static_cast<size_t>(it - prims.begin());
        } else {
            // object median on the widest centroid axis (also the depth-cap fallback)
            int axis = 0;
            float e[3] = {cbox.hi[0] - cbox.lo[0], cbox.hi[1] - cbox.lo[1], cbox.hi[2] - cbox.lo[2]};
            if (e[1] > e[axis]) axis = 1;
            if (e[2] > e[axis]) axis = 2;
            mid = (start + end) / 2;
            std::nth_element(prims.begin() + start, prims.begin() + mid, prims.begin() + end,
                             [axis](const Prim& a, const Prim& b) { return a.c[axis] < b.c[axis]; });
        }
        if (mid == start || mid == end) mid = (start + end) / 2;
        int l = build(start, mid, depth + 1);
        int r = build(mid, end, depth + 1);
        nodes[me].left = l;
        nodes[me].right = r;
        return me;
    }
};

// Collapse the binary tree into 4-wide nodes and quantise the child boxes to 8 bits on a
// per-node power-of-two grid.  Boxes are first nudged outwards by a few ulps and then rounded
// outwards to the grid, so the device slab test (fused multiply-add form) can never cull a
// triangle the exact test would keep.
inline float nudge_down(float v) { return v - std::fabs(v) * 4e-7f - 1e-30f; }
inline float nudge_up(float v) { return v + std::fabs(v) * 4e-7f + 1e-30f; }

struct Flat4 {
    const Builder& b;
    std::vector<DevNode>& out;
    int32_t base;         // index out[0] has in the device node array
    int depth = 0;        // deepest 4-wide level reached (root = 1)
    Flat4(const Builder& bb, std::vector<DevNode>& o, int32_t base_index = 0) : b(bb), out(o), base(base_index) {}

    template <class LeafRef>
    int32_t emit(int node, int level, LeafRef& leaf_ref) {
        const TmpNode& r = b.nodes[node];
        depth = std::max(depth, level);
        if (r.count > 0) return leaf_ref(r.first, r.count);
        // gather up to 4 children: keep splitting the interior child with the largest area
        int kids[4] = {r.left, r.right, -1, -1};
        int n = 2;
        while (n < 4) {
            int best = -1;
            float best_area = -1.0f;
            for (int i = 0; i < n; ++i) {
                const TmpNode& c = b.nodes[kids[i]];
                if (c.count == 0 && c.box.half_area() > best_area) {
                    best_area = c.box.half_area();
                    best = i;
                }
            }
            if (best < 0) break;
            const TmpNode& c = b.nodes[kids[best]];
            kids[best] = c.left;
            kids[n++] = c.right;
        }
        int32_t me = base + static_cast<int32_t>(out.size());
        out.push_back(DevNode());
        int32_t refs[4];
        for (int i = 0; i < 4; ++i) refs[i] = i < n ? emit(kids[i], level + 1, leaf_ref) : static_cast<int32_t>(GBL_REF_NONE);
        DevNode nd;
        memset(&nd, 0, sizeof(nd));
        // node bounds over the (nudged) children
        float lo[3], hi[3];
        for (int a = 0; a < 3; ++a) {
            lo[a] = INFINITY;
            hi[a] = -INFINITY;
            for (int i = 0; i < n; ++i) {
                lo[a] = std::min(lo[a], nudge_down(b.nodes[kids[i]].box.lo[a]));
                hi[a] = std::max(hi[a], nudge_up(b.nodes[kids[i]].box.hi[a]));
            }
        }
        for (int a = 0; a < 3; ++a) {
            nd.o[a] = lo[a];
            // grid step 2^e with 255 * 2^e >= extent (plus headroom for the rounding of o + q * step)
            float extent = (hi[a] - lo[a]) * 1.0001f + 1e-30f;
            int e = 0;
            std::frexp(extent / 255.0f, &e);   // extent/255 = m * 2^e, m in [0.5, 1)  ->  2^e >= extent/255
            int biased = std::min(254, std::max(1, e + 127));
            float step = std::ldexp(1.0f, biased - 127);
            nd.scale[a] = step;
            uint32_t ql = 0, qh = 0;
            for (int i = 0; i < 4; ++i) {
                uint32_t l = 255, h = 0;   // unused slot: inverted box, never hit
                if (i < n) {
                    float cl = nudge_down(b.nodes[kids[i]].box.lo[a]), ch = nudge_up(b.nodes[kids[i]].box.hi[a]);
                    double fl = std::floor((static_cast<double>(cl) - lo[a]) / step);
                    double fh = std::ceil((static_cast<double>(ch) - lo[a]) / step);
                    // guard the float evaluation o + q * step on the device against rounding inwards
                    while (fl > 0 && lo[a] + static_cast<float>(fl) * step > cl) fl -= 1;
                    while (fh < 255 && lo[a] + static_cast<float>(fh) * step < ch) fh += 1;
                    l = static_cast<uint32_t>(std::min(255.0, std::max(0.0, fl)));
                    h = static_cast<uint32_t>(std::min(255.0, std::max(0.0, fh)));
                }
                ql |= l << (8 * i);
                qh |= h << (8 * i);
            }
            nd.qlo[a] = ql;
            nd.qhi[a] = qh;
        }
        for (int i = 0; i < 4; ++i) nd.child[i] = refs[i];
        out[me - base] = nd;
        return me;
    }
};

// -------------------------------------------------------------------- filter
struct Filter {
    uint32_t type;
    float wx, wy, alpha, ex, ey, b, c;
    float gauss(float v, float base) const { return std::max(0.0f, expf(-alpha * v * v) - base); }
    float mitchell1(float x) const {
        x = std::fabs(2.0f * x);
        if (x > 1.0f) return ((-b - 6 * c) * x * x * x + (6 * b + 30 * c) * x * x + (-12 * b - 48 * c) * x + (8 * b + 24 * c)) / 6.0f;
        return ((12 - 9 * b - 6 * c) * x * x * x + (-18 + 12 * b + 6 * c) * x * x + (6 - 2 * b)) / 6.0f;
    }
    float eval(float x, float y) const {
        if (type == GBL_FILTER_BOX) return 1.0f;
        if (type == GBL_FILTER_TRIANGLE) return std::max(0.0f, wx - fabsf(x)) * std::max(0.0f, wy - fabsf(y));
        if (type == GBL_FILTER_MITCHELL) return mitchell1(x * (1.0f / wx)) * mitchell1(y * (1.0f / wy));
        return gauss(x, ex) * gauss(y, ey);
    }
    float norm() const {
        if (type == GBL_FILTER_BOX) return 4.0f * wx * wy;
        if (type == GBL_FILTER_TRIANGLE) return wx * wx * wy * wy;
        if (type == GBL_FILTER_MITCHELL)
            return 4.0f * ((12 - 9 * b - 6 * c) / 4 + (-18 + 12 * b + 6 * c) / 3 + (6 - 2 * b) + 15 * (-b - 6 * b) / 4 +
                           7 * (6 * b + 30 * c) / 3 + 3 * (-12 * b - 48 * c) / 2 + (8 * b + 24 * c)) / 6.0f;
        const size_t steps = 20;   // the reference integrates the gaussian numerically (GoblinFilter.cpp:48-64)
        float dx = wx / static_cast<float>(steps), dy = wy / static_cast<float>(steps), sum = 0.0f;
        for (size_t i = 0; i < steps; ++i)
            for (size_t j = 0; j < steps; ++j) sum += 4.0f * dx * dy * gauss(i * dx, ex) * gauss(j * dy, ey);
        return sum;
    }
};

// Levels below a material slot: a constant is 0, a checkerboard / scale of constants is 1, ...  -1: bad index or cycle.
int texture_depth(const gbl_scene_desc& d, int32_t id, int guard) {
    if (id < 0 || static_cast<uint32_t>(id) >= d.num_textures || guard > 64) return -1;
    const gbl_texture& g = d.textures[id];
    if (g.type == GBL_TEX_CONSTANT) return 0;
    if (g.type == GBL_TEX_IMAGE) return 1;   // a leaf with a lookup of its own
    int a = texture_depth(d, g.child[0], guard + 1), b = texture_depth(d, g.child[1], guard + 1);
    if (a < 0 || b < 0) return -1;
    return 1 + std::max(a, b);
}

int ceil_i(float f) { return static_cast<int>(std::ceil(f)); }
int floor_i(float f) { return static_cast<int>(std::floor(f)); }

// ------------------------------------------------ what a check and a packer share
// The arrays of one mesh inside the description's
struct MeshView {
    const float *P, *N, *uv;
    const uint32_t* I;
    const float* p(uint32_t t, int k) const { return P + 3 * I[3 * t + k]; }   // position, normal, uv of triangle t's vertex k
    const float* n(uint32_t t, int k) const { return N + 3 * I[3 * t + k]; }
    const float* t_uv(uint32_t t, int k) const { return uv + 2 * I[3 * t + k]; }
};
MeshView view_of(const gbl_scene_desc& d, const gbl_mesh& m) {
    const size_t v = m.vertex_offset;
    return MeshView{d.positions + 3 * v, d.normals + 3 * v, d.uvs + 2 * v, d.indices + 3 * static_cast<size_t>(m.tri_offset)};
}

// Per triangle of a mesh its vertices' bound (Triangle::getObjectBound), the bound's centre and its number
std::vector<Prim> triangle_prims(const MeshView& mv, uint32_t n) {
    std::vector<Prim> prims(n);
    for (uint32_t t = 0; t < n; ++t) {
        Prim& p = prims[t];
        for (int k = 0; k < 3; ++k) p.box.grow(mv.p(t, k));
        for (int k = 0; k < 3; ++k) p.c[k] = 0.5f * (p.box.lo[k] + p.box.hi[k]);
        p.id = t;
    }
    return prims;
}

uint32_t tri_flags(const gbl_mesh& m) { return (m.has_normal ? 1u : 0u) | (m.has_uv ? 2u : 0u); }

// The texture slots a material of this type reads (-1: none)
std::array<int32_t, 6> texture_slots(const gbl_material& m) {
    return {m.tex_color, m.tex_color2, m.tex_exponent, m.type == GBL_MAT_SUBSURFACE ? m.tex_color3 : -1, m.tex_bump, m.tex_normal};
}

// An instance's transform, or the one refusal build_tlas makes (validate_desc makes it first)
bool instance_transform(const gbl_instance& gi, uint32_t i, Trs* t, std::string* err) {
    *t = compose(gi.to_world.position, gi.to_world.orientation, gi.to_world.scale);
    if (!t->invertible)
        *err = "instance " + std::to_string(i) + ": |det(toWorld)| < 1e-5, the reference cannot invert this transform "
               "(GoblinMatrix.cpp:451); use a uniform scale >= 0.0216";
    return t->invertible;
}

uint64_t level_texels(const gbl_image& gi, uint32_t level) {
    return static_cast<uint64_t>(std::max(1u, gi.width >> level)) * std::max(1u, gi.height >> level) * gi.channels;
}

// The medium's box (BBox(p1, p2), GoblinBBox.h:20-23) and its transform
struct VolumeRegion { float lo[3], hi[3]; Trs to_world; };
VolumeRegion region_of(const gbl_volume& g) {
    VolumeRegion r;
    for (int k = 0; k < 3; ++k) r.lo[k] = std::min(g.box_min[k], g.box_max[k]), r.hi[k] = std::max(g.box_min[k], g.box_max[k]);
    r.to_world = compose(g.to_world.position, g.to_world.orientation, g.to_world.scale);
    return r;
}
// The region's longest world-space diagonal: a march is at most this / step_size points long
double march_diagonal(const VolumeRegion& r) {
    double diag = 0.0;
    for (int sgn = 0; sgn < 4; ++sgn) {
        const double e[3] = {double(r.hi[0] - r.lo[0]), (sgn & 1 ? -1.0 : 1.0) * double(r.hi[1] - r.lo[1]), (sgn & 2 ? -1.0 : 1.0) * double(r.hi[2] - r.lo[2])};
        double w[3];
        for (int k = 0; k < 3; ++k) w[k] = r.to_world.m.v[k][0] * e[0] + r.to_world.m.v[k][1] * e[1] + r.to_world.m.v[k][2] * e[2];
        diag = std::max(diag, std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]));
    }
    return diag;
}

void store_bound(const Aabb& b, float lo[3], float hi[3]) {
    for (int k = 0; k < 3; ++k) lo[k] = b.lo[k], hi[k] = b.hi[k];
}

int filter_halo(const gbl_film& f) { return ceil_i(std::max(f.filter_width[0], f.filter_width[1]) + 0.5f); }

// ---------------------------------------------------------------- validation
gbl_status refuse(gbl_status st, const std::string& why, std::string* err) { *err = why; return st; }

gbl_status validate_meshes(const gbl_scene_desc& d, std::string* err) {
    for (uint32_t i = 0; i < d.num_meshes; ++i) {
        const gbl_mesh& m = d.meshes[i];
        const std::string who = "mesh " + std::to_string(i);
        if (m.shape == GBL_SHAPE_SPHERE || m.shape == GBL_SHAPE_DISK) continue;
        if (m.shape != GBL_SHAPE_MESH) return refuse(GBL_ERR_INVALID, who + " has an unknown shape", err);
        if (m.tri_count == 0 || static_cast<uint64_t>(m.vertex_offset) + m.vertex_count > d.num_vertices || static_cast<uint64_t>(m.tri_offset) + m.tri_count > d.num_triangles)
            return refuse(GBL_ERR_INVALID, who + " is empty or out of range", err);
        const MeshView mv = view_of(d, m);
        for (uint32_t t = 0; t < 3 * m.tri_count; ++t)
            if (mv.I[t] >= m.vertex_count) return refuse(GBL_ERR_INVALID, who + " has a vertex index out of range", err);
        if (!m.has_uv) continue;
        // A triangle whose uv determinant is 0 makes the reference build its tangent from whatever Fragment the caller passed in
        // (GoblinTriangle.cpp:113-117): not reproducible.
        for (uint32_t t = 0; t < m.tri_count; ++t) {
            const float *a = mv.t_uv(t, 0), *b = mv.t_uv(t, 1), *c = mv.t_uv(t, 2);
            float du1 = b[0] - a[0], dv1 = b[1] - a[1], du2 = c[0] - a[0], dv2 = c[1] - a[1];
            if (du1 * dv2 - dv1 * du2 == 0.0f)
                return refuse(GBL_ERR_UNSUPPORTED, who + " triangle " + std::to_string(t) + " has degenerate texture coordinates (stale-fragment branch of the reference)", err);
        }
    }
    return GBL_OK;
}

// The occupied texture slots of material i: in range, no cycle, no deeper than the device evaluates
gbl_status validate_material_slots(const gbl_scene_desc& d, uint32_t i, std::string* err) {
    for (int32_t t : texture_slots(d.materials[i])) {
        if (t < 0) continue;
        const int depth = texture_depth(d, t, 0);
        if (depth < 0)
            return refuse(GBL_ERR_INVALID, "material " + std::to_string(i) + " references a texture out of range (or a cyclic texture graph)", err);
        if (depth > GBL_TEX_MAX_DEPTH)
            return refuse(GBL_ERR_UNSUPPORTED, "material " + std::to_string(i) + ": texture graph deeper than " +
                          std::to_string(GBL_TEX_MAX_DEPTH) + " levels below the material slot is outside the device path", err);
    }
    return GBL_OK;
}

gbl_status validate_materials(const gbl_scene_desc& d, std::string* err) {
    for (uint32_t i = 0; i < d.num_materials; ++i) {
        const gbl_material& m = d.materials[i];
        if (m.type > GBL_MAT_SUBSURFACE) return refuse(GBL_ERR_INVALID, "unknown material type", err);
        if (m.type == GBL_MAT_MASK && (m.masked_material < 0 || static_cast<uint32_t>(m.masked_material) >= d.num_materials ||
                                       d.materials[m.masked_material].type == GBL_MAT_MASK || d.materials[m.masked_material].type == GBL_MAT_SUBSURFACE))
            return refuse(GBL_ERR_INVALID, "mask material " + std::to_string(i) + " must wrap a non-mask, non-subsurface material of the scene", err);
        const gbl_status st = validate_material_slots(d, i, err);
        if (st != GBL_OK) return st;
    }
    return GBL_OK;
}

gbl_status validate_images(const gbl_scene_desc& d, std::string* err) {
    for (uint32_t i = 0; i < d.num_images; ++i) {
        const gbl_image& gi = d.images[i];
        if (gi.width == 0 || gi.height == 0 || (gi.width & (gi.width - 1)) || (gi.height & (gi.height - 1)) || (gi.channels != 1 && gi.channels != 4) ||
            gi.levels == 0 || gi.levels > 18)
            return refuse(GBL_ERR_INVALID, "image " + std::to_string(i) + ": sides must be powers of two, channels 1 or 4, at most 18 levels", err);
        uint64_t texels = 0;
        for (uint32_t l = 0; l < gi.levels; ++l) texels += level_texels(gi, l);
        if (gi.texel_offset + texels > d.num_texels || texels >= (1ull << 32))
            return refuse(GBL_ERR_INVALID, "image " + std::to_string(i) + ": texels out of range", err);
    }
    return GBL_OK;
}

gbl_status validate_textures(const gbl_scene_desc& d, std::string* err) {
    for (uint32_t i = 0; i < d.num_textures; ++i) {
        const gbl_texture& g = d.textures[i];
        if (g.type > GBL_TEX_IMAGE || g.mapping > GBL_MAP_SPHERICAL) return refuse(GBL_ERR_INVALID, "unknown texture or mapping type", err);
        if (g.type == GBL_TEX_IMAGE && (g.image < 0 || static_cast<uint32_t>(g.image) >= d.num_images || g.image_filter > GBL_IMAGE_FILTER_EWA ||
                                        g.address > GBL_ADDRESS_BORDER || d.images[g.image].channels != (g.is_float ? 1u : 4u)))
            return refuse(GBL_ERR_INVALID, "image texture " + std::to_string(i) + ": bad image index, filter, address mode or channel count", err);
    }
    return GBL_OK;
}

gbl_status validate_lights(const gbl_scene_desc& d, std::string* err) {
    for (uint32_t i = 0; i < d.num_lights; ++i) {
        const gbl_light& gl = d.lights[i];
        if (gl.type == GBL_LIGHT_AREA && gl.mesh >= d.num_meshes) return refuse(GBL_ERR_INVALID, "area light references a mesh out of range", err);
        if (gl.type == GBL_LIGHT_IBL && (gl.image < 0 || static_cast<uint32_t>(gl.image) >= d.num_images || d.images[gl.image].channels != 4))
            return refuse(GBL_ERR_INVALID, "image based light " + std::to_string(i) + ": bad image index", err);
        if (gl.type > GBL_LIGHT_IBL) return refuse(GBL_ERR_INVALID, "unknown light type", err);
    }
    // an emissive instance emits through an AREA light: the path kernels' MIS test instances[hit].area_light == picked light
    // can then only hold for an area light (render_kernels.h skips the capped vertex's ray on that ground)
    for (uint32_t i = 0; i < d.num_instances; ++i)
        if (d.instances[i].area_light >= 0 && d.lights[d.instances[i].area_light].type != GBL_LIGHT_AREA)
            return refuse(GBL_ERR_INVALID, "instance " + std::to_string(i) + ": area_light names a light that is not an area light", err);
    return GBL_OK;
}

gbl_status validate_volume(const gbl_volume& g, std::string* err) {
    if (g.type == GBL_VOLUME_NONE || g.type == GBL_VOLUME_HOMOGENEOUS) return GBL_OK;
    if (g.type != GBL_VOLUME_HETEROGENEOUS) return refuse(GBL_ERR_INVALID, "unknown volume type", err);
    if (g.grid[0] <= 0 || g.grid[1] <= 0 || g.grid[2] <= 0 || (g.grid_channels != 1 && g.grid_channels != 3) || g.density == nullptr)
        return refuse(GBL_ERR_INVALID, "heterogeneous volume: the density grid needs positive dimensions, 1 or 3 channels and its data", err);
    // the march loops of kernels/medium.h advance t by step_size: zero, negative, NaN or a step below the float spacing
    // of t never terminates -- a spin on the reference's CPU, an unrecoverable hang on a GPU
    if (!(g.step_size > 0.0f) || !std::isfinite(g.step_size))
        return refuse(GBL_ERR_INVALID, "heterogeneous volume: step_size must be a positive finite number", err);
    // the device indexes the grid with 32-bit ints
    const uint64_t cells = static_cast<uint64_t>(g.grid[0]) * static_cast<uint64_t>(g.grid[1]);
    if (cells > (1ull << 31) || cells * static_cast<uint64_t>(g.grid[2]) > (1ull << 31) ||
        cells * static_cast<uint64_t>(g.grid[2]) * static_cast<uint64_t>(g.grid_channels) >= (1ull << 31))
        return refuse(GBL_ERR_INVALID, "heterogeneous volume: the density grid holds 2^31 values or more", err);
    // bounded at the 10^6 points the stream sampler's draw budget assumes (api_render.hip medium_draws_per_sample) -- a step
    // of 1e-12 is a hang, not a render
    if (!(march_diagonal(region_of(g)) / double(g.step_size) <= 1.0e6))
        return refuse(GBL_ERR_INVALID, "heterogeneous volume: step_size is too small for the region (more than 10^6 steps across it)", err);
    return GBL_OK;
}

gbl_status validate_film(const gbl_film& f, std::string* err) {
    if (f.xres <= 0 || f.yres <= 0) return refuse(GBL_ERR_INVALID, "film resolution must be positive", err);
    if (!(f.filter_width[0] > 0.0f) || !(f.filter_width[1] > 0.0f) || filter_halo(f) > GBL_MAX_FILTER_HALO)
        return refuse(GBL_ERR_UNSUPPORTED, "filter width must be in (0, " + std::to_string(GBL_MAX_FILTER_HALO - 0.5f) + "] pixels", err);
    return GBL_OK;
}

// Every refusal pack_scene makes, in a fixed order (a description with two faults reports the earlier section's), before
// anything is packed: writes nothing but *err.
gbl_status validate_desc(const gbl_scene_desc* d, std::string* err) {
    if (!d || d->abi_version != GBL_ABI_VERSION) return refuse(GBL_ERR_INVALID, "scene description has the wrong abi_version", err);
    if (d->camera.type > GBL_CAMERA_ORTHOGRAPHIC) return refuse(GBL_ERR_INVALID, "unknown camera type", err);
    for (uint32_t i = 0; i < d->num_instances; ++i)
        if (d->instances[i].mesh >= d->num_meshes || d->instances[i].material >= d->num_materials || d->instances[i].area_light >= static_cast<int32_t>(d->num_lights))
            return refuse(GBL_ERR_INVALID, "instance " + std::to_string(i) + " references a mesh/material/light out of range", err);
    gbl_status st = validate_meshes(*d, err);
    Trs t;
    for (uint32_t i = 0; i < d->num_instances && st == GBL_OK; ++i)
        if (!instance_transform(d->instances[i], i, &t, err)) st = GBL_ERR_INVALID;
    if (st == GBL_OK) st = validate_materials(*d, err);
    if (st == GBL_OK) st = validate_images(*d, err);
    if (st == GBL_OK) st = validate_textures(*d, err);
    if (st == GBL_OK) st = validate_lights(*d, err);
    if (st == GBL_OK) st = validate_volume(d->volume, err);
    if (st == GBL_OK) st = validate_film(d->film, err);
    return st;
}

// The TLAS over instance primitives (box, centre, id = instance index): what build_tlas and build_tlas_nodes share
void tlas_over(std::vector<Prim>& iprims, int32_t tlas_base, std::vector<DevNode>* nodes, int32_t* root_out, int* depth_out) {
    const int kTlasCap = 22;
    nodes->clear();
    *depth_out = 0;
    *root_out = 0;
    if (iprims.empty()) return;
    Builder tb(iprims, 1, kTlasCap);
    int root = tb.build(0, iprims.size(), 1);
    Flat4 t4(tb, *nodes, tlas_base);
    auto inst_ref = [&](uint32_t first, uint32_t) { return ~static_cast<int32_t>(iprims[first].id << 2); };
    *root_out = t4.emit(root, 1, inst_ref);
    *depth_out = t4.depth;
}

}  // namespace

int scene_stack_entries(const std::vector<DevNode>& tlas, int32_t tlas_base, int32_t tlas_root, const std::vector<DevInstance>& instances,
                        const std::vector<int>& mesh_stack_need) {
    return 1 + tlas_stack_need(tlas, tlas_base, tlas_root, instances, mesh_stack_need) + 1;
}

// Instances (transforms in the reference's float order, world boxes by Transform::onBBox) and the TLAS over them.
// TLAS node k gets device index tlas_base + k; bound_lo/hi return the union of the instance boxes.
gbl_status build_tlas(const TlasInput& in, TlasResult* out, std::string* err) {
    out->instances.resize(in.count);
    out->instance_bounds.resize(in.count);
    out->nodes.clear();
    std::vector<Prim> iprims(in.count);
    Aabb scene_bound;
    for (uint32_t i = 0; i < in.count; ++i) {
        const gbl_instance& gi = in.instances[i];
        Trs t;
        if (!instance_transform(gi, i, &t, err)) return GBL_ERR_INVALID;
        DevInstance& di = out->instances[i];
        memset(&di, 0, sizeof(di));
        store3x4(t.m, di.m);
        store3x4(t.inv, di.inv);
        di.root = in.mesh_root[gi.mesh];
        di.material = static_cast<int32_t>(gi.material);
        di.area_light = gi.area_light;
        di.mesh = static_cast<int32_t>(gi.mesh);
        di.shape = in.meshes[gi.mesh].shape;
        di.radius = in.meshes[gi.mesh].radius;
        // MaskMaterial ORs BSDFnullptr into its type; SubsurfaceMaterial's type is BSDFAll, which holds the bit as well
        di.is_mask = (in.materials[gi.material].type == GBL_MAT_MASK || in.materials[gi.material].type == GBL_MAT_SUBSURFACE) ? 1u : 0u;
        // Transform::onBBox: the 8 corners of the mesh bound
        const float *lo = in.mesh_lo + 3 * gi.mesh, *hi = in.mesh_hi + 3 * gi.mesh;
        Prim& p = iprims[i];
        for (int c = 0; c < 8; ++c) {
            float corner[3] = {(c & 1) ? hi[0] : lo[0], (c & 2) ? hi[1] : lo[1], (c & 4) ? hi[2] : lo[2]};
            float w[3];
            point_by(t.m, corner, w);
            p.box.grow(w);
        }
        for (int k = 0; k < 3; ++k) p.c[k] = 0.5f * (p.box.lo[k] + p.box.hi[k]);
        store_bound(p.box, out->instance_bounds[i].lo, out->instance_bounds[i].hi);
        p.id = i;
        scene_bound.grow(p.box.lo);
        scene_bound.grow(p.box.hi);
    }
    store_bound(scene_bound, out->bound_lo, out->bound_hi);
    tlas_over(iprims, in.tlas_base, &out->nodes, &out->root, &out->depth);
    return GBL_OK;
}

void build_tlas_nodes(const DevInstanceBound* bounds, uint32_t count, int32_t tlas_base, std::vector<DevNode>* nodes, int32_t* root, int* depth) {
    std::vector<Prim> iprims(count);
    for (uint32_t i = 0; i < count; ++i) {   // the primitives build_tlas makes: it stores exactly these boxes
        Prim& p = iprims[i];
        for (int k = 0; k < 3; ++k) {
            p.box.lo[k] = bounds[i].lo[k];
            p.box.hi[k] = bounds[i].hi[k];
            p.c[k] = 0.5f * (p.box.lo[k] + p.box.hi[k]);
        }
        p.id = i;
    }
    tlas_over(iprims, tlas_base, nodes, root, depth);
}

bool pack_transform(const gbl_trs& to_world, uint32_t i, float m[12], float inv[12], std::string* err) {
    gbl_instance gi;
    memset(&gi, 0, sizeof(gi));
    gi.to_world = to_world;
    Trs t;
    if (!instance_transform(gi, i, &t, err)) return false;
    store3x4(t.m, m);
    store3x4(t.inv, inv);
    return true;
}

bool camera_extended(const gbl_camera& c) { return c.lens_radius != 0.0f || c.type != GBL_CAMERA_PERSPECTIVE; }

void pack_camera(const gbl_camera& c, const gbl_film& film, DevCamera* out) {
    memset(out, 0, sizeof(*out));
    for (int k = 0; k < 3; ++k) out->pos[k] = c.position[k];
    for (int k = 0; k < 4; ++k) out->q[k] = c.orientation[k];
    float aspect = static_cast<float>(film.xres) / static_cast<float>(film.yres);
    float fov = kPi * (c.fov_degrees / 180.0f);
    float ys = 1.0f / std::tan(fov / 2.0f);
    out->proj11 = ys;
    out->proj00 = ys / aspect;
    out->inv_xres = 1.0f / static_cast<float>(film.xres);
    out->inv_yres = 1.0f / static_cast<float>(film.yres);
    out->type = c.type;
    out->lens_radius = c.lens_radius;
    out->focal_distance = c.focal_distance;
    out->film_w = c.film_width;              // OrthographicCamera ctor, GoblinCamera.cpp:288-296
    out->film_h = c.film_width / aspect;
}

// ------------------------------------------------------------------ geometry
namespace {
// BVH::buildLinearBVH (GoblinBVH.cpp:81-151) with the EqualCount split, followed only as far as the SHAPE of the tree:
// per triangle the root-to-leaf path, the split axes along it and its place in a multi-triangle leaf.
void reference_order(std::vector<Prim>& it, uint32_t start, uint32_t end, uint32_t depth, uint32_t path, uint64_t axes, DevTriOrder* out) {
    auto leaf = [&]() {
        for (uint32_t i = start; i < end; ++i) {
            DevTriOrder& o = out[it[i].id];
            o.path = path;
            o.axes_lo = static_cast<uint32_t>(axes);
            o.axes_hi = static_cast<uint32_t>(axes >> 32);
            o.depth_rank = depth | ((i - start) << 8);
        }
    };
    if (end - start == 1 || depth >= 32) return leaf();
    float clo[3] = {INFINITY, INFINITY, INFINITY}, chi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (uint32_t i = start; i < end; ++i)
        for (int k = 0; k < 3; ++k) {
            clo[k] = std::min(clo[k], it[i].c[k]);
            chi[k] = std::max(chi[k], it[i].c[k]);
        }
    const float dx = chi[0] - clo[0], dy = chi[1] - clo[1], dz = chi[2] - clo[2];
    const int dim = (dx > dy && dx > dz) ? 0 : (dy > dz ? 1 : 2);   // BBox::longestAxis, GoblinBBox.cpp:79-88
    if (clo[dim] == chi[dim]) return leaf();
    const uint32_t mid = (start + end) / 2;
    std::nth_element(&it[start], &it[mid], &it[end - 1] + 1, [dim](const Prim& a, const Prim& b) { return a.c[dim] < b.c[dim]; });
    axes |= static_cast<uint64_t>(dim) << (2 * depth);
    reference_order(it, start, mid, depth + 1, path, axes, out);
    reference_order(it, mid, end, depth + 1, path | (1u << depth), axes, out);
}
}   // namespace

void mesh_reference_order(const float* positions, const uint32_t* indices, uint32_t tri_count, DevTriOrder* out) {
    for (uint32_t t = 0; t < tri_count; ++t) out[t] = DevTriOrder();
    if (tri_count == 0) return;
    std::vector<Prim> items = triangle_prims(MeshView{positions, nullptr, nullptr, indices}, tri_count);   // BVHPrimitiveInfo (GoblinBVH.cpp:8-14)
    reference_order(items, 0, tri_count, 0, 0u, 0ull, out);
}

void mesh_object_bound(const float* positions, uint32_t vertex_count, float lo[3], float hi[3]) {
    Aabb bound;
    for (uint32_t v = 0; v < vertex_count; ++v) bound.grow(positions + 3 * static_cast<size_t>(v));
    store_bound(bound, lo, hi);
}

namespace {

// The vertex attributes used at shading time
void pack_attributes(const gbl_scene_desc& d, PackedScene* out) {
    out->positions.assign(d.positions, d.positions + 3 * static_cast<size_t>(d.num_vertices));
    out->normals.assign(d.normals, d.normals + 3 * static_cast<size_t>(d.num_vertices));
    out->uvs.assign(d.uvs, d.uvs + 2 * static_cast<size_t>(d.num_vertices));
}

// Per triangle of every mesh: the reference's visiting order (DevTriOrder) and the triangle's own bound (the reference
// BLAS's leaf boxes, DevTriBound)
void pack_tri_order_and_bounds(const gbl_scene_desc& d, PackedScene* out) {
    out->tri_order.assign(d.num_triangles, DevTriOrder());
    out->tri_bounds.assign(d.num_triangles, DevTriBound());
    for (uint32_t mi = 0; mi < d.num_meshes; ++mi) {
        const gbl_mesh& gm = d.meshes[mi];
        if (gm.shape != GBL_SHAPE_MESH) continue;
        const MeshView mv = view_of(d, gm);
        mesh_reference_order(mv.P, mv.I, gm.tri_count, out->tri_order.data() + gm.tri_offset);
        for (uint32_t t = 0; t < gm.tri_count; ++t) {
            DevTriBound& b = out->tri_bounds[gm.tri_offset + t];
            memset(&b, 0, sizeof(b));
            const float *a = mv.p(t, 0), *bb = mv.p(t, 1), *c = mv.p(t, 2);
            for (int k = 0; k < 3; ++k) {
                b.lo[k] = std::min(std::min(a[k], bb[k]), c[k]);
                b.hi[k] = std::max(std::max(a[k], bb[k]), c[k]);
            }
        }
    }
}

// The SAH tree over one mesh's triangles, appended to `nodes`, and its triangles in leaf order, appended to `tris`
void build_host_blas(const gbl_mesh& gm, const MeshView& mv, uint32_t mi, PackedScene* out) {
    const int kBlasCap = 40;
    std::vector<Prim> prims = triangle_prims(mv, gm.tri_count);
    const int leaf_knob = [] { const char* e = getenv("GBL_MAX_LEAF"); return e ? std::max(1, std::min(GBL_MAX_LEAF_TRIS, atoi(e))) : GBL_MAX_LEAF_TRIS; }();
    Builder b(prims, leaf_knob, kBlasCap);
    int root = b.build_parallel(prims.size());
    Flat4 f4(b, out->nodes);
    const uint32_t tri_base = static_cast<uint32_t>(out->tris.size());
    for (const Prim& p : prims) {
        const float *p0 = mv.p(p.id, 0), *p1 = mv.p(p.id, 1), *p2 = mv.p(p.id, 2);
        DevTri t;
        memset(&t, 0, sizeof(t));
        for (int k = 0; k < 3; ++k) t.p0[k] = p0[k], t.e1[k] = p1[k] - p0[k], t.e2[k] = p2[k] - p0[k];
        t.shade = gm.tri_offset + p.id;
        t.flags = tri_flags(gm);
        out->tris.push_back(t);
    }
    auto leaf_ref = [&](uint32_t first, uint32_t count) { return ~static_cast<int32_t>(((tri_base + first) << 2) | (count - 1)); };
    out->mesh_root[mi] = f4.emit(root, 1, leaf_ref);
    out->blas_max_depth = std::max(out->blas_max_depth, f4.depth);
    out->mesh_stack_need[mi] = blas_stack_need(out->nodes, out->mesh_root[mi]);
}

// One mesh: its object bound, root reference and shading records; the tree itself unless the device builds it (kernels/lbvh.h
// then makes the tree and the DevTri order)
void pack_blas(const gbl_scene_desc& d, uint32_t mi, bool device_blas, PackedScene* out) {
    const gbl_mesh& gm = d.meshes[mi];
    Aabb bound;
    if (gm.shape != GBL_SHAPE_MESH) {
        // Sphere / Disk::getObjectBound (GoblinSphere.cpp:140-143, GoblinDisk.cpp:81-84); no BLAS: the
        // instance's root is a marker reference and the traversal tests the shape analytically
        const float r = gm.radius, z = gm.shape == GBL_SHAPE_SPHERE ? gm.radius : 0.0f;
        float hi[3] = {r, r, z}, lo[3] = {-r, -r, -z};
        bound.grow(hi);
        bound.grow(lo);
        out->mesh_root[mi] = gm.shape == GBL_SHAPE_SPHERE ? GBL_REF_SPHERE : GBL_REF_DISK;
        out->extended = 1;
    } else {
        const MeshView mv = view_of(d, gm);
        for (uint32_t v = 0; v < gm.vertex_count; ++v) bound.grow(mv.P + 3 * v);
        for (uint32_t t = 0; t < gm.tri_count; ++t) {
            DevTriShade& s = out->tri_shade[gm.tri_offset + t];
            for (int k = 0; k < 3; ++k) s.v[k] = gm.vertex_offset + mv.I[3 * t + k];
            s.flags = tri_flags(gm);
        }
        if (!device_blas) build_host_blas(gm, mv, mi, out);   // (a device build patches the root, 0 until then, after its build)
    }
    store_bound(bound, &out->mesh_lo[3 * mi], &out->mesh_hi[3 * mi]);
}

// One BLAS per mesh, then the triangle bounds in the order of `tris` (what the kernels index with a hit's triangle; a device
// build gathers them itself)
void pack_meshes(const gbl_scene_desc& d, bool device_blas, PackedScene* out) {
    out->tris.clear();
    out->tri_shade.assign(d.num_triangles, DevTriShade());
    out->blas_max_depth = 0;
    out->mesh_stack_need.assign(d.num_meshes, 0);
    out->mesh_root.assign(d.num_meshes, 0);
    out->mesh_lo.resize(3 * d.num_meshes);
    out->mesh_hi.resize(3 * d.num_meshes);
    for (uint32_t mi = 0; mi < d.num_meshes; ++mi) pack_blas(d, mi, device_blas, out);
    out->blas_nodes = out->nodes.size();
    out->tri_bounds_leaf.resize(out->tris.size());
    for (size_t i = 0; i < out->tris.size(); ++i) out->tri_bounds_leaf[i] = out->tri_bounds[out->tris[i].shade];
}

// The instance records and the TLAS behind the BLAS nodes; returns the scene bound: BVH::getAABB of the scene BVH, the union
// of the instance boxes (GoblinBVH.cpp:46-50)
gbl_status pack_instances(const gbl_scene_desc& d, PackedScene* out, Aabb* scene_bound, std::string* err) {
    out->tlas_base = static_cast<int32_t>(out->nodes.size());
    out->tlas_capacity = std::max<uint32_t>(1u, d.num_instances);
    const TlasInput in = {d.instances,         d.num_instances,       d.meshes,     d.materials, out->mesh_lo.data(),
                          out->mesh_hi.data(), out->mesh_root.data(), out->tlas_base};
    TlasResult tlas;
    const gbl_status st = build_tlas(in, &tlas, err);
    if (st != GBL_OK) return st;
    out->instances.swap(tlas.instances);
    out->instance_bounds.swap(tlas.instance_bounds);
    out->tlas_root = tlas.root;
    out->tlas_depth = tlas.depth;
    for (const DevInstance& di : out->instances)
        if (di.is_mask) out->has_masks = out->extended = 1;
    scene_bound->grow(tlas.bound_lo);
    scene_bound->grow(tlas.bound_hi);
    out->nodes.insert(out->nodes.end(), tlas.nodes.begin(), tlas.nodes.end());
    out->tlas_nodes = tlas.nodes.size();
    // room for any TLAS over the same instances (gbl_update_instances rebuilds it in place)
    out->nodes.resize(static_cast<size_t>(out->tlas_base) + out->tlas_capacity, DevNode());
    // (with device-built BLASes the caller fills mesh_stack_need from their depths and calls scene_stack_entries again)
    out->stack_entries = scene_stack_entries(tlas.nodes, out->tlas_base, out->tlas_root, out->instances, out->mesh_stack_need);
    return GBL_OK;
}

// ------------------------------------------- materials, images and textures
// One material's record: its type and slots, a mask's view of the material it wraps, then the editable fields (kernels/materials.h
// mat_compose, which the device edit runs as well).  `all` is the description's whole list: a mask reads the one it wraps.
void pack_material(const gbl_material* all, uint32_t i, DevMaterial* out) {
    const gbl_material& m = all[i];
    DevMaterial& dm = *out;
    memset(&dm, 0, sizeof(dm));
    dm.type = m.type;
    dm.tex_color = m.tex_color;
    dm.tex_color2 = m.tex_color2;
    dm.tex_exponent = m.tex_exponent;
    dm.has_tex = (m.tex_color >= 0 || m.tex_color2 >= 0 || m.tex_exponent >= 0) ? 1u : 0u;
    dm.masked = m.type == GBL_MAT_MASK ? m.masked_material : -1;
    dm.tex_color3 = -1;
    // Material::perturb -> BumpShaders::evaluate; MaskMaterial::perturb forwards to the wrapped material (GoblinMaterial.h:456-458)
    const gbl_material& bump_of = m.type == GBL_MAT_MASK ? all[m.masked_material] : m;
    dm.tex_bump = bump_of.tex_bump;
    dm.tex_normal = bump_of.tex_normal;
    if (dm.tex_bump >= 0 || dm.tex_normal >= 0) dm.has_tex = 1u;
    if (m.type == GBL_MAT_SUBSURFACE) {
        dm.tex_color3 = m.tex_color3;
        dm.has_tex = 1u;   // its fragments always carry dpdu / dpdv: BSSRDF::sampleProbeRay and MISWeight read them
    }
    if (m.type == GBL_MAT_MASK) {
        const gbl_material& in = all[m.masked_material];
        if (in.tex_color >= 0 || in.tex_color2 >= 0 || in.tex_exponent >= 0) dm.has_tex = 1u;
    }
    // colours, index, k, and the exponent: a subsurface material's is A of the BSSRDF ctor (GoblinMaterial.cpp:32-38)
    float row[GBL_MAT_ROW_FLOATS];
    mat_row_of(m, row);
    mat_compose(&dm, row);
}

void pack_materials(const gbl_scene_desc& d, PackedScene* out) {
    out->materials.resize(d.num_materials);
    for (uint32_t i = 0; i < d.num_materials; ++i) {
        const gbl_material& m = d.materials[i];
        pack_material(d.materials, i, &out->materials[i]);
        if (m.type == GBL_MAT_SUBSURFACE) out->has_bssrdf = out->extended = 1;
        for (int32_t t : texture_slots(m))
            if (t >= 0) out->extended = 1;
    }
}

// The pyramids arrive built (gbl_image); the device wants every level's offset
void pack_images(const gbl_scene_desc& d, PackedScene* out) {
    out->images.resize(d.num_images);
    for (uint32_t i = 0; i < d.num_images; ++i) {
        const gbl_image& gi = d.images[i];
        DevImage& di = out->images[i];
        memset(&di, 0, sizeof(di));
        di.width = gi.width, di.height = gi.height, di.levels = gi.levels, di.channels = gi.channels;
        di.offset = gi.texel_offset;
        uint64_t off = 0;
        for (uint32_t l = 0; l < gi.levels; ++l) {
            di.level_offset[l] = static_cast<uint32_t>(off);
            off += level_texels(gi, l);
        }
    }
    // MIPMap<T>::initEWALut (GoblinTexture.cpp:262-271)
    out->ewa_lut.resize(128);
    for (int i = 0; i < 128; ++i) {
        const float r2 = static_cast<float>(i) / static_cast<float>(128 - 1);
        out->ewa_lut[i] = expf(-2.0f * r2) - expf(-2.0f);
    }
}

// One texture's record: everything but value and the uv mapping, then those (kernels/materials.h tex_compose)
void pack_texture(const gbl_texture& g, DevTexture* out) {
    DevTexture& t = *out;
    memset(&t, 0, sizeof(t));
    t.type = g.type;
    t.is_float = g.is_float;
    t.child[0] = g.child[0], t.child[1] = g.child[1];
    t.mapping = g.mapping;
    t.filter = g.type == GBL_TEX_IMAGE ? g.image_filter : g.filter;
    t.image = g.type == GBL_TEX_IMAGE ? g.image : -1;
    t.address = g.address;
    t.max_aniso = g.max_anisotropy;
    if ((g.type == GBL_TEX_CHECKERBOARD || g.type == GBL_TEX_IMAGE) && g.mapping == GBL_MAP_SPHERICAL) {
        Trs tt = compose(g.to_tex.position, g.to_tex.orientation, g.to_tex.scale);   // SphericalMapping::mToTex
        store3x4(tt.m, t.to_tex);
    }
    float row[GBL_TEX_ROW_FLOATS];
    tex_row_of(g, row);
    tex_compose(&t, row);
}

void pack_textures(const gbl_scene_desc& d, PackedScene* out) {
    out->textures.resize(d.num_textures);
    for (uint32_t i = 0; i < d.num_textures; ++i) pack_texture(d.textures[i], &out->textures[i]);
}

// -------------------------------------------------------------------- lights
// CDF1D::init over f[0 .. n): the normalised cdf[0 .. n], returns the integral
float cdf1d(const float* f, size_t n, std::vector<float>* cdf) {
    const float dx = 1.0f / n;
    cdf->assign(n + 1, 0.0f);
    for (size_t k = 1; k < n + 1; ++k) (*cdf)[k] = (*cdf)[k - 1] + (f[k - 1] * dx);
    const float integral = (*cdf)[n];
    for (size_t k = 1; k < n + 1; ++k) (*cdf)[k] /= integral;
    return integral;
}

// Scene::getBoundingSphere's radius: the full diagonal of the scene bound (GoblinBBox.h:51-54)
float bounding_radius(const Aabb& b) {
    const float dx = b.hi[0] - b.lo[0], dy = b.hi[1] - b.lo[1], dz = b.hi[2] - b.lo[2];
    return std::sqrt(dx * dx + dy * dy + dz * dz);
}

float luminance(const float c[3]) { return 0.212671f * c[0] + 0.715160f * c[1] + 0.072169f * c[2]; }

// Luminance of a light's power c * k1 * k2, each channel multiplied in that order
float power_of(const float c[3], float k1, float k2 = 1.0f) {
    const float p[3] = {c[0] * k1 * k2, c[1] * k1 * k2, c[2] * k1 * k2};
    return luminance(p);
}

struct Quat { float w, x, y, z; };
Quat qmul(const Quat& a, const Quat& b) {   // GoblinQuaternion.h:45-48
    const float d3 = a.x * b.x + a.y * b.y + a.z * b.z;
    Quat r;
    r.w = a.w * b.w - d3;
    r.x = a.w * b.x + b.w * a.x + (a.y * b.z - a.z * b.y);
    r.y = a.w * b.y + b.w * a.y + (a.z * b.x - a.x * b.z);
    r.z = a.w * b.z + b.w * a.z + (a.x * b.y - a.y * b.x);
    return r;
}
Quat qnorm(const Quat& q) {   // normalize(Quaternion), GoblinQuaternion.cpp:94-100
    const float inv = 1.0f / sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
    return Quat{q.w * inv, q.x * inv, q.y * inv, q.z * inv};
}
Quat axis_angle(int axis, float angle) {   // Quaternion(axis, angle), GoblinQuaternion.cpp:9-15 (unit axes x = 0, y = 1)
    const float t = angle * 0.5f, st = sinf(t);
    return Quat{cosf(t), axis == 0 ? 1.0f * st : 0.0f * st, axis == 1 ? 1.0f * st : 0.0f * st, 0.0f * st};
}

// Light::setOrientation (GoblinLight.cpp:66-76): direction -> basis -> matrix -> quaternion (w x y z)
void orientation_of(const float dir[3], float q[4]) {
    float xa[3], ya[3];
    if (fabsf(dir[0]) > fabsf(dir[1])) {
        float il = 1.0f / sqrtf(dir[0] * dir[0] + dir[2] * dir[2]);
        xa[0] = -dir[2] * il; xa[1] = 0.0f; xa[2] = dir[0] * il;
    } else {
        float il = 1.0f / sqrtf(dir[1] * dir[1] + dir[2] * dir[2]);
        xa[0] = 0.0f; xa[1] = -dir[2] * il; xa[2] = dir[1] * il;
    }
    ya[0] = dir[1] * xa[2] - dir[2] * xa[1];
    ya[1] = dir[2] * xa[0] - dir[0] * xa[2];
    ya[2] = dir[0] * xa[1] - dir[1] * xa[0];
    float R[3][3] = {{xa[0], ya[0], dir[0]}, {xa[1], ya[1], dir[1]}, {xa[2], ya[2], dir[2]}};
    float qv[4];   // x y z w
    float trace = R[0][0] + R[1][1] + R[2][2];
    if (trace > 0.0f) {
        float s = std::sqrt(trace + 1.0f);
        qv[3] = s * 0.5f;
        float t = 0.5f / s;
        qv[0] = (R[2][1] - R[1][2]) * t;
        qv[1] = (R[0][2] - R[2][0]) * t;
        qv[2] = (R[1][0] - R[0][1]) * t;
    } else {
        int a = 0;
        if (R[1][1] > R[0][0]) a = 1;
        if (R[2][2] > R[a][a]) a = 2;
        int b2 = (a + 1) % 3, c2 = (b2 + 1) % 3;
        float s = std::sqrt(R[a][a] - R[b2][b2] - R[c2][c2] + 1.0f);
        qv[a] = s * 0.5f;
        float t = s != 0.0f ? 0.5f / s : s;
        qv[3] = (R[c2][b2] - R[b2][c2]) * t;
        qv[b2] = (R[b2][a] + R[a][b2]) * t;
        qv[c2] = (R[c2][a] + R[a][c2]) * t;
    }
    q[0] = qv[3]; q[1] = qv[0]; q[2] = qv[1]; q[3] = qv[2];
}

const float kOne[3] = {1.0f, 1.0f, 1.0f}, kZero[3] = {0.0f, 0.0f, 0.0f};

// Spot and directional lights: the axis the light works with is the third column of the matrix of its orientation.  The
// spot light's ctor normalises the direction, the directional light's does not (GoblinLight.cpp:136-143).
float pack_aimed_light(const gbl_light& gl, const Aabb& scene_bound, DevLight* dl) {
    const bool spot = gl.type == GBL_LIGHT_SPOT;
    float dir[3] = {gl.direction[0], gl.direction[1], gl.direction[2]};
    if (spot) {
        float inv_len = 1.0f / std::sqrt(dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2]);
        for (int k = 0; k < 3; ++k) dir[k] *= inv_len;
    }
    float q[4];
    orientation_of(dir, q);
    const Trs t = compose(spot ? gl.position : kZero, q, kOne);
    for (int k = 0; k < 3; ++k) dl->axis[k] = t.m.v[k][0] * 0.0f + t.m.v[k][1] * 0.0f + t.m.v[k][2] * 1.0f;
    if (spot) return power_of(dl->color, kTwoPi, 1.0f - 0.5f * (dl->cos_max + dl->cos_falloff));
    // DirectionalLight::power (:203-210): radius^2 * PI * radiance over Scene::getBoundingSphere
    const float radius = bounding_radius(scene_bound);
    return power_of(dl->color, radius * radius * kPi);
}

// A mesh light's triangles with the CDF1D over their areas; returns the sum of the areas
float pack_light_tris(const gbl_scene_desc& d, const gbl_mesh& gm, PackedScene* out, DevLight* dl) {
    const MeshView mv = view_of(d, gm);
    dl->tri_first = static_cast<uint32_t>(out->light_tris.size());
    dl->tri_count = gm.tri_count;
    std::vector<float> areas(gm.tri_count), cdf;
    float sum = 0.0f;
    for (uint32_t k = 0; k < gm.tri_count; ++k) {
        const float *p0 = mv.p(k, 0), *p1 = mv.p(k, 1), *p2 = mv.p(k, 2);
        float e1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
        float e2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
        float cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
        areas[k] = 0.5f * std::sqrt(cx * cx + cy * cy + cz * cz);
        sum += areas[k];
    }
    cdf1d(areas.data(), areas.size(), &cdf);
    for (uint32_t k = 0; k < gm.tri_count; ++k) {
        DevLightTri lt;
        memset(&lt, 0, sizeof(lt));
        for (int c = 0; c < 3; ++c) {
            lt.p0[c] = mv.p(k, 0)[c], lt.p1[c] = mv.p(k, 1)[c], lt.p2[c] = mv.p(k, 2)[c];
            lt.n0[c] = mv.n(k, 0)[c], lt.n1[c] = mv.n(k, 1)[c], lt.n2[c] = mv.n(k, 2)[c];
        }
        lt.area = areas[k];
        lt.cdf_lo = cdf[k], lt.cdf_hi = cdf[k + 1];
        lt.has_normal = gm.has_normal ? 1.0f : 0.0f;
        out->light_tris.push_back(lt);
    }
    return sum;
}

// AreaLight over a mesh's triangles or, as a GeometrySet over one intersectable geometry (GoblinLight.cpp:289-303), a sphere / disk:
// the emitting geometry, which no light edit changes ...
void attach_area_geometry(const gbl_scene_desc& d, const gbl_light& gl, PackedScene* out, DevLight* dl) {
    const gbl_mesh& gm = d.meshes[gl.mesh];
    if (gm.shape != GBL_SHAPE_MESH) {
        out->extended = 1;
        dl->shape = gm.shape, dl->radius = gm.radius;
        const float a = gm.shape == GBL_SHAPE_SPHERE ? 4.0f * kPi * gm.radius * gm.radius : kPi * gm.radius * gm.radius;
        dl->sum_area = 0.0f + a;   // the set's sum over its one geometry
    } else {
        dl->sum_area = pack_light_tris(d, gm, out, dl);
    }
}
// ... and its transform, with the power over the world area
float pack_area_light(const gbl_light& gl, DevLight* dl) {
    const Trs t = compose(gl.to_world.position, gl.to_world.orientation, gl.to_world.scale);
    store3x4(t.m, dl->m);
    store3x4(t.inv, dl->inv);
    const float world_area = dl->sum_area * (gl.to_world.scale[0] * gl.to_world.scale[1]);
    return power_of(dl->color, kPi, world_area);
}

// The environment map's texels, AddressRepeat
struct IblTexels {
    const DevImage& im;
    const float* texels;
    int width(uint32_t level) const { return static_cast<int>(std::max(1u, im.width >> level)); }
    int height(uint32_t level) const { return static_cast<int>(std::max(1u, im.height >> level)); }
    float at(uint32_t level, int s, int t, int c) const {
        const int w = width(level), h = height(level);
        s %= w; t %= h;
        if (s < 0) s += w;
        if (t < 0) t += h;
        return texels[im.offset + im.level_offset[level] + (static_cast<size_t>(t) * w + s) * 4 + c];
    }
};

// CDF1D::init as a block of the device's distribution table: func[n], cdf[n + 1], integral
float append_cdf_block(const std::vector<float>& f, std::vector<float>* block) {
    std::vector<float> cdf;
    const float integral = cdf1d(f.data(), f.size(), &cdf);
    block->insert(block->end(), f.begin(), f.end());
    block->insert(block->end(), cdf.begin(), cdf.end());
    block->push_back(integral);
    return integral;
}

// The IBL's sampling distribution: luminance * sin(theta) of level max(0, maxLevel - 8), as a CDF2D (marginal block, then the rows')
void pack_ibl_distribution(const IblTexels& tx, PackedScene* out, DevLight* dl) {
    const uint32_t level = tx.im.levels > 9 ? tx.im.levels - 1 - 8 : 0;
    const int dw = tx.width(level), dh = tx.height(level);
    dl->dist_offset = static_cast<uint32_t>(out->ibl_dist.size());
    dl->dist_w = static_cast<uint32_t>(dw), dl->dist_h = static_cast<uint32_t>(dh);
    std::vector<float> rows_block, row_integrals, marginal_block, sin_table;
    ibl_sin_theta(static_cast<uint32_t>(dh), &sin_table);
    for (int r = 0; r < dh; ++r) {
        const float sin_theta = sin_table[r];
        std::vector<float> f(dw);
        for (int c = 0; c < dw; ++c) {
            const float rgb[3] = {tx.at(level, c, r, 0), tx.at(level, c, r, 1), tx.at(level, c, r, 2)};
            f[c] = luminance(rgb) * sin_theta;
        }
        row_integrals.push_back(append_cdf_block(f, &rows_block));
    }
    append_cdf_block(row_integrals, &marginal_block);
    out->ibl_dist.insert(out->ibl_dist.end(), marginal_block.begin(), marginal_block.end());
    out->ibl_dist.insert(out->ibl_dist.end(), rows_block.begin(), rows_block.end());
}

// ImageBasedLight's constructor (GoblinLight.cpp:464-508): the rotation, which an edit may change ...
void pack_ibl_rotation(const gbl_light& gl, DevLight* dl) {
    // mToWorld.rotateX(-PI / 2); rotateY(-PI / 2); setOrientation(orientation * mToWorld.getOrientation())
    Quat q = {1.0f, 0.0f, 0.0f, 0.0f};
    q = qnorm(qmul(axis_angle(0, -0.5f * kPi), q));
    q = qnorm(qmul(axis_angle(1, -0.5f * kPi), q));
    q = qmul(Quat{gl.to_world.orientation[0], gl.to_world.orientation[1], gl.to_world.orientation[2], gl.to_world.orientation[3]}, q);
    const float qq[4] = {q.w, q.x, q.y, q.z};
    const Trs t = compose(kZero, qq, kOne);
    store3x4(t.m, dl->m);
    store3x4(t.inv, dl->inv);
}
// ... and what its texels decide: the image, the sampling distribution and the power
float attach_ibl_texels(const gbl_scene_desc& d, const gbl_light& gl, const Aabb& scene_bound, PackedScene* out, DevLight* dl) {
    out->extended = 1;
    out->has_ibl = 1;
    dl->image = gl.image;
    const IblTexels tx = {out->images[gl.image], d.texels};
    // mAverageRadiance = mRadiance->lookup(maxLevel, 0, 0): the bilinear lookup of the 1 x 1 level
    const uint32_t max_level = tx.im.levels - 1;
    const float s_res = 0.0f * tx.width(max_level) - 0.5f, t_res = 0.0f * tx.height(max_level) - 0.5f;
    const int s0 = static_cast<int>(floorf(s_res)), t0 = static_cast<int>(floorf(t_res));
    const float ds = s_res - static_cast<float>(s0), dt = t_res - static_cast<float>(t0);
    float avg[3];
    for (int c = 0; c < 3; ++c)
        avg[c] = (1.0f - ds) * (1.0f - dt) * tx.at(max_level, s0, t0, c) + (ds) * (1.0f - dt) * tx.at(max_level, s0 + 1, t0, c) +
                 (1.0f - ds) * (dt)*tx.at(max_level, s0, t0 + 1, c) + (ds) * (dt)*tx.at(max_level, s0 + 1, t0 + 1, c);
    pack_ibl_distribution(tx, out, dl);
    // ImageBasedLight::power (:606-613): mAverageRadiance * PI * (4 PI r^2) over the scene's bounding sphere
    return power_of(avg, kPi, ibl_sphere_area(scene_bound.lo, scene_bound.hi));
}

// Per light: the part the scene's geometry decides (emitting triangles, texels, the Whitted quota), then pack_light for the part
// its gbl_light decides, which returns the light's power; then the power distribution
void pack_lights(const gbl_scene_desc& d, const Aabb& scene_bound, PackedScene* out) {
    out->lights.resize(d.num_lights);
    out->light_tris.clear();
    out->light_power.assign(d.num_lights, 0.0f);
    for (int k = 0; k < 3; ++k) out->bound_lo[k] = scene_bound.lo[k], out->bound_hi[k] = scene_bound.hi[k];
    for (uint32_t i = 0; i < d.num_lights; ++i) {
        const gbl_light& gl = d.lights[i];
        DevLight& dl = out->lights[i];
        memset(&dl, 0, sizeof(dl));
        float texel_power = 0.0f;
        if (gl.type == GBL_LIGHT_DIRECTIONAL) out->extended = 1;
        if (gl.type == GBL_LIGHT_AREA) attach_area_geometry(d, gl, out, &dl);
        if (gl.type == GBL_LIGHT_IBL) texel_power = attach_ibl_texels(d, gl, scene_bound, out, &dl);
        // WhittedRenderer::querySampleQuota: LightSampleIndex(quota, getSamplesNum()) -> roundToSquare slots
        const int root = static_cast<int>(std::ceil(std::sqrt(static_cast<float>(gl.sample_num))));
        dl.wh_n = static_cast<uint32_t>(root * root);
        dl.wh_prefix = static_cast<uint32_t>(out->wh_slots);
        out->wh_slots += static_cast<int32_t>(dl.wh_n);
        out->light_power[i] = pack_light(gl, out->bound_lo, out->bound_hi, texel_power, &dl);
    }
    pack_light_distribution(out->light_power, &out->light_cdf, &out->light_pick_pdf);
}

// ------------------------------------------------------ medium, film, hot prefix
void pack_volume(const gbl_scene_desc& d, const Aabb& scene_bound, PackedScene* out) {
    const gbl_volume& g = d.volume;
    DevVolume& v = out->volume;
    memset(&v, 0, sizeof(v));
    if (g.type == GBL_VOLUME_NONE) return;
    v.on = 1u;
    if (g.type == GBL_VOLUME_HETEROGENEOUS) {
        v.hetero = 1u;
        v.step = g.step_size;
        v.nx = g.grid[0], v.ny = g.grid[1], v.nz = g.grid[2], v.nch = g.grid_channels;
        out->vol_density.assign(g.density, g.density + static_cast<size_t>(v.nx) * v.ny * v.nz * v.nch);
    }
    const VolumeRegion region = region_of(g);
    for (int k = 0; k < 3; ++k) {
        v.attenuation[k] = g.attenuation[k], v.albedo[k] = g.albedo[k], v.emission[k] = g.emission[k];
        v.scatter[k] = g.attenuation[k] * g.albedo[k];
        v.lo[k] = region.lo[k], v.hi[k] = region.hi[k];
        v.normalize[k] = 1.0f / (v.hi[k] - v.lo[k]);
        v.bound_center[k] = 0.5f * (scene_bound.lo[k] + scene_bound.hi[k]);
    }
    v.g = g.g;
    v.sample_num = g.sample_num;
    store3x4(region.to_world.m, v.m);
    store3x4(region.to_world.inv, v.inv);
    v.bound_radius = bounding_radius(scene_bound);
    out->extended = 1;
}

void pack_film(const gbl_film& f, PackedScene* out) {
    DevFilm& df = out->film;
    memset(&df, 0, sizeof(df));
    df.xres = f.xres, df.yres = f.yres;
    df.xstart = ceil_i(f.xres * f.crop[0]);
    df.xcount = std::max(1, ceil_i(f.xres * f.crop[1]) - df.xstart);
    df.ystart = ceil_i(f.yres * f.crop[2]);
    df.ycount = std::max(1, ceil_i(f.yres * f.crop[3]) - df.ystart);
    df.wx = f.filter_width[0], df.wy = f.filter_width[1];
    df.window[0] = floor_i(df.xstart + 0.5f - df.wx);
    df.window[1] = floor_i(df.xstart + 0.5f + df.xcount + df.wx);
    df.window[2] = floor_i(df.ystart + 0.5f - df.wy);
    df.window[3] = floor_i(df.ystart + 0.5f + df.ycount + df.wy);
    df.halo = filter_halo(f);
    const float alpha = f.gaussian_falloff;
    const Filter flt = {f.filter_type, df.wx, df.wy, alpha, expf(-alpha * df.wx * df.wx), expf(-alpha * df.wy * df.wy), f.mitchell_b, f.mitchell_c};
    float norm = flt.norm();
    float dxs = flt.wx / 16, dys = flt.wy / 16;
    for (int y = 0; y < 16; ++y)
        for (int x = 0; x < 16; ++x) out->filter_table[16 * y + x] = flt.eval(x * dxs, y * dys) / norm;
}

bool interior_ref(int32_t r) { return r >= 0 && static_cast<uint32_t>(r) < static_cast<uint32_t>(GBL_REF_NONE); }

// Hot prefix: the nodes every ray starts with, once more, at indices [0, hot_nodes) in breadth-first order.  The lean kernels
// keep as many of them as their LDS has room for beside the traversal stacks (trace.h HotNodes): a reference below hot_nodes is
// served from LDS, anything else from memory.  The originals stay where they were (unreferenced from now on: at most
// GBL_HOT_NODES_MAX * 64 bytes); every interior reference -- child slots, instance roots, mesh roots, the TLAS root -- is
// rewritten to `hot index` or `old index + hot_nodes`, and tlas_base moves with the rest, so gbl_update_instances rebuilds the
// TLAS in the ordinary region and the BLAS part of the prefix stays valid.  (Host-built trees only: the device builder writes
// its nodes on the device.)
void hot_prefix(const gbl_scene_desc& d, PackedScene* out) {
    if (out->nodes.empty() || out->instances.empty()) return;
    uint32_t want = GBL_HOT_NODES_MAX;
    if (const char* e = getenv("GBL_HOT_NODES")) want = static_cast<uint32_t>(std::max(0, std::min(4096, atoi(e))));
    const PackedScene& s = *out;
    std::vector<int32_t> order;          // old indices in breadth-first order: from the TLAS root through the instances' BLAS roots
    std::vector<int32_t> hot_of(s.nodes.size(), -1);
    auto visit = [&](int32_t r) {
        if (interior_ref(r) && static_cast<size_t>(r) < s.nodes.size() && hot_of[r] < 0 && order.size() < want) {
            hot_of[r] = static_cast<int32_t>(order.size());
            order.push_back(r);
        }
    };
    visit(s.tlas_root);
    for (size_t head = 0; head < order.size() && order.size() < want; ++head) {
        const DevNode& nd = s.nodes[order[head]];
        for (int k = 0; k < 4; ++k) {
            const int32_t c = nd.child[k];
            if (interior_ref(c)) {
                visit(c);
            } else if (c < 0 && order[head] >= s.tlas_base) {   // a TLAS leaf: on into the instance's BLAS
                const uint32_t inst = (~static_cast<uint32_t>(c)) >> 2;
                if (inst < s.instances.size() && s.instances[inst].shape == 0u) visit(s.instances[inst].root);
            }
        }
    }
    if (!interior_ref(s.tlas_root))   // a one-instance scene: the TLAS "root" is the instance's leaf reference itself
        for (const DevInstance& di : s.instances)
            if (di.shape == 0u) visit(di.root);
    for (size_t head = 0; head < order.size() && order.size() < want; ++head)
        for (int k = 0; k < 4; ++k) visit(s.nodes[order[head]].child[k]);
    const int32_t H = static_cast<int32_t>(order.size());
    if (H == 0) return;
    auto remap = [&](int32_t r) { return !interior_ref(r) ? r : (hot_of[r] >= 0 ? hot_of[r] : r + H); };
    std::vector<DevNode> moved;
    moved.reserve(out->nodes.size() + H);
    for (int32_t i = 0; i < H; ++i) moved.push_back(out->nodes[order[i]]);
    moved.insert(moved.end(), out->nodes.begin(), out->nodes.end());
    for (DevNode& nd : moved)
        for (int k = 0; k < 4; ++k) nd.child[k] = remap(nd.child[k]);
    out->nodes.swap(moved);
    for (DevInstance& di : out->instances)
        if (di.shape == 0u) di.root = remap(di.root);
    for (uint32_t mi = 0; mi < d.num_meshes; ++mi)
        if (d.meshes[mi].shape == GBL_SHAPE_MESH) out->mesh_root[mi] = remap(out->mesh_root[mi]);
    out->tlas_root = remap(out->tlas_root);
    out->tlas_base += H;
    out->hot_nodes = static_cast<uint32_t>(H);
}

}  // namespace

// One statement of what an image based light's tables take from the host besides its texels: pack_scene's and
// gbl_update_environment's (api_environment.hip)
void ibl_sin_theta(uint32_t dist_h, std::vector<float>* table) {
    table->resize(dist_h);
    for (uint32_t r = 0; r < dist_h; ++r) (*table)[r] = sinf((static_cast<float>(r) + 0.5f) / static_cast<float>(dist_h) * kPi);
}

float ibl_sphere_area(const float bound_lo[3], const float bound_hi[3]) {
    Aabb scene_bound;
    for (int k = 0; k < 3; ++k) scene_bound.lo[k] = bound_lo[k], scene_bound.hi[k] = bound_hi[k];
    const float radius = bounding_radius(scene_bound);
    return 4.0f * kPi * radius * radius;
}

// One statement of each light's packing: pack_scene's and gbl_update_lights'
float pack_light(const gbl_light& gl, const float bound_lo[3], const float bound_hi[3], float kept_power, DevLight* dl) {
    dl->type = gl.type;
    for (int k = 0; k < 3; ++k) dl->color[k] = gl.color[k], dl->pos[k] = gl.position[k];
    dl->cos_max = gl.cos_theta_max, dl->cos_falloff = gl.cos_falloff_start;
    Aabb scene_bound;
    for (int k = 0; k < 3; ++k) scene_bound.lo[k] = bound_lo[k], scene_bound.hi[k] = bound_hi[k];
    switch (gl.type) {
        case GBL_LIGHT_SPOT:
        case GBL_LIGHT_DIRECTIONAL: return pack_aimed_light(gl, scene_bound, dl);
        case GBL_LIGHT_AREA: return pack_area_light(gl, dl);
        case GBL_LIGHT_IBL: pack_ibl_rotation(gl, dl); return kept_power;
        default: return power_of(dl->color, 4.0f * kPi);   // GBL_LIGHT_POINT
    }
}

void pack_light_distribution(const std::vector<float>& power, std::vector<float>* cdf, std::vector<float>* pick_pdf) {
    const uint32_t n = static_cast<uint32_t>(power.size());
    cdf->assign(1, 0.0f);
    pick_pdf->assign(std::max<uint32_t>(1, n), 0.0f);
    if (n == 0) return;
    const float integral = cdf1d(power.data(), power.size(), cdf);
    const float dx = 1.0f / n;
    for (uint32_t i = 0; i < n; ++i) (*pick_pdf)[i] = (power[i] / integral) * dx;
}

void repack_lights(const gbl_light* edited, uint32_t first, uint32_t count, const float bound_lo[3], const float bound_hi[3], std::vector<DevLight>* lights,
                   std::vector<float>* power, std::vector<float>* cdf, std::vector<float>* pick_pdf) {
    for (uint32_t i = 0; i < count; ++i) (*power)[first + i] = pack_light(edited[i], bound_lo, bound_hi, (*power)[first + i], &(*lights)[first + i]);
    pack_light_distribution(*power, cdf, pick_pdf);
}

// Validate, then pack: every refusal comes from validate_desc, before any table is built; of the packers only the TLAS step
// returns a status (build_tlas keeps its check for gbl_update_instances) and after validation it cannot fail.
void repack_materials(const gbl_material* all, uint32_t num, uint32_t first, uint32_t count, std::vector<DevMaterial>* records, std::vector<uint32_t>* touched) {
    touched->clear();
    for (uint32_t i = 0; i < num; ++i) {
        const bool edited = i >= first && i - first < count;
        const bool wraps = all[i].type == GBL_MAT_MASK && static_cast<uint32_t>(all[i].masked_material) >= first && static_cast<uint32_t>(all[i].masked_material) - first < count;
        if (!edited && !wraps) continue;
        pack_material(all, i, &(*records)[i]);
        touched->push_back(i);
    }
}

void repack_textures(const gbl_texture* edited, uint32_t first, uint32_t count, std::vector<DevTexture>* records) {
    for (uint32_t i = 0; i < count; ++i) pack_texture(edited[i], &(*records)[first + i]);
}

gbl_status check_material_slots(const gbl_material* materials, uint32_t num_materials, const gbl_texture* textures, uint32_t num_textures, uint32_t first, uint32_t count,
                                std::string* err) {
    gbl_scene_desc d;
    memset(&d, 0, sizeof(d));
    d.materials = materials, d.num_materials = num_materials;
    d.textures = textures, d.num_textures = num_textures;
    for (uint32_t i = first; i < first + count; ++i) {
        const gbl_status st = validate_material_slots(d, i, err);
        if (st != GBL_OK) return st;
    }
    return GBL_OK;
}

gbl_status pack_scene(const gbl_scene_desc* desc, PackedScene* out, std::string* err, bool device_blas) {
    const gbl_status valid = validate_desc(desc, err);
    if (valid != GBL_OK) return valid;
    const gbl_scene_desc& d = *desc;
    out->extended = 0;   // the scene's part first; the camera's is added below
    pack_attributes(d, out);
    pack_tri_order_and_bounds(d, out);
    pack_meshes(d, device_blas, out);
    Aabb scene_bound;
    const gbl_status st = pack_instances(d, out, &scene_bound, err);
    if (st != GBL_OK) return st;
    pack_materials(d, out);
    pack_images(d, out);
    pack_textures(d, out);
    pack_lights(d, scene_bound, out);
    pack_volume(d, scene_bound, out);
    out->scene_extended = out->extended;
    if (camera_extended(d.camera)) out->extended = 1;
    pack_camera(d.camera, d.film, &out->camera);
    pack_film(d.film, out);
    out->hot_nodes = 0;
    if (!device_blas) hot_prefix(d, out);
    return GBL_OK;
}
