// Device-pointer instance edits (gbl_update_instances_device): what gbl_update_instances does to the caller's
// transforms with loops on the host, done where the floats are, and a TLAS built over the instance boxes by the device builder.
//
//   inst_compose_kernel       per edited instance: m / inv and the world box, in scene_prep.cpp's float association, into STAGING
//                             records; a refusal goes into one 64-bit word by atomicMin over (kind, instance index)
//   inst_scene_bound_kernel   the bound of the instance boxes' centres, as order keys reduced by 32-bit atomic minima / maxima
//   inst_keys_kernel          30-bit Morton code of a box centre inside that bound, key = code << 32 | instance index
//   inst_collapse_kernel      lbvh_collapse's sibling: a leaf is ONE instance, referred to by its own index (the instance table is
//                             not permuted), node k is index tlas_base + k
//
// The arithmetic is in host + device inline functions (the first half of this header needs no HIP: tests/test_instances_device_cpu.py
// compiles it with g++ beside scene_prep.cpp and compares bits).  The kernels, and lbvh.h which they build on, follow under
// __HIPCC__.  Every index is bounded by a count the host passes in; the one index read from device data (an instance's mesh) is
// checked against the mesh count before it is used.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>
#ifdef __HIPCC__
#define GBL_INST_HD __host__ __device__ __forceinline__
#else
#define GBL_INST_HD inline
#endif

#include "instances_args.h"

struct InstMat {
    float v[4][4];
};

GBL_INST_HD uint32_t inst_float_bits(float f) {
    uint32_t u;
    memcpy(&u, &f, sizeof(u));
    return u;
}
// Not finite by the bits (the exponent field is all ones), whatever the compiler assumes about floats
GBL_INST_HD bool inst_not_finite(float f) { return (inst_float_bits(f) & 0x7F800000u) == 0x7F800000u; }

GBL_INST_HD void inst_identity(InstMat* r) {
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) r->v[i][j] = i == j ? 1.0f : 0.0f;
}

// scene_prep.cpp multiply: the zero terms are added as well (they round nothing, but they keep the sign of a zero)
GBL_INST_HD void inst_multiply(const InstMat& a, const InstMat& b, InstMat* r) {
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            float acc = a.v[i][0] * b.v[0][j];
            acc = acc + a.v[i][1] * b.v[1][j];
            acc = acc + a.v[i][2] * b.v[2][j];
            acc = acc + a.v[i][3] * b.v[3][j];
            r->v[i][j] = acc;
        }
}

// scene_prep.cpp rotation_of: q = w x y z, not normalised
GBL_INST_HD void inst_rotation_of(const float q[4], InstMat* r) {
    const float w = q[0], x = q[1], y = q[2], z = q[3];
    const float tx = 2.0f * x, ty = 2.0f * y, tz = 2.0f * z;
    const float xx = tx * x, xy = tx * y, xz = tx * z, xw = tx * w;
    const float yy = ty * y, yz = ty * z, yw = ty * w;
    const float zz = tz * z, zw = tz * w;
    inst_identity(r);
    r->v[0][0] = 1 - yy - zz; r->v[0][1] = xy - zw;     r->v[0][2] = xz + yw;
    r->v[1][0] = xy + zw;     r->v[1][1] = 1 - xx - zz; r->v[1][2] = yz - xw;
    r->v[2][0] = xz - yw;     r->v[2][1] = yz + xw;     r->v[2][2] = 1 - xx - yy;
}

GBL_INST_HD float inst_minor2(const InstMat& m, int r0, int r1, int c0, int c1) { return m.v[r0][c0] * m.v[r1][c1] - m.v[r0][c1] * m.v[r1][c0]; }

// One cofactor row of scene_prep.cpp invert (its `cof` lambda)
GBL_INST_HD void inst_cof(const InstMat& m, int row, const float s[6], float r[4]) {
    r[0] = m.v[row][1] * s[0] - m.v[row][2] * s[1] + m.v[row][3] * s[2];
    r[1] = m.v[row][0] * s[0] - m.v[row][2] * s[3] + m.v[row][3] * s[4];
    r[2] = m.v[row][0] * s[1] - m.v[row][1] * s[3] + m.v[row][3] * s[5];
    r[3] = m.v[row][0] * s[2] - m.v[row][1] * s[4] + m.v[row][2] * s[5];
}

// 1 / det rounded as IEEE division rounds it, on either side
GBL_INST_HD float inst_reciprocal(float det) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(1.0f, det);
#else
    return 1.0f / det;
#endif
}

// scene_prep.cpp invert: false when |det| < 1e-5, *out then holds its first column only
GBL_INST_HD bool inst_invert(const InstMat& m, InstMat* out) {
    const int cols[6][2] = {{2, 3}, {1, 3}, {1, 2}, {0, 3}, {0, 2}, {0, 1}};
    float a[6], b[6], c[6];   // minors of row pairs (2,3), (1,3), (1,2)
    for (int k = 0; k < 6; ++k) {
        a[k] = inst_minor2(m, 2, 3, cols[k][0], cols[k][1]);
        b[k] = inst_minor2(m, 1, 3, cols[k][0], cols[k][1]);
        c[k] = inst_minor2(m, 1, 2, cols[k][0], cols[k][1]);
    }
    float k0[4], k1[4], k2[4], k3[4];
    inst_cof(m, 1, a, k0);
    inst_cof(m, 0, a, k1);
    inst_cof(m, 0, b, k2);
    inst_cof(m, 0, c, k3);
    InstMat& o = *out;
    for (int i = 0; i < 4; ++i) o.v[i][0] = (i & 1) == 0 ? k0[i] : -k0[i];
    const float det = m.v[0][0] * o.v[0][0] + m.v[0][1] * o.v[1][0] + m.v[0][2] * o.v[2][0] + m.v[0][3] * o.v[3][0];
    if (fabsf(det) < 1e-5f) return false;
    const float inv_det = inst_reciprocal(det);
    for (int i = 0; i < 4; ++i) {
        o.v[i][1] = (i & 1) == 0 ? -k1[i] : k1[i];
        o.v[i][2] = (i & 1) == 0 ? k2[i] : -k2[i];
        o.v[i][3] = (i & 1) == 0 ? -k3[i] : k3[i];
    }
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) o.v[i][j] *= inv_det;
    return true;
}

// scene_prep.cpp compose + store3x4 over one gbl_trs (t = position, orientation wxyz, scale): the 3x4 rows of toWorld and of
// its inverse.  false when the reference cannot invert it; inv is then not for use.
GBL_INST_HD bool inst_compose(const float t[10], float m[12], float inv[12]) {
    InstMat S, R, M, I;
    inst_identity(&S);
    S.v[0][0] = t[7]; S.v[1][1] = t[8]; S.v[2][2] = t[9];
    inst_rotation_of(t + 3, &R);
    inst_multiply(R, S, &M);
    M.v[0][3] = t[0]; M.v[1][3] = t[1]; M.v[2][3] = t[2];
    inst_identity(&I);
    const bool ok = inst_invert(M, &I);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j) {
            m[4 * i + j] = M.v[i][j];
            inv[4 * i + j] = I.v[i][j];
        }
    return ok;
}

GBL_INST_HD bool inst_trs_not_finite(const float t[10]) {
    bool bad = false;
    for (int k = 0; k < 10; ++k) bad = bad || inst_not_finite(t[k]);
    return bad;
}

// build_tlas's world box (Transform::onBBox): the eight corners of the mesh bound through m, folded by std::min / std::max in
// corner order from the empty box
GBL_INST_HD void inst_world_box(const float m[12], const float mesh_lo[3], const float mesh_hi[3], float lo[3], float hi[3]) {
    for (int k = 0; k < 3; ++k) {
        lo[k] = INFINITY;
        hi[k] = -INFINITY;
    }
    for (int c = 0; c < 8; ++c) {
        const float corner[3] = {(c & 1) ? mesh_hi[0] : mesh_lo[0], (c & 2) ? mesh_hi[1] : mesh_lo[1], (c & 4) ? mesh_hi[2] : mesh_lo[2]};
        for (int i = 0; i < 3; ++i) {
            const float w = m[4 * i + 0] * corner[0] + m[4 * i + 1] * corner[1] + m[4 * i + 2] * corner[2] + m[4 * i + 3];
            lo[i] = w < lo[i] ? w : lo[i];   // std::min(lo, w)
            hi[i] = hi[i] < w ? w : hi[i];   // std::max(hi, w)
        }
    }
}

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include "../device_scene.h"
#include "lbvh.h"

#define GBL_INSTANCES_BLOCK 256

// One lane per edited instance.  trs: the caller's records (10 floats each); live: the context's instance table (every field
// but m / inv is kept); mesh_bounds: lo then hi, 6 floats per mesh.  The host has checked first + count <= the table's length.
// Writes staging record i (not the live tables), or folds a refusal into *refusal (all ones before the launch).
__global__ void inst_compose_kernel(const float* trs, uint32_t first, uint32_t count, const DevInstance* live, const float* mesh_bounds, uint32_t num_meshes,
                                    uint32_t refuse_box, DevInstance* out_inst, DevInstanceBound* out_bound, unsigned long long* refusal) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint32_t index = first + i;
    float t[10];
    for (int k = 0; k < 10; ++k) t[k] = trs[10 * static_cast<size_t>(i) + k];
    DevInstance di = live[index];
    DevInstanceBound db;
    uint32_t kind = 0xFFFFFFFFu;
    if (inst_trs_not_finite(t)) {
        kind = GBL_INST_NOT_FINITE;
    } else if (!inst_compose(t, di.m, di.inv)) {
        kind = GBL_INST_SINGULAR;
    } else if (di.mesh < 0 || static_cast<uint32_t>(di.mesh) >= num_meshes) {
        kind = GBL_INST_BAD_MESH;
    } else {
        const float* b = mesh_bounds + 6 * static_cast<size_t>(di.mesh);
        inst_world_box(di.m, b, b + 3, db.lo, db.hi);
        bool box_bad = false;
        for (int k = 0; k < 3; ++k) box_bad = box_bad || inst_not_finite(db.lo[k]) || inst_not_finite(db.hi[k]);
        if (refuse_box != 0u && box_bad) kind = GBL_INST_BOX_NOT_FINITE;
    }
    if (kind != 0xFFFFFFFFu) {
        atomicMin(refusal, (static_cast<unsigned long long>(kind) << 32) | index);   // the lowest kind, then the lowest index, whatever the launch order
        return;
    }
    out_inst[i] = di;
    out_bound[i] = db;
}

// A float as an unsigned key that orders like the float compares (kernels/vertices.h has the same map), and back
__device__ __forceinline__ uint32_t inst_order_key(float v) {
    uint32_t b = __float_as_uint(v);
    if (b == 0x80000000u) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float inst_key_value(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

// The bound the Morton codes are scaled by: of the box CENTRES, not of the boxes.  One instance far larger than the rest (a
// floor under ten thousand props) would stretch the bound of the boxes until every other centre fell into a handful of the
// 1024 cells per axis, and the tree over equal codes is a tree over instance indices: measured, a grid of 10^4 instances on a
// floor 200 times its size then traced 9 times slower than the host's tree, 10^5 of them 20 times.
// keys[0..2]: the lowest centre per axis (all ones before the launch); keys[3..5]: the highest (zero before it).  Minima and
// maxima do not depend on the order they are folded in: two builds over the same boxes see the same bound.
__global__ void inst_scene_bound_kernel(const DevInstanceBound* bounds, uint32_t n, uint32_t* keys) {
    uint32_t lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const DevInstanceBound b = bounds[i];
        for (int a = 0; a < 3; ++a) {
            const uint32_t c = inst_order_key(0.5f * (b.lo[a] + b.hi[a]));   // (inst_keys_kernel forms the same float)
            lo[a] = min(lo[a], c);
            hi[a] = max(hi[a], c);
        }
        if (i + stride < i) break;
    }
    for (int a = 0; a < 3; ++a)
        for (int off = 32; off > 0; off >>= 1) {
            lo[a] = min(lo[a], static_cast<uint32_t>(__shfl_xor(static_cast<int>(lo[a]), off)));
            hi[a] = max(hi[a], static_cast<uint32_t>(__shfl_xor(static_cast<int>(hi[a]), off)));
        }
    if ((threadIdx.x & 63u) == 0u)
        for (int a = 0; a < 3; ++a) {
            atomicMin(keys + a, lo[a]);
            atomicMax(keys + 3 + a, hi[a]);
        }
}

// lbvh_keys for instances: the box centre inside the bound of the centres; the index makes every key unique and orders identical centres
__global__ void inst_keys_kernel(const DevInstanceBound* bounds, uint32_t n, const uint32_t* bound_keys, unsigned long long* keys) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const DevInstanceBound b = bounds[i];
    uint32_t q[3];
    for (int a = 0; a < 3; ++a) {
        const float slo = inst_key_value(bound_keys[a]), shi = inst_key_value(bound_keys[3 + a]);
        const float ext = shi - slo;
        const float c = 0.5f * (b.lo[a] + b.hi[a]);
        const float u = ext > 0.0f ? (c - slo) / ext : 0.0f;
        q[a] = static_cast<uint32_t>(fminf(fmaxf(u * 1024.0f, 0.0f), 1023.0f));   // (fmaxf drops a NaN)
    }
    const uint32_t code = (lbvh_expand_bits(q[0]) << 2) | (lbvh_expand_bits(q[1]) << 1) | lbvh_expand_bits(q[2]);
    keys[i] = (static_cast<unsigned long long>(code) << 32) | i;
}

// lbvh_collapse over instances.  t.leaf_box holds the instance boxes in sorted order, keys the sorted keys (their low words
// are the instance indices, each below n by inst_keys_kernel's construction and checked again here).  A 4-wide node takes the
// slot its parent reserved; a slot at or beyond `capacity` is counted but not written, and the host refuses the tree.
__global__ void inst_collapse_kernel(LbvhTree t, const unsigned long long* keys, uint32_t n, const LbvhFrontier* in, uint32_t n_in, LbvhFrontier* out, uint32_t* n_out,
                                     uint32_t* n_nodes, DevNode* nodes, uint32_t capacity, int32_t tlas_base) {
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_in) return;
    const LbvhFrontier f = in[w];
    int kids[4] = {t.left[f.node], t.right[f.node], 0, 0};
    int nk = 2;
    while (nk < 4) {   // open the interior child with the largest surface area (scene_prep.cpp Flat4::emit)
        int best = -1;
        float best_area = -1.0f;
        for (int i = 0; i < nk; ++i) {
            if (kids[i] < 0) continue;
            const LbvhBox b = t.box[kids[i]];
            const float dx = b.hi[0] - b.lo[0], dy = b.hi[1] - b.lo[1], dz = b.hi[2] - b.lo[2];
            const float area = dx * dy + dy * dz + dz * dx;
            if (area > best_area) {
                best_area = area;
                best = i;
            }
        }
        if (best < 0) break;
        const int c = kids[best];
        kids[best] = t.left[c];
        kids[nk++] = t.right[c];
    }
    DevNode nd;
    LbvhBox kb[4];
    for (int i = 0; i < 4; ++i) {
        nd.child[i] = static_cast<int32_t>(GBL_REF_NONE);
        if (i >= nk) continue;
        kb[i] = lbvh_node_box(t, kids[i]);
        if (kids[i] < 0) {
            const uint32_t sorted = static_cast<uint32_t>(~kids[i]);
            const uint32_t inst = sorted < n ? static_cast<uint32_t>(keys[sorted] & 0xffffffffull) : 0u;
            nd.child[i] = ~static_cast<int32_t>((inst < n ? inst : 0u) << 2);
        } else {
            const uint32_t slot = atomicAdd(n_nodes, 1u);
            nd.child[i] = tlas_base + static_cast<int32_t>(slot);
            const uint32_t q = atomicAdd(n_out, 1u);
            if (q + 1u < n) {   // (a binary tree over n leaves has n - 1 interior nodes: the frontier arrays hold that many)
                out[q].node = kids[i];
                out[q].slot = static_cast<int32_t>(slot);
            }
        }
    }
    for (int a = 0; a < 3; ++a) {
        float lo = INFINITY, hi = -INFINITY;
        for (int i = 0; i < nk; ++i) {
            lo = fminf(lo, lbvh_nudge_down(kb[i].lo[a]));
            hi = fmaxf(hi, lbvh_nudge_up(kb[i].hi[a]));
        }
        nd.o[a] = lo;
        // grid step 2^e with 255 * 2^e >= extent (same rule as the host packer and lbvh_collapse)
        const float extent = (hi - lo) * 1.0001f + 1e-30f;
        int e = 0;
        frexpf(extent / 255.0f, &e);
        const int biased = min(254, max(1, e + 127));
        const float step = ldexpf(1.0f, biased - 127);
        nd.scale[a] = step;
        uint32_t ql = 0, qh = 0;
        for (int i = 0; i < 4; ++i) {
            uint32_t l = 255, h = 0;
            if (i < nk) {
                const float cl = lbvh_nudge_down(kb[i].lo[a]), ch = lbvh_nudge_up(kb[i].hi[a]);
                // (clamped before the corrections: each of them ends within 255 steps whatever the boxes hold)
                double fl = fmin(255.0, fmax(0.0, floor((static_cast<double>(cl) - lo) / step)));
                double fh = fmin(255.0, fmax(0.0, ceil((static_cast<double>(ch) - lo) / step)));
                while (fl > 0 && lo + static_cast<float>(fl) * step > cl) fl -= 1;
                while (fh < 255 && lo + static_cast<float>(fh) * step < ch) fh += 1;
                l = static_cast<uint32_t>(fl);
                h = static_cast<uint32_t>(fh);
            }
            ql |= l << (8 * i);
            qh |= h << (8 * i);
        }
        nd.qlo[a] = ql;
        nd.qhi[a] = qh;
    }
    if (static_cast<uint32_t>(f.slot) < capacity) nodes[f.slot] = nd;
}
#endif   // __HIPCC__
