// Vertex edits (gbl_update_vertices): a mesh's BLAS refitted in place over edited positions.  The tree's shape,
// the leaves' contents and every child reference stay; what is derived from positions is computed again by the builders' own
// rules (scene_prep.cpp build_host_blas / Flat4::emit, kernels/lbvh.h lbvh_tris / lbvh_collapse), so a refit over unchanged
// positions rewrites every byte with the value it had.
//
//   refit_tris    per DevTri of the mesh: p0, e1, e2 and the triangle's bound from the edited positions
//   refit_level   per interior node of one level (the plan of scene_refit.h), deepest level first: the children's exact
//                 boxes -- a leaf's from the triangle bounds, an interior child's from the launch before -- quantised again
//
// One launch per level and no counters: a level's launch follows the deeper one's in the stream, which is all the ordering the
// scheme needs.
#pragma once
#include <hip/hip_runtime.h>

#include "../device_scene.h"
#include "refit_args.h"

// std::min / std::max as the host packer applies them to a triangle's vertices (they keep the first of two equal values, which
// tells +0 from -0; fminf / fmaxf need not)
__device__ __forceinline__ float refit_min(float a, float b) { return b < a ? b : a; }
__device__ __forceinline__ float refit_max(float a, float b) { return a < b ? b : a; }

__global__ void refit_tris(DevTri* tris, DevTriBound* bounds, const DevTriShade* tri_shade, const float* pos, uint32_t num_vertices, uint32_t first,
                           uint32_t count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const size_t k = static_cast<size_t>(first) + i;
    const DevTriShade s = tri_shade[tris[k].shade];
    if (s.v[0] >= num_vertices || s.v[1] >= num_vertices || s.v[2] >= num_vertices) return;
    const float* p0 = pos + 3 * static_cast<size_t>(s.v[0]);
    const float* p1 = pos + 3 * static_cast<size_t>(s.v[1]);
    const float* p2 = pos + 3 * static_cast<size_t>(s.v[2]);
    for (int a = 0; a < 3; ++a) {
        const float x0 = p0[a], x1 = p1[a], x2 = p2[a];
        tris[k].p0[a] = x0;
        tris[k].e1[a] = x1 - x0;
        tris[k].e2[a] = x2 - x0;
        bounds[k].lo[a] = refit_min(refit_min(x0, x1), x2);
        bounds[k].hi[a] = refit_max(refit_max(x0, x1), x2);
    }
}

__device__ __forceinline__ float refit_nudge_down(float v) { return v - fabsf(v) * 4e-7f - 1e-30f; }
__device__ __forceinline__ float refit_nudge_up(float v) { return v + fabsf(v) * 4e-7f + 1e-30f; }

// Records [begin, end) of `plan` are one level.  node_box is indexed like the plan.
__global__ void refit_level(DevNode* nodes, const DevTriBound* bounds, const RefitRecord* plan, RefitBox* node_box, uint32_t begin, uint32_t end) {
    const uint32_t r = begin + blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= end) return;
    const RefitRecord rec = plan[r];
    DevNode* nd = nodes + rec.node;
    RefitBox kb[4];
    bool used[4];
    RefitBox self;
    for (int a = 0; a < 3; ++a) {
        self.lo[a] = INFINITY;
        self.hi[a] = -INFINITY;
    }
    for (int c = 0; c < 4; ++c) {
        const int32_t ref = nd->child[c];
        used[c] = ref != static_cast<int32_t>(GBL_REF_NONE);
        for (int a = 0; a < 3; ++a) {
            kb[c].lo[a] = INFINITY;
            kb[c].hi[a] = -INFINITY;
        }
        if (!used[c]) continue;
        if (ref < 0) {
            const uint32_t bits = ~static_cast<uint32_t>(ref);
            const uint32_t first = bits >> 2, count = (bits & 3u) + 1u;
            for (uint32_t t = 0; t < count; ++t) {
                const DevTriBound b = bounds[first + t];
                for (int a = 0; a < 3; ++a) {
                    kb[c].lo[a] = fminf(kb[c].lo[a], b.lo[a]);
                    kb[c].hi[a] = fmaxf(kb[c].hi[a], b.hi[a]);
                }
            }
        } else {
            kb[c] = node_box[rec.child_plan[c]];
        }
        for (int a = 0; a < 3; ++a) {
            self.lo[a] = fminf(self.lo[a], kb[c].lo[a]);
            self.hi[a] = fmaxf(self.hi[a], kb[c].hi[a]);
        }
    }
    node_box[r] = self;
    // the builders' quantiser (scene_prep.cpp Flat4::emit, kernels/lbvh.h lbvh_collapse)
    for (int a = 0; a < 3; ++a) {
        float lo = INFINITY, hi = -INFINITY;
        for (int c = 0; c < 4; ++c) {
            if (!used[c]) continue;
            lo = fminf(lo, refit_nudge_down(kb[c].lo[a]));
            hi = fmaxf(hi, refit_nudge_up(kb[c].hi[a]));
        }
        const float extent = (hi - lo) * 1.0001f + 1e-30f;
        int e = 0;
        frexpf(extent / 255.0f, &e);
        const int biased = min(254, max(1, e + 127));
        const float step = ldexpf(1.0f, biased - 127);
        uint32_t ql = 0, qh = 0;
        for (int c = 0; c < 4; ++c) {
            uint32_t l = 255, h = 0;
            if (used[c]) {
                const float cl = refit_nudge_down(kb[c].lo[a]), ch = refit_nudge_up(kb[c].hi[a]);
                double fl = floor((static_cast<double>(cl) - lo) / step);
                double fh = ceil((static_cast<double>(ch) - lo) / step);
                while (fl > 0 && lo + static_cast<float>(fl) * step > cl) fl -= 1;
                while (fh < 255 && lo + static_cast<float>(fh) * step < ch) fh += 1;
                l = static_cast<uint32_t>(fmin(255.0, fmax(0.0, fl)));
                h = static_cast<uint32_t>(fmin(255.0, fmax(0.0, fh)));
            }
            ql |= l << (8 * c);
            qh |= h << (8 * c);
        }
        nd->o[a] = lo;
        nd->scale[a] = step;
        nd->qlo[a] = ql;
        nd->qhi[a] = qh;
    }
}
