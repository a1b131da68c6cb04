// The refit plan of one mesh's BLAS (gbl_update_vertices): its interior nodes in the order a bottom-up refit
// visits them.  Host only and free of HIP: tests/refit_dump.cpp builds it stand-alone with g++.
#pragma once
#include <string>
#include <vector>

#include "device_scene.h"
#include "kernels/refit_args.h"

struct RefitPlan {
    std::vector<RefitRecord> records;    // sorted by level, the root first
    std::vector<uint32_t> level_first;   // levels + 1 entries: level l is records[level_first[l] .. level_first[l + 1])
    uint32_t levels() const { return level_first.empty() ? 0u : static_cast<uint32_t>(level_first.size() - 1); }
};

// Walks `nodes` (num_nodes records, as the device holds them) from the child reference `root` BY REFERENCE: only nodes some
// reference leads to are visited, so the unreferenced originals of the hot prefix (scene_prep.cpp hot_prefix) never are.  Every
// node index must lie in [0, num_nodes), no node may be reached twice, every leaf's triangles must lie in [tri_first, tri_first +
// tri_count) -- the mesh's own range of `tris` -- and the walk may not be deeper than 64 levels; otherwise false with *err set
// and *out unspecified.  A root that is itself a leaf reference gives an empty plan.
bool build_refit_plan(const DevNode* nodes, uint64_t num_nodes, int32_t root, uint32_t tri_first, uint32_t tri_count, RefitPlan* out, std::string* err);
