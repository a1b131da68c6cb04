// The refit plan of one mesh's BLAS: see scene_refit.h.
#include "scene_refit.h"

namespace {

// A leaf reference's triangles lie inside the mesh's range of `tris`
bool leaf_inside(int32_t ref, uint32_t tri_first, uint32_t tri_count) {
    const uint32_t bits = ~static_cast<uint32_t>(ref);
    const uint64_t first = bits >> 2, count = (bits & 3u) + 1u;
    return first >= tri_first && first + count <= static_cast<uint64_t>(tri_first) + tri_count;
}

}   // namespace

bool build_refit_plan(const DevNode* nodes, uint64_t num_nodes, int32_t root, uint32_t tri_first, uint32_t tri_count, RefitPlan* out, std::string* err) {
    const int kMaxLevels = 64;
    out->records.clear();
    out->level_first.clear();
    if (root == static_cast<int32_t>(GBL_REF_NONE)) {
        *err = "refit plan: the mesh has no root";
        return false;
    }
    if (root < 0) {   // the whole mesh is one leaf
        if (!leaf_inside(root, tri_first, tri_count)) {
            *err = "refit plan: the root leaf's triangles lie outside the mesh's range";
            return false;
        }
        return true;
    }
    if (static_cast<uint64_t>(root) >= num_nodes) {
        *err = "refit plan: the root lies outside the node array";
        return false;
    }
    std::vector<bool> seen(num_nodes, false);
    seen[static_cast<size_t>(root)] = true;
    out->records.push_back(RefitRecord{root, 0, {-1, -1, -1, -1}});
    out->level_first.push_back(0);
    // breadth first: the children of level l's records are appended behind them, which sorts the records by level
    for (uint32_t begin = 0, level = 0; begin < out->records.size(); ++level) {
        if (level >= static_cast<uint32_t>(kMaxLevels)) {
            *err = "refit plan: the tree is deeper than 64 levels";
            return false;
        }
        const uint32_t end = static_cast<uint32_t>(out->records.size());
        for (uint32_t r = begin; r < end; ++r) {
            const DevNode& nd = nodes[out->records[r].node];
            for (int c = 0; c < 4; ++c) {
                const int32_t ref = nd.child[c];
                if (ref == static_cast<int32_t>(GBL_REF_NONE)) continue;
                if (ref < 0) {
                    if (!leaf_inside(ref, tri_first, tri_count)) {
                        *err = "refit plan: node " + std::to_string(out->records[r].node) + " has a leaf outside the mesh's range of triangles";
                        return false;
                    }
                    continue;
                }
                if (static_cast<uint64_t>(ref) >= num_nodes) {
                    *err = "refit plan: node " + std::to_string(out->records[r].node) + " refers to a node outside the node array";
                    return false;
                }
                if (seen[static_cast<size_t>(ref)]) {
                    *err = "refit plan: node " + std::to_string(ref) + " is reached twice";
                    return false;
                }
                seen[static_cast<size_t>(ref)] = true;
                out->records[r].child_plan[c] = static_cast<int32_t>(out->records.size());
                out->records.push_back(RefitRecord{ref, static_cast<int32_t>(level) + 1, {-1, -1, -1, -1}});
            }
        }
        out->level_first.push_back(end);
        begin = end;
    }
    // (the loop's last pass appended nothing: level_first's last entry is records.size())
    return true;
}
