// What the refit plan builder (scene_refit.cpp, host only) and the refit kernels (kernels/refit.h) share: plain data.
#pragma once
#include <stdint.h>

// One interior node of a mesh's BLAS, found by walking the child references from the mesh's root.  The records of a plan are
// sorted by level (the root's is 0), so record r's interior children sit behind it: child_plan[c] is the record of the interior
// child in slot c, -1 for a leaf and for an unused slot.
struct RefitRecord {
    int32_t node;            // index into DevScene::nodes
    int32_t level;
    int32_t child_plan[4];
};

// The exact (unquantised, un-nudged) box of a plan record's node: the union of the triangle bounds beneath it
struct RefitBox {
    float lo[3], hi[3];
};
