// What the host side of gbl_update_instances_device shares with its compose kernel (kernels/instances.h): why an edit is refused,
// in the order the refusals are tested.  The kernel folds (kind << 32 | instance index) into one 64-bit word by atomicMin, so the
// lowest kind and within it the lowest index win whatever the launch order; the word is all ones when nothing is refused.
#pragma once

#define GBL_INST_NOT_FINITE 0u      // a float of the transform is NaN or infinite
#define GBL_INST_SINGULAR 1u        // |det| < 1e-5 (scene_prep.cpp invert)
#define GBL_INST_BAD_MESH 2u        // the live record's mesh is out of range (cannot happen: the host wrote it)
#define GBL_INST_BOX_NOT_FINITE 3u  // GBL_INSTANCES_DEVICE_TLAS only: the world box overflowed a float
