// libgoblin_hip.so, kernel unit: gbl_radiance_rays' kernels (kernels/radiance.h), picked as kernels_path.hip picks the megakernel's:
// lean native, lean native with the tie rule, lean replay, EXT native, EXT replay.  Replay and EXT builds follow the tie rule always.
#include "gbl_internal.h"
#include "kernels/radiance.h"

gbl_radiance_kernel gbl_kernel_radiance(bool replay, bool ext, bool exact_ties) {
    if (replay) return ext ? radiance_trace<true, true, true> : radiance_trace<true, false, true>;
    if (ext) return radiance_trace<false, true, true>;
    return exact_ties ? radiance_trace<false, false, true> : radiance_trace<false, false, false>;
}
