// libgoblin_hip.so, kernel unit: gbl_trace_rays' kernels (kernels/query.h).  The persistent form ships; -DGBL_QUERY_PLAIN builds
// the one-ray-per-lane form in its place for the measurement of DESIGN.md 4.11 (tools/query_bench.py).
#include "gbl_internal.h"
#include "kernels/query.h"

#ifdef GBL_QUERY_PLAIN
#define GBL_QUERY_KERNEL query_plain
#else
#define GBL_QUERY_KERNEL query_trace
#endif

bool gbl_query_plain(void) {
#ifdef GBL_QUERY_PLAIN
    return true;
#else
    return false;
#endif
}

gbl_query_kernel gbl_kernel_query(bool any, bool ext, bool ties, bool normal) {
    if (any) {
        if (normal) return nullptr;
        if (ext) return ties ? GBL_QUERY_KERNEL<true, true, true, false> : GBL_QUERY_KERNEL<true, true, false, false>;
        return ties ? GBL_QUERY_KERNEL<true, false, true, false> : GBL_QUERY_KERNEL<true, false, false, false>;
    }
    if (ext) {
        if (normal) return ties ? GBL_QUERY_KERNEL<false, true, true, true> : GBL_QUERY_KERNEL<false, true, false, true>;
        return ties ? GBL_QUERY_KERNEL<false, true, true, false> : GBL_QUERY_KERNEL<false, true, false, false>;
    }
    if (normal) return ties ? GBL_QUERY_KERNEL<false, false, true, true> : GBL_QUERY_KERNEL<false, false, false, true>;
    return ties ? GBL_QUERY_KERNEL<false, false, true, false> : GBL_QUERY_KERNEL<false, false, false, false>;
}
