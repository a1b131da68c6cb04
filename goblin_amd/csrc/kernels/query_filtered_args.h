// Arguments of gbl_trace_rays_filtered's kernels (kernels/query_filtered.h): gbl_trace_rays' own, and beside them the filter and the
// transmittance output.
#pragma once
#include "query_args.h"

// The twelve query_trace kernels keep QueryArgs as it is; what the filtered family adds travels beside it.
struct FilteredQueryArgs {
    QueryArgs q;
    float4* transmittance;   // GBL_QUERY_TRANSMITTANCE: gbl_ray_transmittance, one 16-byte store per ray
    int filter;              // GBL_FILTER_* (device_scene.h) of a closest-hit or any-hit query
};
