// Argument block of the first-hit feature kernels (kernels/aov.h).  A header of its own so the host side can hold one without
// pulling the kernels in.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../../include/goblin_hip.h"

// What the kernel writes for one chunk of the call's samples (samples pass_k0 .. pass_k0 + pass_spp of every pixel).  The three
// planes are what wf_splat filters into the three films: float4 per sample, indexed pixel * pass_spp + kk like WfArgs::li_buf.
// `samples` is the caller's record array, indexed like li_out (pixel * spp + k).  Any of the four may be null.
struct AovArgs {
    float4* albedo;      // {albedo.rgb, -}
    float4* normal;      // {n.xyz, -}
    float4* depth;       // {t * hit, hit, 0, -}
    gbl_aov_sample* samples;
    int32_t pass_k0, pass_spp;
};
