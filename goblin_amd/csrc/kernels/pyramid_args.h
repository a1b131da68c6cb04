// What the image edits (api_images.hip, host only) and the pyramid kernel (kernels/pyramid.h) share: plain data.
#pragma once
#include <stdint.h>

// One level of a MIP pyramid made from the level above it: resizeImage (csrc/host/mipmap.cpp) of sw x sh texels of `channels`
// floats at `src` into dw x dh at `dst`.  The taps are the host's (csrc/host/mipmap_taps.h): destination column s reads source
// columns s_index[s] .. s_index[s] + n - 1, clamped to the level, with s_weight[s * n ..]; rows likewise with t_*.
struct PyramidArgs {
    const float* src;
    float* dst;
    const float* s_weight;   // dw * n
    const float* t_weight;   // dh * n
    const int32_t* s_index;  // dw
    const int32_t* t_index;  // dh
    int32_t sw, sh, dw, dh;
    int32_t n;               // taps per axis: 2 * the filter width, 4 between the levels of a power-of-two pyramid
    int32_t channels;        // 1, or 4 of which r, g, b are filtered and alpha is written as 1
};
