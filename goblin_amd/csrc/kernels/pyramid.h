// The MIP pyramid of an edited image, level by level (gbl_update_image*, api_images.hip): resizeImage<T> (GoblinTexture.cpp:531-597)
// as csrc/host/mipmap.cpp restates it, one destination texel per thread.
//
// The texels must equal the host builder's bit for bit, so the sum keeps its order and its operations: for i over the row taps,
// then j over the column taps, w = t_weight * s_weight (one multiply), d[c] = d[c] + w * p[c] (a multiply, then an add: the
// unit is built with -ffp-contract=off) from 0.0f.  The weights come from the host, which made them with the loader's expf.
// T = Color accumulates r, g, b only (Color::operator+= leaves alpha alone) into Color(0.0f), whose alpha is 1.
//
// A 4-channel pyramid may start at a float offset that is no multiple of four (device_scene.h): texels are read and written
// float by float.  Consecutive lanes take consecutive texels of a row, so a wave's loads and stores still cover whole lines.
#pragma once
#include "../device_scene.h"
#include "pyramid_args.h"

__global__ __launch_bounds__(GBL_BLOCK) void pyramid_level(PyramidArgs a) {
    const uint32_t k = blockIdx.x * GBL_BLOCK + threadIdx.x;
    if (k >= static_cast<uint32_t>(a.dw) * static_cast<uint32_t>(a.dh)) return;
    const int t = static_cast<int>(k / static_cast<uint32_t>(a.dw)), s = static_cast<int>(k - static_cast<uint32_t>(t) * static_cast<uint32_t>(a.dw));
    const int t0 = a.t_index[t], s0 = a.s_index[s];
    const float* tw = a.t_weight + static_cast<size_t>(t) * a.n;
    const float* sw = a.s_weight + static_cast<size_t>(s) * a.n;
    float* d = a.dst + static_cast<size_t>(k) * a.channels;
    if (a.channels == 4) {
        float r = 0.0f, g = 0.0f, b = 0.0f;
        for (int i = 0; i < a.n; ++i) {
            const int src_t = min(max(t0 + i, 0), a.sh - 1);
            for (int j = 0; j < a.n; ++j) {
                const int src_s = min(max(s0 + j, 0), a.sw - 1);
                const float w = tw[i] * sw[j];
                const float* p = a.src + (static_cast<size_t>(src_t) * a.sw + src_s) * 4;
                r = r + w * p[0];
                g = g + w * p[1];
                b = b + w * p[2];
            }
        }
        d[0] = r, d[1] = g, d[2] = b, d[3] = 1.0f;
    } else {
        float v = 0.0f;
        for (int i = 0; i < a.n; ++i) {
            const int src_t = min(max(t0 + i, 0), a.sh - 1);
            for (int j = 0; j < a.n; ++j) {
                const int src_s = min(max(s0 + j, 0), a.sw - 1);
                const float w = tw[i] * sw[j];
                v = v + w * a.src[static_cast<size_t>(src_t) * a.sw + src_s];
            }
        }
        d[0] = v;
    }
}
