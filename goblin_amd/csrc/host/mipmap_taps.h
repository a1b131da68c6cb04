// resizeImage's tap step (GoblinTexture.cpp:531-565), shared by the host's pyramid builder (mipmap.cpp) and the image edits of
// libgoblin_hip.so (api_images.hip): the filter width of a resize, and per destination column or row the first source index and
// the 2 * width normalised gaussian weights.  They depend on the two sizes only, never on the texels.  Same float operations in
// the same order as the reference's, so the weights equal its bits.
#pragma once
#include <algorithm>
#include <cmath>

namespace gbl_host_detail {

inline int floor_int(float f) { return static_cast<int>(floorf(f)); }
inline float gaussian(float x, float w, float falloff = 2.0f) { return std::max(0.0f, expf(-falloff * x * x) - expf(-falloff * w * w)); }

// The filter width of a sw x sh -> dw x dh resize; every destination texel sums n = 2 * floor_int(width) taps per axis
inline float resize_filter_width(int sw, int sh, int dw, int dh) {
    return floorf(std::max(2.0f, std::max(static_cast<float>(sw) / static_cast<float>(dw), static_cast<float>(sh) / static_cast<float>(dh))));
}

// One axis: destination s of `count` reads sources index[s] .. index[s] + n - 1 (the caller clamps them to [0, src_size)) with
// weight[s * n ..], which sum to 1 up to rounding
inline void resize_taps(int count, int src_size, float filter_width, int n, float* weight, int* index) {
    for (int s = 0; s < count; ++s) {
        const float center = (static_cast<float>(s) + 0.5f) / count * src_size;
        index[s] = floor_int(center - filter_width + 0.5f);
        float sum = 0.0f;
        const int off = s * n;
        for (int i = 0; i < n; ++i) {
            const float p = index[s] + 0.5f + i;
            weight[off + i] = gaussian(p - center, filter_width);
            sum += weight[off + i];
        }
        const float inv = 1.0f / sum;
        for (int i = 0; i < n; ++i) weight[off + i] *= inv;
    }
}

}  // namespace gbl_host_detail
