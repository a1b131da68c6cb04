// What the environment edits (api_environment.hip, host only) and their kernels (kernels/environment.h) share: plain data.
#pragma once
#include <stdint.h>

// An image based light's tables made again from its image's texels (scene_prep.cpp pack_ibl_distribution, attach_ibl_texels and
// pack_light_distribution).  `dist` is the light's block of DevScene::ibl_dist: the marginal block over the dh row integrals,
// then one block per row over its dw values, each block func[n], cdf[n + 1], integral.
struct EnvironmentArgs {
    const float* level;      // the pyramid level the distribution is taken from: dw x dh texels of 4 floats
    const float* top;        // the pyramid's last level: one texel
    const float* sin_theta;  // dh, the host's (scene_prep.h ibl_sin_theta)
    float* dist;
    float* power;            // the context's copy of the lights' powers, num_lights: entry `light` is replaced
    float* light_cdf;        // DevScene::light_cdf, num_lights + 1
    float* light_pick_pdf;   // DevScene::light_pick_pdf, num_lights
    uint32_t dw, dh;
    uint32_t light, num_lights;
    float sphere_area;       // 4 pi r^2 of the scene bound's sphere (scene_prep.h ibl_sphere_area)
};
