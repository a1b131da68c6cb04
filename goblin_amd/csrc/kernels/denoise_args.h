// What the host side of gbl_film_denoise (api_film.hip) and its kernels (kernels/denoise.h) share: the level kernel's tile, the
// flag bits of a packed pixel and the arguments of one level.
#pragma once
#include <stdint.h>

#define GBL_DN_TILE_W 32
#define GBL_DN_TILE_H 8
#define GBL_DN_VALID 1u
#define GBL_DN_SURF 2u

struct DenoiseArgs {
    int W, H;
    int stride;
    float sigma_l;       // sigma_luminance
    float inv_sn2;       // 1 / (sigma_normal * sigma_normal), 0 without a normal film
    float inv_sa2;       // 1 / (sigma_albedo * sigma_albedo), 0 without an albedo film
    float sz;            // sigma_depth * stride, 0 without a depth film
    uint32_t has_var;    // a variance plane was given
    uint32_t demodulate;
};
