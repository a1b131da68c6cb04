// What the host side of gbl_film_accumulate (api_film.hip) and its kernels (kernels/temporal.h) share: the accumulate kernel's
// tile, the flag bits of a prepared pixel and the arguments of the call.
#pragma once
#include <stdint.h>

#include "../device_scene.h"

#define GBL_TP_TILE_W 32
#define GBL_TP_TILE_H 8
#define GBL_TP_HALO 2       // the spatial variance estimate's 5 x 5 neighbourhood
#define GBL_TP_VALID 1u
#define GBL_TP_SURF 2u

struct TemporalArgs {
    int W, H;
    DevCamera cur, prev;     // the context's camera and params->prev_camera, both packed by pack_camera with the context's film
    float alpha_min, max_history, sigma_depth, cos_normal;
    uint32_t has_normal;     // a normal film was given: the history taps are tested against cos_normal
    uint32_t has_history;    // history_in was given
};
