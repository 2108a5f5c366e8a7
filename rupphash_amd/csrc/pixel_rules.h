// pixel_rules.h -- from a decoded image's native pixel to what is hashed, shared by the PNG and TIFF paths (host decoders and device
// kernels): the rules of include/rupphash.h, "What is hashed".  v[0 .. out_ch) are the native samples of one pixel in out_depth bits.
#pragma once
#include <stdint.h>

#include "inflate.h"

namespace rphx {

// channels of the 8-bit hasher pixels for a native layout: 1 Luma8, 3 Rgb8, 4 Rgba8 (LumaA8 travels as Rgba8; 16-bit images as Rgb8)
RPHZ_HD uint8_t hasher_channels(uint32_t out_ch, uint32_t out_depth) { return (uint8_t)(out_depth == 16 ? 3 : out_ch == 1 ? 1 : out_ch == 3 ? 3 : 4); }

// The 8-bit pixels the hasher takes: Luma8 as it is; LumaA8 as Rgba8 (l, l, l, a); Rgb8 / Rgba8 as they are; 16-bit images as to_rgb8
// gives them, each sample v -> round(v / 257) = (v + 128) / 257 (no ties: 257 is odd) -- UNPINNED against the crate
RPHZ_HD void hasher_pixel(uint32_t out_ch, uint32_t out_depth, const uint32_t v[4], uint8_t o[4])
{
    if (out_depth == 16) {
        const uint32_t g = (v[0] + 128) / 257;
        if (out_ch <= 2) {
            o[0] = o[1] = o[2] = (uint8_t)g;
        } else {
            o[0] = (uint8_t)g;
            o[1] = (uint8_t)((v[1] + 128) / 257);
            o[2] = (uint8_t)((v[2] + 128) / 257);
        }
        return;
    }
    switch (out_ch) {
    case 1: o[0] = (uint8_t)v[0]; break;
    case 2: o[0] = o[1] = o[2] = (uint8_t)v[0]; o[3] = (uint8_t)v[1]; break;
    default: o[0] = (uint8_t)v[0]; o[1] = (uint8_t)v[1]; o[2] = (uint8_t)v[2]; o[3] = (uint8_t)v[3]; break;
    }
}

// to_rgba16 of a 16-bit pixel (gray replicated, missing alpha 65535)
RPHZ_HD void rgba16_pixel(uint32_t out_ch, const uint32_t v[4], uint16_t o[4])
{
    switch (out_ch) {
    case 1: o[0] = o[1] = o[2] = (uint16_t)v[0]; o[3] = 65535; break;
    case 2: o[0] = o[1] = o[2] = (uint16_t)v[0]; o[3] = (uint16_t)v[1]; break;
    case 3: o[0] = (uint16_t)v[0]; o[1] = (uint16_t)v[1]; o[2] = (uint16_t)v[2]; o[3] = 65535; break;
    default: o[0] = (uint16_t)v[0]; o[1] = (uint16_t)v[1]; o[2] = (uint16_t)v[2]; o[3] = (uint16_t)v[3]; break;
    }
}

}  // namespace rphx
