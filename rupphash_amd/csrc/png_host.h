// png_host.h -- PNG container parsing and the pixel rules shared by the host decoder (png_host.cpp) and the device kernels
// (png_kernels.hip).  Plain C++ for the host half, so that tools/fuzz_png_host.cpp can build it with g++ and the sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "inflate.h"
#include "pixel_rules.h"

namespace rphp {

// Adam7 passes: x0, y0, dx, dy (pass 0 of a non-interlaced image is the whole image)
RPHZ_HD void adam7(int p, uint32_t &x0, uint32_t &y0, uint32_t &dx, uint32_t &dy)
{
    // (0,0,8,8) (4,0,8,8) (0,4,4,8) (2,0,4,4) (0,2,2,4) (1,0,2,2) (0,1,1,2), as arithmetic
    dx = 8u >> (p / 2);
    dy = p == 0 ? 8u : 8u >> ((p - 1) / 2);
    x0 = (p & 1) ? dx / 2 : 0;
    y0 = (p && !(p & 1)) ? dy / 2 : 0;
}

// One image as the decoder needs it (host and device alike).  Offsets are relative to the buffers of a call chunk.
struct Image {
    uint32_t w, h;
    uint8_t depth, ctype, interlace, has_trns;
    uint8_t out_ch, out_depth;  // native layout: 1 L, 2 LA, 3 RGB, 4 RGBA; 8 or 16 bit
    uint8_t unit;               // bytes per filter unit: max(1, bits per pixel / 8)
    uint8_t hc;                 // channels of the 8-bit hasher pixels (1 Luma8, 3 Rgb8, 4 Rgba8)
    uint16_t key[3];            // tRNS of colour types 0 and 2
    uint16_t plte_n, trns_n;    // palette entries, palette alpha entries
    uint32_t bpp_bits;          // bits per pixel in the file
    uint32_t pass_w[7], pass_h[7], pass_rb[7];  // rowbytes without the filter byte
    uint64_t pass_off[7];       // offset of each pass inside the image's raw bytes
    uint64_t raw_bytes;         // inflated size of the image: sum over passes of rows * (1 + rowbytes)
    uint64_t raw_off;           // the image's raw bytes in the chunk's raw buffer
    uint64_t hp_off;            // hasher pixels (rows of hstride bytes) in the chunk's hasher buffer, or ~0
    uint32_t hstride;
    uint32_t pal;               // index of the image's 1 KiB palette block (rgb 768 + alpha 256)
    uint64_t x16_off;           // RGBA16 bytes in the chunk's buffer (16-bit images whose pixel hash is wanted), or ~0
    uint64_t nat_off;           // native pixels, or ~0
};

// device work lists (png_pipeline.cpp -> png_kernels.hip)
struct StreamDesc {
    uint64_t comp_off, comp_len, raw_off, raw_bytes;
    uint32_t image, pad;
};
struct UnfilterJob {
    uint64_t off;  // first row (its filter byte) in the raw buffer
    uint32_t rows, rowbytes, unit, image;
};

constexpr uint64_t NONE = ~0ull;
constexpr uint64_t MAX_RAW_BYTES = (uint64_t)1 << 30;  // larger images: RPH_ERR_UNSUPPORTED
constexpr uint64_t MAX_PIXELS = (uint64_t)1 << 28;
constexpr uint64_t INFLATE_RATIO = 1032;                // deflate expands at most 1032:1 (a 258-byte copy from 2 bits)

struct Parsed {
    Image im;
    uint8_t palette[1024];  // rgb x 256, then alpha x 256
    std::vector<std::pair<size_t, size_t>> idat;  // (offset, length) of each IDAT payload in the file
    size_t idat_bytes = 0;
};

// Signature, chunks, CRCs, IHDR / PLTE / tRNS; fills the geometry (raw_off etc. left at 0).  Returns RPH_OK, RPH_ERR_INVALID_ARG
// (damaged) or RPH_ERR_UNSUPPORTED (implausible or too large), by the rule of include/rupphash.h.
int parse(const uint8_t *data, size_t len, Parsed &p);
// IDAT payloads back to back into dst (p.idat_bytes)
void gather(const uint8_t *data, const Parsed &p, uint8_t *dst);
// Undo the filters of the image's raw bytes in place; false for a filter type above 4
bool unfilter_host(const Image &im, uint8_t *raw);
// The whole decoder on the host: native pixels (w * h * out_ch samples of out_depth bits, u16 in native byte order)
int decode_host(const uint8_t *data, size_t len, Parsed &p, std::vector<uint8_t> &native);
uint32_t crc32(const uint8_t *p, size_t n, uint32_t c = 0);

// The sample of pass-local pixel (px, py), channel c, from unfiltered raw bytes
RPHZ_HD uint32_t sample(const Image &im, const uint8_t *raw, int pass, uint32_t px, uint32_t py, uint32_t c)
{
    const uint8_t *row = raw + im.pass_off[pass] + (uint64_t)py * (1 + im.pass_rb[pass]) + 1;
    if (im.depth < 8) {
        const uint32_t bit = px * im.depth;
        return (row[bit >> 3] >> (8 - im.depth - (bit & 7))) & ((1u << im.depth) - 1);
    }
    const uint32_t nch = im.bpp_bits / im.depth;
    if (im.depth == 8) return row[px * nch + c];
    const uint8_t *q = row + 2 * (px * nch + c);
    return ((uint32_t)q[0] << 8) | q[1];
}

RPHZ_HD int pass_of(const Image &im, uint32_t x, uint32_t y, uint32_t &px, uint32_t &py)
{
    const int p = !im.interlace ? 0 : (y & 1) ? 6 : (x & 1) ? 5 : (y & 2) ? 4 : (x & 2) ? 3 : (y & 4) ? 2 : (x & 4) ? 1 : 0;
    uint32_t x0, y0, dx, dy;
    adam7(p, x0, y0, dx, dy);
    const uint32_t sx = im.interlace ? 31 - __builtin_clz(dx) : 0, sy = im.interlace ? 31 - __builtin_clz(dy) : 0;  // (powers of two)
    px = (x - (im.interlace ? x0 : 0)) >> sx;
    py = (y - (im.interlace ? y0 : 0)) >> sy;
    return p;
}

// The native pixel (x, y) by the EXPAND rules: v[0 .. out_ch) in out_depth bits (all four written once, at the end: a store per
// case would let the compiler merge them through a pointer and keep v in private memory)
RPHZ_HD void pixel(const Image &im, const uint8_t *raw, const uint8_t *pal, uint32_t x, uint32_t y, uint32_t v[4])
{
    uint32_t px, py;
    const int p = pass_of(im, x, y, px, py);
    const uint32_t maxv = im.out_depth == 16 ? 65535u : 255u;
    uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    switch (im.ctype) {
    case 0: {
        const uint32_t g = sample(im, raw, p, px, py, 0);
        c0 = im.depth < 8 ? g * (255u / ((1u << im.depth) - 1)) : g;
        c1 = (im.has_trns && g == im.key[0]) ? 0 : maxv;
        break;
    }
    case 2:
        c0 = sample(im, raw, p, px, py, 0);
        c1 = sample(im, raw, p, px, py, 1);
        c2 = sample(im, raw, p, px, py, 2);
        c3 = (im.has_trns && c0 == im.key[0] && c1 == im.key[1] && c2 == im.key[2]) ? 0 : maxv;
        break;
    case 3: {
        const uint32_t i = sample(im, raw, p, px, py, 0);
        if (i < im.plte_n) {
            c0 = pal[3 * i];
            c1 = pal[3 * i + 1];
            c2 = pal[3 * i + 2];
            c3 = i < im.trns_n ? pal[768 + i] : 255;
        } else {
            c3 = 255;
        }
        break;
    }
    case 4:
        c0 = sample(im, raw, p, px, py, 0);
        c1 = sample(im, raw, p, px, py, 1);
        break;
    default:
        c0 = sample(im, raw, p, px, py, 0);
        c1 = sample(im, raw, p, px, py, 1);
        c2 = sample(im, raw, p, px, py, 2);
        c3 = sample(im, raw, p, px, py, 3);
        break;
    }
    v[0] = c0;
    v[1] = c1;
    v[2] = c2;
    v[3] = c3;
}

// The 8-bit pixels the hasher takes (hc channels) and to_rgba16 of a 16-bit pixel: pixel_rules.h, shared with the TIFF path
RPHZ_HD void hasher_pixel(const Image &im, const uint32_t v[4], uint8_t o[4]) { rphx::hasher_pixel(im.out_ch, im.out_depth, v, o); }
RPHZ_HD void rgba16_pixel(const Image &im, const uint32_t v[4], uint16_t o[4]) { rphx::rgba16_pixel(im.out_ch, v, o); }

RPHZ_HD uint8_t paeth(int a, int b, int c)
{
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return (uint8_t)((pa <= pb && pa <= pc) ? a : pb <= pc ? b : c);
}

// One filtered byte back: x filtered, a left, b above, c above-left
RPHZ_HD uint8_t unfilter_byte(uint32_t f, uint8_t x, uint8_t a, uint8_t b, uint8_t c)
{
    switch (f) {
    case 1: return (uint8_t)(x + a);
    case 2: return (uint8_t)(x + b);
    case 3: return (uint8_t)(x + ((a + b) >> 1));
    case 4: return (uint8_t)(x + paeth(a, b, c));
    default: return x;
    }
}

}  // namespace rphp
