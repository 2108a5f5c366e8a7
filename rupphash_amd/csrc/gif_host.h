// gif_host.h -- GIF container parsing and the pixel rule shared by the host decoder (gif_host.cpp) and the device kernels
// (gif_kernels.hip).  Plain C++ for the host half, so that tools/fuzz_gif_host.cpp can build it with g++ and the sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "gif_lzw.h"

namespace rphg {

// One file (its first frame on its logical screen) as the decoder needs it, host and device alike.  The frame's palette indices are
// fw * fh bytes in the order the stream holds them: rows in pass order when the frame is interlaced.
struct Image {
    uint32_t w, h;              // the logical screen: the size of the native pixels
    uint32_t fx, fy, fw, fh;    // the first frame on it (it may reach past the screen: clipped)
    uint8_t interlaced, m;      // m: the minimum code size
    uint8_t has_trans, trans;   // the last Graphic Control Extension before the frame
    uint16_t pal_n;             // entries of the palette in force (local, else global)
    uint8_t out_ch, out_depth;  // native layout: always 4 x 8 (Rgba8)
    uint8_t hc;                 // channels of the 8-bit hasher pixels: 4
    uint32_t pal_off;           // the palette (pal_n words, R | G << 8 | B << 16) in the chunk's palette table, in words
    uint64_t comp_off, comp_len;  // the joined stream in the chunk's staging buffer (4-byte aligned)
    uint64_t dec_off;           // the frame's indices in the chunk's decoded buffer (16-byte aligned)
    uint64_t hp_off;            // hasher pixels (rows of hstride bytes) in the chunk's hasher buffer, or ~0
    uint32_t hstride;
    uint64_t x16_off;           // never used (no 16-bit GIF): ~0
    uint64_t nat_off;           // native pixels, or ~0
};

constexpr uint64_t NONE = ~0ull;
constexpr uint64_t MAX_PIXELS = (uint64_t)1 << 28;  // a larger screen or frame: RPH_ERR_UNSUPPORTED (the PNG bound)

struct Parsed {
    Image im;
    uint32_t pal[256];
    size_t data_off = 0;      // the first data sub-block of the frame in the file
    uint64_t stream_len = 0;  // the bytes of its sub-blocks, joined
};

// Signature, screen descriptor, colour tables, the blocks before the first image descriptor, that descriptor and the sub-block chain of
// its data; RPH_OK, RPH_ERR_INVALID_ARG (damaged) or RPH_ERR_UNSUPPORTED, by the rule of include/rupphash.h.  The codes are not read.
int parse(const uint8_t *data, size_t len, Parsed &p);
// The frame's data sub-blocks joined into dst[0 .. stream_len)
void join(const uint8_t *data, const Parsed &p, uint8_t *dst);
// The joined stream on the host: fw * fh indices into out; false for a stream the rule refuses
bool decode_indices_host(const uint8_t *stream, size_t n, const Image &im, uint8_t *out);
// The whole decoder on the host: native pixels (w * h * 4 bytes)
int decode_host(const uint8_t *data, size_t len, Parsed &p, std::vector<uint8_t> &native);

// Where row r of an interlaced frame of h rows lies in the stream: rows 0, 8, ... first, then 4, 12, ..., then 2, 6, ..., then 1, 3, ...
RPHG_HD uint32_t interlaced_row(uint32_t r, uint32_t h)
{
    if ((r & 7) == 0) return r >> 3;
    const uint32_t n1 = (h + 7) >> 3;
    if ((r & 7) == 4) return n1 + (r >> 3);
    const uint32_t n2 = (h + 3) >> 3;
    if ((r & 3) == 2) return n1 + n2 + (r >> 2);
    const uint32_t n3 = (h + 1) >> 2;
    return n1 + n2 + n3 + (r >> 1);
}

// The pixel rule: screen pixel (x, y) as R | G << 8 | B << 16 | A << 24 (the bytes of an Rgba8 pixel in memory order).  Inside the
// frame: the palette's RGB with alpha 255, alpha 0 where the index is the transparent one, (0, 0, 0, 0) for an index past the
// palette; outside the frame (0, 0, 0, 0).
RPHG_HD uint32_t screen_pixel(const Image &im, const uint32_t *pal, const uint8_t *idx, uint32_t x, uint32_t y)
{
    if (x < im.fx || y < im.fy || x - im.fx >= im.fw || y - im.fy >= im.fh) return 0;
    const uint32_t r = y - im.fy, row = im.interlaced ? interlaced_row(r, im.fh) : r;
    const uint32_t i = idx[(uint64_t)row * im.fw + (x - im.fx)];
    if (i >= im.pal_n) return 0;
    return pal[i] | (im.has_trans && i == im.trans ? 0u : 0xff000000u);
}

}  // namespace rphg
