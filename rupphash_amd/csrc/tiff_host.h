// tiff_host.h -- TIFF container parsing and the pixel rules shared by the host decoder (tiff_host.cpp) and the device kernels
// (tiff_kernels.hip).  Plain C++ for the host half, so that tools/fuzz_tiff_host.cpp can build it with g++ and the sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "inflate.h"
#include "pixel_rules.h"
#include "tiff_lzw.h"

namespace rpht {

// One image (the first IFD) as the decoder needs it, host and device alike.  A segment is a strip (seg_w = w, seg_h = RowsPerStrip) or a
// tile; its decoded bytes are rows of seg_rb bytes in a slot of seg_slot bytes, slot k of the image at dec_off + k * seg_slot.
struct Image {
    uint32_t w, h;
    uint16_t comp;                                          // 1, 5, 8 (32946 is stored as 8), 32773
    uint8_t photo, spp, bps, predictor, big_endian, tiled;  // photo 0 WhiteIsZero, 1 BlackIsZero, 2 RGB
    uint8_t out_ch, out_depth;                              // native layout: 1 L, 2 LA, 3 RGB, 4 RGBA; 8 or 16 bit
    uint8_t hc;                                             // channels of the 8-bit hasher pixels (1 Luma8, 3 Rgb8, 4 Rgba8)
    uint8_t staged;          // device: the segments are read where they were uploaded (Compression 1), not from the decoded buffer
    uint32_t seg_w, seg_h, segs_x, segs_y;
    uint32_t seg_rb;         // bytes per decoded row of a segment
    uint32_t n_segs, first_seg;  // the image's segments in the chunk's table
    uint64_t seg_slot;       // align16(seg_h * seg_rb)
    uint64_t dec_bytes;      // n_segs * seg_slot
    uint64_t dec_off;        // the image's slots in the chunk's decoded buffer
    uint64_t hp_off;         // hasher pixels (rows of hstride bytes) in the chunk's hasher buffer, or ~0
    uint32_t hstride;
    uint64_t x16_off;        // RGBA16 bytes (16-bit images whose pixel hash is wanted), or ~0
    uint64_t nat_off;        // native pixels, or ~0
};

// device work list (tiff_pipeline.cpp -> tiff_kernels.hip), and the host's list of what to copy out of a file
struct Segment {
    uint64_t src_off, src_len;   // in the file
    uint64_t comp_off;           // in the chunk's staging buffer (4-byte aligned)
    uint64_t dec_off, dec_bytes; // in the chunk's decoded buffer (16-byte aligned); dec_bytes: a short last strip holds fewer rows
    uint32_t image, pad;
};

constexpr uint64_t NONE = ~0ull;
constexpr uint64_t MAX_DEC_BYTES = (uint64_t)1 << 30;  // larger images: RPH_ERR_UNSUPPORTED (the PNG bounds)
constexpr uint64_t MAX_PIXELS = (uint64_t)1 << 28;

// The most bytes `comp_len` compressed bytes can decode to: 1032:1 Deflate (a 258-byte copy from 2 bits), 128:2 PackBits (a run of
// 128 from two bytes), 1:1 uncompressed, LZW_MAX_STRING bytes from every 9 bits (tiff_lzw.h)
inline uint64_t max_expansion(uint32_t comp, uint64_t comp_len)
{
    switch (comp) {
    case 1: return comp_len;
    case 5: return LZW_MAX_STRING * (comp_len * 8 / 9);
    case 8: return 1032 * comp_len;
    default: return 64 * comp_len;
    }
}

struct Parsed {
    Image im;
    std::vector<Segment> segs;  // comp_off / dec_off relative to the image
    uint64_t comp_bytes = 0;    // the segments' compressed bytes, each rounded up to 4
};

// Header, first IFD, geometry, every offset and size; RPH_OK, RPH_ERR_INVALID_ARG (damaged) or RPH_ERR_UNSUPPORTED (a layout left to the
// caller's decoders, implausible or too large), by the rule of include/rupphash.h.
int parse(const uint8_t *data, size_t len, Parsed &p);
// One segment on the host: dec_bytes bytes into out; false for a stream the rule refuses
bool decompress_host(uint32_t comp, const uint8_t *in, size_t n, uint8_t *out, uint64_t dec_bytes);
// The whole decoder on the host: native pixels (w * h * out_ch samples of out_depth bits, u16 in native byte order)
int decode_host(const uint8_t *data, size_t len, Parsed &p, std::vector<uint8_t> &native);

// The stored sample c of segment-local pixel px in a decoded row (before the predictor): 16-bit words in the file's byte order
RPHZ_HD uint32_t stored_sample(const Image &im, const uint8_t *row, uint32_t px, uint32_t c)
{
    if (im.bps < 8) {
        const uint32_t bit = px * im.bps;
        return (row[bit >> 3] >> (8 - im.bps - (bit & 7))) & ((1u << im.bps) - 1);
    }
    if (im.bps == 8) return row[px * im.spp + c];
    const uint8_t *q = row + 2 * (px * im.spp + c);
    return im.big_endian ? ((uint32_t)q[0] << 8) | q[1] : ((uint32_t)q[1] << 8) | q[0];
}

// After the predictor: WhiteIsZero inverts every sample (the tiff crate inverts the whole buffer, an alpha sample included: UNPINNED),
// sub-8-bit gray is scaled by 255 / (2^d - 1)
RPHZ_HD uint32_t native_sample(const Image &im, uint32_t v)
{
    const uint32_t maxv = (1u << im.bps) - 1;
    if (im.photo == 0) v = maxv - v;
    return im.bps < 8 ? v * (255u / maxv) : v;
}

}  // namespace rpht
