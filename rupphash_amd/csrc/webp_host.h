// webp_host.h -- WebP container parsing, the serial front of a VP8L stream and the image description shared by the host decoder
// (webp_host.cpp) and the device kernels (webp_kernels.hip).  Plain C++ for the host half, so that tools/fuzz_webp_host.cpp can build it
// with g++ and the sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "vp8l.h"

namespace rphw {

// one transform as its inverse needs it: `xsize` is the width of the image it applies to (colour indexing: of the bundled image it
// reads), `off` the first word of its sub-image (predictor, cross-colour: subsample(xsize, bits) words per row) or of its palette
// (256 words, zero past the last colour) in the chunk's table of words
struct Xform {
    uint32_t type, bits, xsize, off;
};

// One image as the decoder needs it, host and device alike
struct Image {
    uint32_t w, h;
    uint32_t xw;                         // width of the coded ARGB image (w, or fewer when colour indexing bundles pixels)
    uint8_t out_ch, out_depth, hc, n_tr;  // native layout 3 Rgb8 / 4 Rgba8, depth 8; channels of the hasher's pixels; transforms read
    uint32_t hstride;
    uint64_t hp_off, x16_off, nat_off;  // (decoded_hash.h; x16_off stays ~0: no 16-bit WebP)
    Xform tr[4];                        // in the order read; undone last to first
    uint64_t a_off, b_off;              // words: the coded image in the chunk's ARGB buffer, and (colour indexing) the unbundled one
    uint32_t cache_bits, meta_bits, has_ent, n_groups;
    uint64_t ent_off, tab_off;          // uint16 units in the chunk's table of codes: entropy image (group per block), the groups' tables
    uint64_t comp_off, comp_len;        // the VP8L chunk's bytes in the chunk's staging buffer (4-byte aligned, zero-padded)
    uint64_t bit_start;                 // where the main ARGB stream begins in them
};

constexpr uint64_t NONE = ~0ull;
constexpr uint64_t MAX_PIXELS = (uint64_t)1 << 28;       // larger images: RPH_ERR_UNSUPPORTED (the PNG bound)
constexpr uint64_t MAX_TABLE_BYTES = (uint64_t)64 << 20;  // more prefix-code tables than this: RPH_ERR_UNSUPPORTED

struct Parsed {
    Image im;
    const uint8_t *chunk = nullptr;  // the VP8L chunk's payload inside the file
    size_t chunk_len = 0;
    std::vector<uint32_t> words;   // sub-images and palettes of the transforms (Xform::off relative to it)
    std::vector<uint16_t> codes;   // entropy image, then the tables (ent_off / tab_off relative to it)
};

// Container and VP8L header only: geometry, alpha, the size limit.  RPH_OK, RPH_ERR_INVALID_ARG or RPH_ERR_UNSUPPORTED by the rule of
// include/rupphash.h.
int parse(const uint8_t *data, size_t len, Parsed &p);
// parse + the serial front of the stream: transforms with their sub-images, colour cache, entropy image, every group's tables; leaves
// im.bit_start at the main ARGB stream
int front(const uint8_t *data, size_t len, Parsed &p);
// The main ARGB stream on the host: xw * h words into argb; false for a stream the rule refuses
bool decode_main_host(const Parsed &p, uint32_t *argb);
// The whole decoder on the host: native pixels (w * h * out_ch bytes)
int decode_host(const uint8_t *data, size_t len, Parsed &p, std::vector<uint8_t> &native);

}  // namespace rphw
