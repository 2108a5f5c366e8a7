// bmp_host.h -- BMP container parsing, the RLE walk and the image descriptor shared by the host decoder (bmp_host.cpp), the pipeline
// (bmp_pipeline.cpp) and the expand kernel (bmp_kernels.hip).  Plain C++ for the host half, so that tools/fuzz_bmp_host.cpp can build it
// with g++ and the sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#if defined(__HIP__) || defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RPHB_HD __host__ __device__ __attribute__((always_inline)) inline
#else
#define RPHB_HD inline
#endif

namespace rphb {

enum Kind : uint8_t {
    K_PAL = 0,     // 1, 2, 4 or 8 bits per pixel, most significant bits first: indices into the palette
    K_BGR24 = 1,   // three bytes per pixel: B, G, R
    K_FIELDS = 2,  // 16 or 32 bits per pixel, little-endian: four bit fields
};

// One file as the expand kernel needs it.  The source is what the pipeline staged: the file's pixel array as it lies in the file, or,
// for an RLE file, the plane the host threads decoded (K_PAL at 8 bits; K_BGR24 when skipped pixels need a black no palette index has),
// rows of src_stride bytes in file order.
struct Image {
    uint32_t w, h;
    uint8_t kind, bits, top_down, out_ch;  // out_ch: 3 (Rgb8) or 4 (Rgba8, a non-zero alpha mask)
    // K_FIELDS, channel R, G, B, A: sample = (pixel >> shift) & ((1 << len) - 1), len <= 8 (a wider field keeps its top 8 bits: the
    // parser moves shift up); len 0: a zero mask, the sample is 0
    uint8_t shift[4], len[4];
    uint8_t bytes8;  // K_FIELDS at 32 bits whose fields are whole bytes (or zero): a byte permute does it, no table
    uint8_t pad0;
    uint16_t pal_n;        // K_PAL: entries of the palette; an index past it is black
    uint32_t pal_off;      // its place in the chunk's palette table, in words (R | G << 8 | B << 16)
    uint32_t src_stride;   // bytes between source rows, a multiple of 4
    uint32_t out_stride;   // bytes between native rows on the device: align_up(w * out_ch, 4)
    uint32_t band;         // rows of one work item
    uint32_t pad1;
    uint64_t src_off;      // the source in the chunk's staging buffer (16-byte aligned)
    uint64_t out_off;      // the native pixels in the chunk's pixel buffer (256-byte aligned)
};
static_assert(sizeof(Image) % 8 == 0, "descriptors follow each other in the metadata");

// one work item of the expand kernel: rows [row0, row0 + band) of image img
struct Work {
    uint32_t img, row0;
};

constexpr uint64_t MAX_PIXELS = (uint64_t)1 << 28;  // more: RPH_ERR_UNSUPPORTED (the PNG bound)
constexpr uint32_t MAX_SIDE = 65535;
constexpr uint32_t GROUPS_PER_ITEM = 2048;  // a work item covers about this many groups of four pixels

struct Parsed {
    Image im;
    uint32_t pal[256];
    size_t data_off = 0;   // the pixel array in the file
    size_t data_len = 0;   // uncompressed: src_stride * h; RLE: the rest of the file
    uint8_t rle = 0;       // 0, 8 or 4
    bool rle_skips = false;  // the RLE stream leaves pixels out
};

// File header, DIB header, masks, palette, pixel-array offset and size; for an RLE file the whole stream is walked.  RPH_OK,
// RPH_ERR_INVALID_ARG (damaged) or RPH_ERR_UNSUPPORTED, by the rule of include/rupphash.h: a file that parses decodes.
int parse(const uint8_t *data, size_t len, Parsed &p);
// What the kernel reads, into dst (im.src_stride * im.h bytes): a copy of the pixel array, or the decoded RLE plane
void stage(const uint8_t *data, const Parsed &p, uint8_t *dst);
// The whole decoder on the host: native pixels, top-down, rows packed (w * h * out_ch bytes)
int decode_host(const uint8_t *data, size_t len, Parsed &p, std::vector<uint8_t> &native);

// the scaling of a sample v of len bits (1 .. 8) to 8 bits, round to nearest: max = 2^len - 1 is odd, so there are no ties
RPHB_HD uint32_t scale_sample(uint32_t v, uint32_t len)
{
    const uint32_t max = (1u << len) - 1;
    return (v * 255 + max / 2) / max;
}

}  // namespace rphb
