// bmp_kernels.hip -- the device half of the BMP path (bmp_pipeline.cpp): one expand kernel for gfx950.
//
// The pixel array of a BMP crosses PCIe as it lies in the file; this kernel turns it into the native pixels (top-down Rgb8 or Rgba8, rows
// of align_up(w * channels, 4) bytes) that rph_image_hash_ragged_dev hashes where they lie.  The work is data: a workgroup takes one
// (image, row band) item of the chunk's work list and reads the image's descriptor with uniform loads, so a chunk of thousands of sizes
// and depths is one launch.
//   - A lane turns PX_PER_LANE = 4 pixels into three (Rgb8) or four (Rgba8) whole dwords at every depth; a wave pass covers 256 pixels.
//     Source rows are multiples of 4 bytes and so are native rows: every load and store is an aligned dword, guarded by its row's length.
//     A band is flattened over the workgroup's 256 threads (row, group) so that narrow images keep the lanes busy; the step (256 / G,
//     256 % G) is uniform, so a lane divides once.
//   - 24 bits: three dwords in (B G R B | G R B G | R B G R), four v_perm_b32, three dwords out, rows flipped.
//   - 32 bits with whole-byte fields (BGRX, BGRA, ...): one v_perm_b32 per pixel picks R G B A; 16 bits and odd 32-bit fields: shift and
//     mask per channel, then the channel's 8-bit value from a table of 2^len entries in LDS ((v * 255 + max / 2) / max, divided once per
//     entry by the workgroup, never per pixel).
//   - 1, 2, 4, 8 bits (RLE files arrive as 8-bit planes): the dword that holds the lane's four pixels, most significant bits first, and
//     the palette from LDS (256 words, black behind the palette's last entry).  Neighbouring lanes read the same dword at depths < 8.
//   - LDS: 2 KiB per workgroup.  Palette reads are one dword per lane at a data-dependent address (conflicts as the indices fall);
//     the byte tables are read the same way.  The kernel moves 6 .. 8 bytes per pixel and does a few dozen VALU operations for four.
// The host has checked every size and offset (bmp_host.cpp); the guards here are the rows' ends.
#include "bmp_host.h"
#include "rph_internal.h"

namespace {

using rphb::Image;
using rphb::Work;

constexpr uint32_t PX_PER_LANE = 4;
constexpr uint32_t THREADS = 256;

// byte k of the result = byte sel[k] of the eight bytes {hi, lo}: 0..3 from lo, 4..7 from hi, 12 = 0x00
__device__ __forceinline__ uint32_t perm(uint32_t hi, uint32_t lo, uint32_t sel) { return __builtin_amdgcn_perm(hi, lo, sel); }

__global__ void __launch_bounds__(THREADS) bmp_expand_kernel(const uint8_t *__restrict__ src, const Image *__restrict__ imgs, const uint32_t *__restrict__ pals,
                                                             const Work *__restrict__ work, uint8_t *__restrict__ out)
{
    __shared__ uint32_t pal[256];
    __shared__ uint8_t tbl[4][256];
    const Work wk = work[blockIdx.x];
    const Image im = imgs[wk.img];
    const uint32_t t = threadIdx.x;
    const bool table = im.kind == rphb::K_FIELDS && !im.bytes8;
    if (im.kind == rphb::K_PAL) pal[t] = t < im.pal_n ? pals[im.pal_off + t] : 0u;
    if (table)
        for (uint32_t c = 0; c < 4; c++) tbl[c][t] = im.len[c] && t < (1u << im.len[c]) ? (uint8_t)rphb::scale_sample(t, im.len[c]) : (uint8_t)0;
    __syncthreads();

    const uint32_t G = (im.w + PX_PER_LANE - 1) / PX_PER_LANE;
    const uint32_t rows = im.h - wk.row0 < im.band ? im.h - wk.row0 : im.band, total = rows * G;
    const uint32_t dr = THREADS / G, dg = THREADS % G;
    const uint32_t sdw = im.src_stride / 4, odw = im.out_stride / 4, bits = im.bits;
    const bool rgba = im.out_ch == 4;
    // K_FIELDS: the channels' masks; whole-byte fields: the selector that picks R G B A out of the pixel (0x00 for a channel without mask)
    uint32_t cm[4], bsel = 0;
    for (uint32_t c = 0; c < 4; c++) {
        cm[c] = (1u << im.len[c]) - 1;
        bsel |= ((c == 3 && !rgba) || !im.len[c] ? 0x0cu : (uint32_t)im.shift[c] >> 3) << (8 * c);
    }
    uint32_t r = t / G, g = t - r * G;
    for (uint32_t i = t; i < total; i += THREADS) {
        const uint32_t y = wk.row0 + r;
        const uint32_t *srow = reinterpret_cast<const uint32_t *>(src + im.src_off + (uint64_t)(im.top_down ? y : im.h - 1 - y) * im.src_stride);
        uint32_t *orow = reinterpret_cast<uint32_t *>(out + im.out_off + (uint64_t)y * im.out_stride);
        uint32_t o0, o1, o2;
        if (im.kind == rphb::K_BGR24) {  // (uniform)
            const uint32_t a = 3 * g;
            const uint32_t d0 = srow[a], d1 = a + 1 < sdw ? srow[a + 1] : 0u, d2 = a + 2 < sdw ? srow[a + 2] : 0u;
            o0 = perm(d1, d0, 0x05000102u);                               // R0 G0 B0 R1
            o1 = perm(d2, perm(d1, d0, 0x07000304u), 0x03040100u);        // G1 B1 R2 G2
            o2 = perm(d2, d1, 0x05060702u);                               // B2 R3 G3 B3
        } else {
            uint32_t p[4];  // R | G << 8 | B << 16 | A << 24
            if (im.kind == rphb::K_PAL) {
                const uint32_t d = srow[(g * bits) >> 3], vm = (1u << bits) - 1;
#pragma unroll
                for (uint32_t k = 0; k < 4; k++) {
                    const uint32_t bit = (g * 4 + k) * bits, byte = (d >> (8 * ((bit >> 3) & 3))) & 0xffu;
                    p[k] = pal[(byte >> (8 - bits - (bit & 7))) & vm];
                }
            } else {
                uint32_t v[4];
                if (bits == 16) {
                    const uint32_t a = 2 * g, d0 = srow[a], d1 = a + 1 < sdw ? srow[a + 1] : 0u;
                    v[0] = d0 & 0xffffu, v[1] = d0 >> 16, v[2] = d1 & 0xffffu, v[3] = d1 >> 16;
                } else {
#pragma unroll
                    for (uint32_t k = 0; k < 4; k++) v[k] = 4 * g + k < sdw ? srow[4 * g + k] : 0u;
                }
#pragma unroll
                for (uint32_t k = 0; k < 4; k++) {
                    if (!table) {
                        p[k] = perm(0u, v[k], bsel);
                    } else {
                        p[k] = (uint32_t)tbl[0][(v[k] >> im.shift[0]) & cm[0]] | ((uint32_t)tbl[1][(v[k] >> im.shift[1]) & cm[1]] << 8) |
                               ((uint32_t)tbl[2][(v[k] >> im.shift[2]) & cm[2]] << 16);
                        if (rgba) p[k] |= (uint32_t)tbl[3][(v[k] >> im.shift[3]) & cm[3]] << 24;
                    }
                }
            }
            if (rgba) {
#pragma unroll
                for (uint32_t k = 0; k < 4; k++)
                    if (4 * g + k < odw) orow[4 * g + k] = p[k];
            }
            o0 = perm(p[1], p[0], 0x04020100u);  // R0 G0 B0 R1
            o1 = perm(p[2], p[1], 0x05040201u);  // G1 B1 R2 G2
            o2 = perm(p[3], p[2], 0x06050402u);  // B2 R3 G3 B3
        }
        if (!rgba) {
            const uint32_t a = 3 * g;
            orow[a] = o0;
            if (a + 1 < odw) orow[a + 1] = o1;
            if (a + 2 < odw) orow[a + 2] = o2;
        }
        g += dg, r += dr;
        if (g >= G) g -= G, r++;
    }
}

}  // namespace

// one workgroup per item of d_work[0 .. n_work)
int rph_bmp_launch_expand(const uint8_t *d_src, const void *d_images, const uint32_t *d_pals, const void *d_work, uint32_t n_work, uint8_t *d_out, hipStream_t s)
{
    if (!n_work) return RPH_OK;
    hipLaunchKernelGGL(bmp_expand_kernel, dim3(n_work), dim3(THREADS), 0, s, d_src, (const Image *)d_images, d_pals, (const Work *)d_work, d_out);
    RPH_HIP_CHECK(hipGetLastError());
    return RPH_OK;
}
