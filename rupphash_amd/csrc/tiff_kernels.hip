// tiff_kernels.hip -- the device half of the TIFF path (tiff_pipeline.cpp): LZW, PackBits, expand.  (Deflate strips and tiles run
// through png_inflate_kernel, one wave per segment: its sink stores what lies below the segment's bytes and checks the rest.)
//
// lzw: one wave per segment (strip or tile), uniform control flow: every lane runs tiff_lzw.h on the same bits.  The string table
//   (position in the segment's output, length: 24 KiB) lives in LDS.  A code is one copy of bytes the segment already holds, 64 bytes
//   per step.  A segment of up to 16 KiB (libtiff's default strips are 8 KiB) is built in LDS and stored with 16-byte stores at the
//   end; a larger one is built in global memory, where every copy waits for the stores before it.  40 KiB of LDS per wave, four
//   waves per CU.  The bit reader loads dwords (tiff_lzw.h).
// packbits: one wave per segment; a literal run or a fill is written by the whole wave.
// expand: one wave per row of a segment, 64 pixels per step: byte order, predictor 2 as an inclusive scan across the wave per sample
//   channel with a carry between steps, WhiteIsZero, sub-8-bit scaling, tile placement; writes the hasher's 8-bit pixels, the RGBA16
//   bytes of 16-bit images (pixel hash) and / or the native pixels.
// Every loop is bounded by the segment's input bits or output bytes (tiff_lzw.h), and the host has checked every offset and size.
#include "rph_internal.h"
#include "tiff_host.h"
#include "wave_sink.h"

namespace {

using rpht::Image;
using rpht::Segment;

constexpr uint32_t LDS_SEG = 16384;

using DevSegSink = WaveSink;  // the segment's output, LDS or global memory, written by the whole wave

__global__ void __launch_bounds__(64) tiff_lzw_kernel(const uint8_t *__restrict__ comp, const Segment *__restrict__ segs, uint8_t *dec, int32_t *__restrict__ status)
{
    __shared__ rpht::LzwTable table;
    __shared__ __attribute__((aligned(16))) uint8_t seg[LDS_SEG];
    const Segment d = segs[blockIdx.x];
    const bool in_lds = d.dec_bytes <= LDS_SEG;
    DevSegSink s{in_lds ? seg : dec + d.dec_off, d.dec_bytes, 0, threadIdx.x};
    const int rc = rpht::lzw_decode(comp + d.comp_off, d.src_len, table, s);
    if (rc != rpht::L_OK) {
        if (threadIdx.x == 0) status[d.image] = RPH_ERR_INVALID_ARG;
        return;
    }
    if (in_lds) {
        __syncthreads();
        // (the slot is a multiple of 16 bytes and 16-byte aligned: the last store may carry bytes past dec_bytes, inside the slot)
        for (uint32_t o = threadIdx.x * 16; o < d.dec_bytes; o += 64 * 16) *reinterpret_cast<uint4 *>(dec + d.dec_off + o) = *reinterpret_cast<const uint4 *>(seg + o);
    }
}

__global__ void __launch_bounds__(64) tiff_packbits_kernel(const uint8_t *__restrict__ comp, const Segment *__restrict__ segs, uint8_t *__restrict__ dec,
                                                            int32_t *__restrict__ status)
{
    const Segment d = segs[blockIdx.x];
    DevSegSink s{dec + d.dec_off, d.dec_bytes, 0, threadIdx.x};
    if (rpht::packbits_decode(comp + d.comp_off, d.src_len, s) != rpht::L_OK && threadIdx.x == 0) status[d.image] = RPH_ERR_INVALID_ARG;
}

__global__ void __launch_bounds__(256) tiff_expand_kernel(const uint8_t *__restrict__ comp, const uint8_t *__restrict__ dec, const Image *__restrict__ imgs,
                                                          const Segment *__restrict__ segs, const uint32_t *__restrict__ list, uint8_t *__restrict__ hp,
                                                          uint8_t *__restrict__ x16, uint8_t *__restrict__ nat)
{
    const Image im = imgs[list[blockIdx.y]];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t mask = (1u << im.bps) - 1;
    const uint64_t jobs = (uint64_t)im.segs_x * im.h;  // one per row of a segment
    for (uint64_t j = (uint64_t)blockIdx.x * 4 + wave; j < jobs; j += (uint64_t)gridDim.x * 4) {
        const uint32_t y = (uint32_t)(j / im.segs_x), sx = (uint32_t)(j % im.segs_x);
        const Segment &sg = segs[im.first_seg + (y / im.seg_h) * im.segs_x + sx];
        const uint8_t *row = (im.staged ? comp + sg.comp_off : dec + sg.dec_off) + (uint64_t)(y % im.seg_h) * im.seg_rb;
        const uint32_t x0 = sx * im.seg_w, npx = im.w - x0 < im.seg_w ? im.w - x0 : im.seg_w;  // (an edge tile is cropped)
        uint32_t carry[4] = {0, 0, 0, 0};
        for (uint32_t p0 = 0; p0 < npx; p0 += 64) {
            const uint32_t px = p0 + lane;
            const bool live = px < npx;
            uint32_t v[4] = {0, 0, 0, 0};
#pragma unroll
            for (uint32_t c = 0; c < 4; c++)
                if (live && c < im.spp) v[c] = rpht::stored_sample(im, row, px, c);
            if (im.predictor == 2) {
#pragma unroll
                for (uint32_t c = 0; c < 4; c++) {
                    if (c >= im.spp) continue;
                    uint32_t s = v[c];
#pragma unroll
                    for (int off = 1; off < 64; off <<= 1) {
                        const uint32_t t = __shfl_up(s, off);
                        if ((int)lane >= off) s += t;
                    }
                    s = (s + carry[c]) & mask;
                    carry[c] = __shfl(s, 63);
                    v[c] = s;
                }
            }
            if (!live) continue;
#pragma unroll
            for (uint32_t c = 0; c < 4; c++)
                if (c < im.spp) v[c] = rpht::native_sample(im, v[c]);
            const uint32_t x = x0 + px;
            const uint64_t q = (uint64_t)y * im.w + x;
            if (im.hp_off != rpht::NONE) {
                uint8_t o[4];
                rphx::hasher_pixel(im.out_ch, im.out_depth, v, o);
                uint8_t *d = hp + im.hp_off + (uint64_t)y * im.hstride + (uint64_t)x * im.hc;
#pragma unroll
                for (uint32_t c = 0; c < 4; c++)
                    if (c < im.hc) d[c] = o[c];
            }
            if (im.x16_off != rpht::NONE) {
                uint16_t o[4];
                rphx::rgba16_pixel(im.out_ch, v, o);
                *reinterpret_cast<uint2 *>(x16 + im.x16_off + q * 8) = make_uint2((uint32_t)o[0] | ((uint32_t)o[1] << 16), (uint32_t)o[2] | ((uint32_t)o[3] << 16));
            }
            if (im.nat_off != rpht::NONE) {
                if (im.out_depth == 8) {
                    uint8_t *d = nat + im.nat_off + q * im.out_ch;
#pragma unroll
                    for (uint32_t c = 0; c < 4; c++)
                        if (c < im.out_ch) d[c] = (uint8_t)v[c];
                } else {
                    uint16_t *d = reinterpret_cast<uint16_t *>(nat + im.nat_off) + q * im.out_ch;
#pragma unroll
                    for (uint32_t c = 0; c < 4; c++)
                        if (c < im.out_ch) d[c] = (uint16_t)v[c];
                }
            }
        }
    }
}

}  // namespace

// segments [0, n) of one compression (5 or 32773) at d_segs
int rph_tiff_launch_decompress(uint32_t comp, const uint8_t *d_comp, const void *d_segs, uint32_t n, uint8_t *d_dec, int32_t *d_status, hipStream_t s)
{
    if (!n) return RPH_OK;
    if (comp == 5)
        hipLaunchKernelGGL(tiff_lzw_kernel, dim3(n), dim3(64), 0, s, d_comp, (const Segment *)d_segs, d_dec, d_status);
    else
        hipLaunchKernelGGL(tiff_packbits_kernel, dim3(n), dim3(64), 0, s, d_comp, (const Segment *)d_segs, d_dec, d_status);
    RPH_HIP_CHECK(hipGetLastError());
    return RPH_OK;
}

int rph_tiff_launch_expand(const uint8_t *d_comp, const uint8_t *d_dec, const void *d_images, const void *d_segs, const uint32_t *d_list, uint32_t n,
                           uint64_t max_pixels, uint8_t *d_hp, uint8_t *d_x16, uint8_t *d_nat, hipStream_t s)
{
    if (!n) return RPH_OK;
    const uint64_t blocks = (max_pixels + 1023) / 1024;
    const uint32_t gx = (uint32_t)(blocks < 256 ? (blocks ? blocks : 1) : 256);
    for (uint32_t first = 0; first < n; first += 65535) {
        const uint32_t m = n - first < 65535 ? n - first : 65535;
        hipLaunchKernelGGL(tiff_expand_kernel, dim3(gx, m), dim3(256), 0, s, d_comp, d_dec, (const Image *)d_images, (const Segment *)d_segs, d_list + first, d_hp, d_x16,
                           d_nat);
        RPH_HIP_CHECK(hipGetLastError());
    }
    return RPH_OK;
}
