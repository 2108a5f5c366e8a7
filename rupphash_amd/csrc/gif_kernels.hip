// gif_kernels.hip -- the device half of the GIF path (gif_pipeline.cpp): LZW, expand.
//
// lzw: one wave per file, uniform control flow: every lane runs gif_lzw.h on the same bits of the joined stream (the host has taken the
//   sub-blocks apart while staging).  The string table (position in the frame's indices, length: 24 KiB) lives in LDS.  A code is one
//   copy of indices the frame already holds, 64 bytes per step (wave_sink.h).  A frame of up to 16 KiB (icons, buttons) is built in LDS
//   and stored with 16-byte stores at the end; a larger one is built in global memory, where every copy waits for the stores before it.
//   40 KiB of LDS per wave, four waves per CU.  The bit reader loads dwords.
// expand: one wave per row of the logical screen, 64 pixels per step, one pass: the row of the frame under the pixel (interlaced rows
//   lie in pass order), the palette in force, the frame's offset and the clipping to the screen, alpha (gif_host.h, screen_pixel);
//   writes the hasher's Rgba8 pixels and / or the native pixels, one dword per pixel.
// The LZW loop is bounded by the stream's bits and the frame's bytes (gif_lzw.h), and the host has checked every offset and size.
#include "gif_host.h"
#include "rph_internal.h"
#include "wave_sink.h"

namespace {

using rphg::Image;

constexpr uint32_t LDS_FRAME = 16384;

__global__ void __launch_bounds__(64) gif_lzw_kernel(const uint8_t *__restrict__ comp, const Image *__restrict__ imgs, uint8_t *dec, int32_t *__restrict__ status)
{
    __shared__ rphg::LzwTable table;
    __shared__ __attribute__((aligned(16))) uint8_t frame[LDS_FRAME];
    const Image &im = imgs[blockIdx.x];
    const uint64_t bytes = (uint64_t)im.fw * im.fh, dec_off = im.dec_off;
    const bool in_lds = bytes <= LDS_FRAME;
    WaveSink s{in_lds ? frame : dec + dec_off, bytes, 0, threadIdx.x};
    const int rc = rphg::lzw_decode(comp + im.comp_off, im.comp_len, im.m, table, s);
    if (rc != rphg::L_OK) {
        if (threadIdx.x == 0) status[blockIdx.x] = RPH_ERR_INVALID_ARG;
        return;
    }
    if (in_lds) {
        __syncthreads();
        // (the slot is a multiple of 16 bytes and 16-byte aligned: the last store may carry bytes past the frame, inside the slot)
        for (uint32_t o = threadIdx.x * 16; o < bytes; o += 64 * 16) *reinterpret_cast<uint4 *>(dec + dec_off + o) = *reinterpret_cast<const uint4 *>(frame + o);
    }
}

__global__ void __launch_bounds__(256) gif_expand_kernel(const uint8_t *__restrict__ dec, const Image *__restrict__ imgs, const uint32_t *__restrict__ pals,
                                                         const uint32_t *__restrict__ list, uint8_t *__restrict__ hp, uint8_t *__restrict__ nat)
{
    const Image im = imgs[list[blockIdx.y]];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t *pal = pals + im.pal_off;
    const uint8_t *idx = dec + im.dec_off;
    for (uint32_t y = blockIdx.x * 4 + wave; y < im.h; y += gridDim.x * 4) {
        for (uint32_t x = lane; x < im.w; x += 64) {
            const uint32_t v = rphg::screen_pixel(im, pal, idx, x, y);
            if (im.hp_off != rphg::NONE) *reinterpret_cast<uint32_t *>(hp + im.hp_off + (uint64_t)y * im.hstride + (uint64_t)x * 4) = v;
            if (im.nat_off != rphg::NONE) *reinterpret_cast<uint32_t *>(nat + im.nat_off + ((uint64_t)y * im.w + x) * 4) = v;
        }
    }
}

}  // namespace

// one wave per image of d_images[0 .. n)
int rph_gif_launch_lzw(const uint8_t *d_comp, const void *d_images, uint32_t n, uint8_t *d_dec, int32_t *d_status, hipStream_t s)
{
    if (!n) return RPH_OK;
    hipLaunchKernelGGL(gif_lzw_kernel, dim3(n), dim3(64), 0, s, d_comp, (const Image *)d_images, d_dec, d_status);
    RPH_HIP_CHECK(hipGetLastError());
    return RPH_OK;
}

int rph_gif_launch_expand(const uint8_t *d_dec, const void *d_images, const uint32_t *d_pals, const uint32_t *d_list, uint32_t n, uint32_t max_rows,
                          uint8_t *d_hp, uint8_t *d_nat, hipStream_t s)
{
    if (!n) return RPH_OK;
    const uint32_t blocks = (max_rows + 3) / 4;
    const uint32_t gx = blocks < 256 ? (blocks ? blocks : 1) : 256;
    for (uint32_t first = 0; first < n; first += 65535) {
        const uint32_t m = n - first < 65535 ? n - first : 65535;
        hipLaunchKernelGGL(gif_expand_kernel, dim3(gx, m), dim3(256), 0, s, d_dec, (const Image *)d_images, d_pals, d_list + first, d_hp, d_nat);
        RPH_HIP_CHECK(hipGetLastError());
    }
    return RPH_OK;
}
