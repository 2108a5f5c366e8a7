// png_kernels.hip -- the device half of the PNG path (png_pipeline.cpp): inflate, unfilter, expand.
//
// inflate: one wave per zlib stream.  Every lane runs the same decode (inflate.h) on the same bits, so control flow stays uniform;
//   the Huffman tables and a 32 KiB history ring live in LDS (37 KiB per wave, four waves per CU).  A copy is performed by the
//   whole wave, 64 bytes per step: byte i of a copy is out[pos - dist + (i % dist)], which lies before the copy's start, so an
//   overlapping copy (dist < len) needs no serialisation.  Every 4 KiB the ring is flushed to the image's raw buffer (16-byte
//   stores, the bytes past the image are not stored) and folded into the Adler-32 by a wave reduction.
// unfilter: one wave per Adam7 pass (or image), 64 rows at a time on a skewed wavefront: lane i holds row r0 + i and at step t
//   works on filter unit t - i; the unit above and the one above-left come from lane i - 1 through a shuffle.
// expand: one thread per pixel; writes the hasher's 8-bit pixels, the RGBA16 bytes of 16-bit images (pixel hash) and/or the
//   native pixels, by the rules of png_host.h.
#include "png_host.h"
#include "rph_internal.h"

namespace {

constexpr uint32_t WIN = 32768, FLUSH = 4096;

using rphp::StreamDesc;
using rphp::UnfilterJob;

struct DevSink {
    uint8_t *win;    // LDS ring
    uint8_t *out;    // global raw bytes of the image
    uint64_t cap, n, flushed;
    uint32_t s1, s2;
    uint32_t lane;

    __device__ uint64_t pos() const { return n; }

    // fold [flushed, flushed + m) into the Adler-32 and store what lies below cap; m <= FLUSH
    __device__ __forceinline__ void flush(uint32_t m)
    {
        __builtin_amdgcn_wave_barrier();
        const uint32_t b0 = lane * 64;
        uint32_t a = 0;
        uint64_t b = 0;  // sum of (m - b0 - j) * byte j over this lane's 64 bytes
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t o = b0 + 16 * q;
            uint32_t w4[4] = {0, 0, 0, 0};
            if (o + 16 <= m) {
                const uint4 v = *reinterpret_cast<const uint4 *>(win + ((flushed + o) & (WIN - 1)));
                w4[0] = v.x;
                w4[1] = v.y;
                w4[2] = v.z;
                w4[3] = v.w;
            } else {
#pragma unroll
                for (uint32_t j = 0; j < 16; j++)
                    if (o + j < m) w4[j >> 2] |= (uint32_t)win[(flushed + o + j) & (WIN - 1)] << (8 * (j & 3));
            }
            const uint64_t g = flushed + o;
            if (o + 16 <= m && g + 16 <= cap) {
                *reinterpret_cast<uint4 *>(out + g) = make_uint4(w4[0], w4[1], w4[2], w4[3]);
            } else if (o < m && g < cap) {
#pragma unroll
                for (uint32_t j = 0; j < 16; j++)
                    if (o + j < m && g + j < cap) out[g + j] = (uint8_t)(w4[j >> 2] >> (8 * (j & 3)));
            }
#pragma unroll
            for (uint32_t j = 0; j < 16; j++) {
                const uint32_t v = (w4[j >> 2] >> (8 * (j & 3))) & 0xFF;
                a += v;
                if (o + j < m) b += (uint64_t)(m - o - j) * v;
            }
        }
        uint32_t part = (uint32_t)(b % ADLER), asum = a;
        for (int off = 32; off > 0; off >>= 1) {
            asum += __shfl_xor(asum, off);
            part += __shfl_xor(part, off);
            part %= ADLER;
        }
        asum %= ADLER;
        s2 = (uint32_t)((s2 + (uint64_t)(m % ADLER) * s1 + part) % ADLER);
        s1 = (s1 + asum) % ADLER;
        flushed += m;
        __builtin_amdgcn_wave_barrier();
    }
    static constexpr uint32_t ADLER = rphz::ADLER_MOD;

    __device__ __forceinline__ void settle()
    {
        if (n - flushed >= FLUSH) flush(FLUSH);
    }
    __device__ __forceinline__ void lit(uint32_t b)
    {
        if (lane == 0) win[n & (WIN - 1)] = (uint8_t)b;
        n++;
        settle();
    }
    __device__ __forceinline__ void copy(uint32_t len, uint32_t dist)
    {
        for (uint32_t base = 0; base < len; base += 64) {
            const uint32_t i = base + lane;
            uint8_t v = 0;
            if (i < len) v = win[(n - dist + (dist >= len ? i : i % dist)) & (WIN - 1)];
            __builtin_amdgcn_wave_barrier();
            if (i < len) win[(n + i) & (WIN - 1)] = v;
            __builtin_amdgcn_wave_barrier();
        }
        n += len;
        settle();
    }
    __device__ __forceinline__ void stored(const uint8_t *p, uint32_t len)
    {
        for (uint32_t base = 0; base < len; base += 64) {
            const uint32_t i = base + lane;
            if (i < len) win[(n + lane) & (WIN - 1)] = p[i];  // (n has advanced by base already)
            __builtin_amdgcn_wave_barrier();
            const uint32_t m = len - base < 64 ? len - base : 64;
            n += m;
            settle();
        }
    }
    __device__ __forceinline__ uint32_t adler()
    {
        if (n > flushed) flush((uint32_t)(n - flushed));
        return (s2 << 16) | s1;
    }
};

__global__ void __launch_bounds__(64) png_inflate_kernel(const uint8_t *__restrict__ comp, const StreamDesc *__restrict__ sd,
                                                         uint8_t *__restrict__ raw, int32_t *__restrict__ status)
{
    __shared__ __attribute__((aligned(16))) uint8_t win[WIN];
    __shared__ rphz::Tables tables;
    const StreamDesc d = sd[blockIdx.x];
    DevSink s;
    s.win = win;
    s.out = raw + d.raw_off;
    s.cap = d.raw_bytes;
    s.n = s.flushed = 0;
    s.s1 = 1;
    s.s2 = 0;
    s.lane = threadIdx.x;
    int rc = rphz::inflate_zlib(comp + d.comp_off, d.comp_len, tables, s);
    if (rc == rphz::Z_OK && s.n < d.raw_bytes) rc = rphz::Z_SHORT;
    if (rc != rphz::Z_OK && threadIdx.x == 0) status[d.image] = RPH_ERR_INVALID_ARG;
}


// unit <= 8 bytes, packed in two dwords
__global__ void __launch_bounds__(64) png_unfilter_kernel(uint8_t *__restrict__ raw, const UnfilterJob *__restrict__ jobs, int32_t *__restrict__ status)
{
    const UnfilterJob J = jobs[blockIdx.x];
    if (status[J.image] != RPH_OK) return;
    const uint32_t lane = threadIdx.x, u = J.unit, nu = J.rowbytes / u + (J.rowbytes % u ? 1 : 0);
    const uint64_t stride = 1 + (uint64_t)J.rowbytes;
    bool bad = false;
    for (uint32_t r0 = 0; r0 < J.rows; r0 += 64) {
        const uint32_t r = r0 + lane;
        const bool live = r < J.rows;
        uint8_t *row = raw + J.off + (uint64_t)r * stride;
        const uint32_t f = live ? row[0] : 0;
        if (f > 4) bad = true;
        const uint8_t *above0 = r0 ? raw + J.off + (uint64_t)(r0 - 1) * stride + 1 : nullptr;  // lane 0's row above: final since the last group
        uint32_t left_lo = 0, left_hi = 0, ul_lo = 0, ul_hi = 0;  // this lane's unit to the left, and the unit above-left (8 bytes in two dwords)
        uint32_t cur_lo = 0, cur_hi = 0;                             // this lane's unit of the previous step
        const uint32_t span = (J.rows - r0 < 64 ? J.rows - r0 : 64);
        for (uint32_t t = 0; t < nu + span - 1; t++) {
            // the unit above = lane i-1's result of the previous step (lane 0: the last row of the previous group, from memory)
            uint32_t up_lo = __shfl_up(cur_lo, 1), up_hi = __shfl_up(cur_hi, 1);
            const int32_t k = (int32_t)t - (int32_t)lane;
            if (live && k >= 0 && (uint32_t)k < nu) {
                if (lane == 0) {
                    up_lo = up_hi = 0;
                    if (above0) {
#pragma unroll
                        for (uint32_t j = 0; j < 8; j++) {
                            const uint32_t b = k * u + j;
                            const uint32_t v = (j < u && b < J.rowbytes) ? above0[b] : 0;
                            if (j < 4) up_lo |= v << (8 * j);
                            else up_hi |= v << (8 * (j - 4));
                        }
                    }
                }
                if (k == 0) left_lo = left_hi = ul_lo = ul_hi = 0;
                uint32_t lo = 0, hi = 0;
#pragma unroll
                for (uint32_t j = 0; j < 8; j++) {
                    const uint32_t b = k * u + j;
                    const uint32_t sh = 8 * (j & 3);
                    const uint8_t a = (uint8_t)(((j < 4) ? left_lo : left_hi) >> sh), bv = (uint8_t)(((j < 4) ? up_lo : up_hi) >> sh),
                                  c = (uint8_t)(((j < 4) ? ul_lo : ul_hi) >> sh);
                    uint32_t v = 0;
                    if (j < u && b < J.rowbytes) {
                        v = rphp::unfilter_byte(f, row[1 + b], a, bv, c);
                        row[1 + b] = (uint8_t)v;
                    }
                    if (j < 4) lo |= v << sh;
                    else hi |= v << sh;
                }
                left_lo = cur_lo = lo;
                left_hi = cur_hi = hi;
                ul_lo = up_lo;
                ul_hi = up_hi;
            }
        }
        __syncthreads();  // the group's last row is read by lane 0 of the next group
    }
    if (bad) status[J.image] = RPH_ERR_INVALID_ARG;
}

__global__ void __launch_bounds__(256) png_expand_kernel(const uint8_t *__restrict__ raw, const rphp::Image *__restrict__ imgs, const uint32_t *__restrict__ list,
                                                         const uint8_t *__restrict__ pal, uint8_t *__restrict__ hp, uint8_t *__restrict__ x16,
                                                         uint8_t *__restrict__ nat)
{
    __shared__ uint8_t lp[1024];
    const rphp::Image &im = imgs[list[blockIdx.y]];  // (read from memory: the pass arrays are indexed by pixel)
    if (im.ctype == 3) {
        for (uint32_t i = threadIdx.x; i < 1024; i += blockDim.x) lp[i] = pal[(size_t)im.pal * 1024 + i];
        __syncthreads();
    }
    const uint64_t npx = (uint64_t)im.w * im.h;
    const uint8_t *r = raw + im.raw_off;
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < npx; q += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t y = (uint32_t)(q / im.w), x = (uint32_t)(q % im.w);
        uint32_t v[4] = {0, 0, 0, 0};
        rphp::pixel(im, r, lp, x, y, v);
        if (im.hp_off != rphp::NONE) {
            uint8_t o[4];
            rphp::hasher_pixel(im, v, o);
            uint8_t *d = hp + im.hp_off + (uint64_t)y * im.hstride + (uint64_t)x * im.hc;
#pragma unroll
            for (uint32_t c = 0; c < 4; c++)
                if (c < im.hc) d[c] = o[c];
        }
        if (im.x16_off != rphp::NONE) {
            uint16_t o[4];
            rphp::rgba16_pixel(im, v, o);
            uint2 pk = make_uint2((uint32_t)o[0] | ((uint32_t)o[1] << 16), (uint32_t)o[2] | ((uint32_t)o[3] << 16));
            *reinterpret_cast<uint2 *>(x16 + im.x16_off + q * 8) = pk;
        }
        if (im.nat_off != rphp::NONE) {
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

}  // namespace

int rph_png_launch_inflate(const uint8_t *d_comp, const void *d_streams, uint32_t n, uint8_t *d_raw, int32_t *d_status, hipStream_t s)
{
    if (!n) return RPH_OK;
    hipLaunchKernelGGL(png_inflate_kernel, dim3(n), dim3(64), 0, s, d_comp, (const StreamDesc *)d_streams, d_raw, d_status);
    RPH_HIP_CHECK(hipGetLastError());
    return RPH_OK;
}

int rph_png_launch_unfilter(uint8_t *d_raw, const void *d_jobs, uint32_t n_jobs, int32_t *d_status, hipStream_t s)
{
    if (!n_jobs) return RPH_OK;
    hipLaunchKernelGGL(png_unfilter_kernel, dim3(n_jobs), dim3(64), 0, s, d_raw, (const UnfilterJob *)d_jobs, d_status);
    RPH_HIP_CHECK(hipGetLastError());
    return RPH_OK;
}

int rph_png_launch_expand(const uint8_t *d_raw, const void *d_images, const uint32_t *d_list, uint32_t n, uint64_t max_pixels, const uint8_t *d_pal,
                          uint8_t *d_hp, uint8_t *d_x16, uint8_t *d_nat, hipStream_t s)
{
    if (!n) return RPH_OK;
    const uint64_t blocks = (max_pixels + 255) / 256;
    const uint32_t gx = (uint32_t)(blocks < 256 ? (blocks ? blocks : 1) : 256);
    for (uint32_t first = 0; first < n; first += 65535) {
        const uint32_t m = n - first < 65535 ? n - first : 65535;
        hipLaunchKernelGGL(png_expand_kernel, dim3(gx, m), dim3(256), 0, s, d_raw, (const rphp::Image *)d_images, d_list + first, d_pal, d_hp, d_x16, d_nat);
        RPH_HIP_CHECK(hipGetLastError());
    }
    return RPH_OK;
}

