// webp_kernels.hip -- the device half of the WebP path (webp_pipeline.cpp): VP8L entropy decoding, the inverse transforms, expand.
//
// entropy: one wave per stream, uniform control flow: every lane runs vp8l.h on the same bits.  The host has read the serial front of
//   the stream and built the groups' tables; the groups in use sit in LDS slots (32 KiB, direct-mapped by group number), filled from
//   the per-stream table in global memory by the whole wave when a block names a group its slot does not hold.  The colour cache lives in LDS as (position + 1) << 32 | argb
//   entered with a 64-bit maximum: the lanes of a copy enter their pixels at once and the last pixel of a slot still wins, as it does
//   in the serial order of the format.  Literals collect in a register (lane = position mod 64) and leave as one store of up to 64
//   pixels.  A backward reference is copied by the whole wave, 64 pixels per step; its sources lie in the image's own ARGB buffer in
//   global memory, possibly stored a few steps earlier by other lanes of this wave, so a copy first drains the wave's stores
//   (drain_stores: s_waitcnt vmcnt(0)).  The compressed bytes are read as aligned dwords, the next one loaded
//   ahead of its use (vp8l.h).
// inverse transforms: one launch per transform level, last read first.  Predictor: one wave per image over groups of 64 rows as a
//   skewed wavefront of two pixels per row: lane i holds row r0 + i and reconstructs pixel t - 2 i at step t; T, TL and TR come from
//   lane i - 1 by cross-lane moves (its last three results), L is the lane's own, lane 0 reads the row above from memory, 64 pixels
//   at a time, after the group before it has been stored.  Cross-colour, add-green: elementwise in place.  Colour indexing: unbundle
//   and look up into the image's second buffer, the palette in LDS.
// expand: ARGB words -> the hasher's Rgb8 / Rgba8 pixels and / or the native pixels.
// Every loop is bounded by the pixels still to produce (vp8l.h); the host has checked every size and built every table.
#include "rph_internal.h"
#include "webp_host.h"

namespace {

using rphw::Image;
using rphw::Xform;

constexpr uint32_t LDS_TABLE_U16 = 16384;  // 32 KiB of table slots: six groups without a colour cache, three with an 11-bit one
constexpr uint32_t MAX_SLOTS = 8;

// Every store this wave has issued is complete before anything behind this point is issued: s_waitcnt vmcnt(0) (gfx9 encoding: vmcnt
// 0, expcnt 7 and lgkmcnt 15 left alone), between two compiler fences so that no memory operation is moved across it.  Lanes of one
// wave then read what other lanes stored through the same CU's write-through L1.
__device__ __forceinline__ void drain_stores()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_waitcnt(0x0F70);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

struct DevPixelSink {
    uint32_t *out;
    unsigned long long *cache;  // LDS
    uint32_t shift, lane, has_cache;
    uint64_t n, flushed;
    uint32_t pend;
    uint16_t *slots;     // LDS: n_slots table slots of `stride` uint16, direct-mapped by group number
    uint32_t *tags;      // LDS: group held by each slot + 1, 0 = empty
    uint32_t n_slots;
    // the tables of the group a block names: from its LDS slot, filled from global memory by the whole wave when another group (or
    // none) holds it.  Consecutive pixels of an entropy block share a group, so this runs once per block the stream enters.
    __device__ __forceinline__ const uint16_t *group(const uint16_t *g, uint32_t id, uint32_t stride)
    {
        const uint32_t slot = id % n_slots;
        uint16_t *dst = slots + slot * stride;
        if (tags[slot] != id + 1) {
            const uint32_t *src = reinterpret_cast<const uint32_t *>(g);  // (strides and offsets are even)
            for (uint32_t k = lane; k < stride / 2; k += 64) reinterpret_cast<uint32_t *>(dst)[k] = src[k];
            if (lane == 0) tags[slot] = id + 1;
            __syncthreads();  // (one wave: orders the LDS writes before the look-ups for the compiler)
        }
        return dst;
    }
    __device__ __forceinline__ void enter(uint32_t v, uint64_t at)
    {
        if (has_cache) atomicMax(&cache[(v * rphw::CACHE_MUL) >> shift], ((unsigned long long)(at + 1) << 32) | v);
    }
    // the literals since the last flush lie in one aligned block of 64 positions
    __device__ __forceinline__ void flush()
    {
        const uint64_t at = (flushed & ~63ull) + lane;
        if (at >= flushed && at < n) out[at] = pend;
        flushed = n;
    }
    __device__ __forceinline__ void lit(uint32_t v)
    {
        if (lane == (uint32_t)(n & 63)) {
            pend = v;
            enter(v, n);
        }
        n++;
        if ((n & 63) == 0) flush();
    }
    // (LDS operations of one wave complete in order: the entries of earlier pixels, whichever lane made them, are in)
    __device__ __forceinline__ void cached(uint32_t key) { lit((uint32_t) * static_cast<volatile unsigned long long *>(cache + key)); }
    __device__ __forceinline__ void copy(uint32_t dist, uint32_t len)
    {
        flush();
        drain_stores();  // the sources may have been stored by other lanes a moment ago
        const uint64_t from = n - dist;
        for (uint32_t base = 0; base < len; base += 64) {
            const uint32_t i = base + lane;
            if (i < len) {
                // (every source lies below n: no step of a copy reads what an earlier step of it wrote)
                const uint32_t v = out[from + (dist >= len ? i : i % dist)];
                out[n + i] = v;
                enter(v, n + i);
            }
        }
        n += len;
        flushed = n;
    }
};

__global__ void __launch_bounds__(64) webp_entropy_kernel(const uint8_t *__restrict__ comp, const Image *__restrict__ imgs, const uint16_t *__restrict__ codes,
                                                          uint32_t *argb, int32_t *__restrict__ status)
{
    __shared__ unsigned long long cache[2048];
    __shared__ uint16_t tables[LDS_TABLE_U16];
    __shared__ uint32_t tags[MAX_SLOTS];
    const Image &im = imgs[blockIdx.x];
    const uint32_t lane = threadIdx.x, stride = rphw::group_stride(im.cache_bits);
    const uint32_t fit = LDS_TABLE_U16 / stride, n_slots = fit < MAX_SLOTS ? fit : MAX_SLOTS;
    if (lane < MAX_SLOTS) tags[lane] = 0;
    if (im.cache_bits)
        for (uint32_t k = lane; k < (1u << im.cache_bits); k += 64) cache[k] = 0;
    __syncthreads();
    const rphw::Stream s{im.xw, im.h, im.cache_bits, im.meta_bits, im.has_ent ? codes + im.ent_off : nullptr, codes + im.tab_off};
    rphw::Bits br;
    br.start(comp + im.comp_off, im.comp_len, im.bit_start);
    DevPixelSink sink{argb + im.a_off, cache, 32 - im.cache_bits, lane, im.cache_bits, 0, 0, 0, tables, tags, n_slots};
    const int rc = rphw::decode_pixels(s, br, sink);
    sink.flush();
    if (rc != rphw::W_OK && lane == 0) status[blockIdx.x] = RPH_ERR_INVALID_ARG;
}

// the `level`-th inverse transform (0 = the transform read last) of every listed image that has one
__global__ void __launch_bounds__(256) webp_inverse_kernel(const Image *__restrict__ imgs, const uint32_t *__restrict__ list, const uint32_t *__restrict__ words,
                                                           uint32_t *argb, uint32_t level)
{
    __shared__ uint32_t pal[256];
    const Image &im = imgs[list[blockIdx.y]];
    if (level >= im.n_tr) return;
    const Xform t = im.tr[im.n_tr - 1 - level];
    // an image sits in its second buffer once its colour indexing has been undone (it is read before the transforms undone later)
    bool in_b = false;
    for (uint32_t k = im.n_tr - level; k < im.n_tr; k++) in_b |= im.tr[k].type == rphw::TR_COLOUR_INDEXING;
    uint32_t *px = argb + (in_b ? im.b_off : im.a_off);
    const uint32_t *aux = words + t.off;
    const uint32_t w = t.xsize, h = im.h, bw = rphw::subsample(w, t.bits);
    const uint64_t total = (uint64_t)w * h, step = (uint64_t)gridDim.x * 256, first = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t.type == rphw::TR_SUBTRACT_GREEN) {
        for (uint64_t q = first; q < total; q += step) px[q] = rphw::add_green(px[q]);
    } else if (t.type == rphw::TR_CROSS_COLOUR) {
        for (uint64_t q = first; q < total; q += step) {
            const uint32_t y = (uint32_t)(q / w), x = (uint32_t)(q % w);
            px[q] = rphw::cross_colour(aux[(uint64_t)(y >> t.bits) * bw + (x >> t.bits)], px[q]);
        }
    } else if (t.type == rphw::TR_COLOUR_INDEXING) {
        pal[threadIdx.x] = aux[threadIdx.x];
        __syncthreads();
        uint32_t *dst = argb + im.b_off;
        for (uint64_t q = first; q < total; q += step) {
            const uint32_t y = (uint32_t)(q / w), x = (uint32_t)(q % w);
            dst[q] = pal[rphw::bundled_index(px[(uint64_t)y * bw + (x >> t.bits)], x, t.bits)];
        }
    } else {
        if (blockIdx.x != 0 || threadIdx.x >= 64) return;
        const uint32_t lane = threadIdx.x;
        for (uint32_t r0 = 0; r0 < h; r0 += 64) {
            // (rows r0 - 1 and above are final: stored by this wave in the group before)
            drain_stores();
            const uint32_t y = r0 + lane;
            const bool row_live = y < h;
            uint32_t *row = px + (uint64_t)(row_live ? y : 0) * w;
            const uint32_t *up0 = px + (uint64_t)(r0 ? r0 - 1 : 0) * w;  // lane 0's row above
            const uint32_t *mrow = aux + (uint64_t)((row_live ? y : 0) >> t.bits) * bw;
            uint32_t h1 = 0, h2 = 0, h3 = 0;  // the lane's last three results, junk included: what it made 1, 2 and 3 steps ago
            uint32_t own0 = 0;                // its pixel 0: TR of the last column is the next pixel in memory
            // lane 0's row above, 64 pixels at a time; u_tr, u_t, u_tl slide along it
            uint32_t above = (r0 && lane < w) ? up0[lane] : 0;
            uint32_t u_tr = __shfl(above, 0), u_t = 0, u_tl = 0;
            // the residuals of the next four steps through a register rotation (the generated loop still waits for all of them every step:
            // vmcnt counts the step's store with them, so about one step of work overlaps)
            auto residual = [&](int xq) -> uint32_t { return (row_live && xq >= 0 && xq < (int)w) ? row[xq] : 0; };
            uint32_t n0 = residual(-2 * (int)lane), n1 = residual(1 - 2 * (int)lane), n2 = residual(2 - 2 * (int)lane), n3 = residual(3 - 2 * (int)lane);
            // (and the mode words of their blocks, so that no step waits for a load it has just issued)
            auto mode_word = [&](int xq) -> uint32_t { return (row_live && xq >= 0 && xq < (int)w) ? mrow[(uint32_t)xq >> t.bits] : 0; };
            uint32_t m0 = mode_word(-2 * (int)lane), m1 = mode_word(1 - 2 * (int)lane), m2 = mode_word(2 - 2 * (int)lane), m3 = mode_word(3 - 2 * (int)lane);
            const uint32_t steps = w + 2 * 63;
            for (uint32_t t0 = 0; t0 < steps; t0++) {
                if (((t0 + 1) & 63) == 0) {
                    const uint32_t a = t0 + 1 + lane;
                    above = (r0 && a < w) ? up0[a] : 0;
                }
                u_tl = u_t;
                u_t = u_tr;
                u_tr = __shfl(above, (t0 + 1) & 63);
                const int xi = (int)t0 - 2 * (int)lane;
                const bool live = row_live && xi >= 0 && xi < (int)w;
                const uint32_t x = live ? (uint32_t)xi : 0;
                const uint32_t res = n0;
                n0 = n1, n1 = n2, n2 = n3;
                n3 = residual(xi + 4);
                const uint32_t mode = (m0 >> 8) & 15;
                m0 = m1, m1 = m2, m2 = m3;
                m3 = mode_word(xi + 4);
                // lane i - 1 works on pixel x + 2 of the row above: what it made 1, 2 and 3 steps ago are that row's x + 1, x, x - 1
                uint32_t TR = __shfl_up(h1, 1), T = __shfl_up(h2, 1), TL = __shfl_up(h3, 1);
                if (lane == 0) TR = u_tr, T = u_t, TL = u_tl;
                uint32_t p;
                if (y == 0)
                    p = x == 0 ? 0xff000000u : h1;
                else if (x == 0)
                    p = T;
                else
                    p = rphw::predict(mode, h1, T, TL, x + 1 < w ? TR : own0);
                const uint32_t v = rphw::add_pixels(res, p);
                if (live) row[x] = v;
                if (live && x == 0) own0 = v;
                h3 = h2;
                h2 = h1;
                h1 = v;
            }
        }
    }
}

__global__ void __launch_bounds__(256) webp_expand_kernel(const Image *__restrict__ imgs, const uint32_t *__restrict__ list, const uint32_t *__restrict__ argb,
                                                          uint8_t *__restrict__ hp, uint8_t *__restrict__ nat)
{
    const Image &im = imgs[list[blockIdx.y]];
    bool in_b = false;
    for (uint32_t k = 0; k < im.n_tr; k++) in_b |= im.tr[k].type == rphw::TR_COLOUR_INDEXING;
    const uint32_t *px = argb + (in_b ? im.b_off : im.a_off);
    const uint64_t total = (uint64_t)im.w * im.h;
    for (uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (uint64_t)gridDim.x * 256) {
        const uint32_t v = px[q];
        const uint8_t o[4] = {(uint8_t)(v >> 16), (uint8_t)(v >> 8), (uint8_t)v, (uint8_t)(v >> 24)};
        if (im.hp_off != rphw::NONE) {
            uint8_t *d = hp + im.hp_off + (q / im.w) * im.hstride + (q % im.w) * im.hc;
#pragma unroll
            for (uint32_t c = 0; c < 4; c++)
                if (c < im.hc) d[c] = o[c];
        }
        if (im.nat_off != rphw::NONE) {
            uint8_t *d = nat + im.nat_off + q * im.out_ch;
#pragma unroll
            for (uint32_t c = 0; c < 4; c++)
                if (c < im.out_ch) d[c] = o[c];
        }
    }
}

}  // namespace

// the main ARGB streams of images [0, n) at d_images, one wave each; a refused stream sets its image's status
int rph_webp_launch_entropy(const uint8_t *d_comp, const void *d_images, const void *d_codes, uint32_t n, uint32_t *d_argb, int32_t *d_status, hipStream_t s)
{
    if (!n) return RPH_OK;
    hipLaunchKernelGGL(webp_entropy_kernel, dim3(n), dim3(64), 0, s, d_comp, (const Image *)d_images, (const uint16_t *)d_codes, d_argb, d_status);
    RPH_HIP_CHECK(hipGetLastError());
    return RPH_OK;
}

// every inverse transform of the listed images (up to four levels), then their hasher and / or native pixels
int rph_webp_launch_finish(const void *d_images, const uint32_t *d_list, uint32_t n, uint32_t levels, uint64_t max_pixels, const uint32_t *d_words, uint32_t *d_argb,
                           uint8_t *d_hp, uint8_t *d_nat, hipStream_t s)
{
    if (!n) return RPH_OK;
    const uint64_t blocks = (max_pixels + 1023) / 1024;
    const uint32_t gx = (uint32_t)(blocks < 256 ? (blocks ? blocks : 1) : 256);
    for (uint32_t first = 0; first < n; first += 65535) {
        const uint32_t m = n - first < 65535 ? n - first : 65535;
        for (uint32_t level = 0; level < levels; level++) {
            hipLaunchKernelGGL(webp_inverse_kernel, dim3(gx, m), dim3(256), 0, s, (const Image *)d_images, d_list + first, d_words, d_argb, level);
            RPH_HIP_CHECK(hipGetLastError());
        }
        hipLaunchKernelGGL(webp_expand_kernel, dim3(gx, m), dim3(256), 0, s, (const Image *)d_images, d_list + first, (const uint32_t *)d_argb, d_hp, d_nat);
        RPH_HIP_CHECK(hipGetLastError());
    }
    return RPH_OK;
}
