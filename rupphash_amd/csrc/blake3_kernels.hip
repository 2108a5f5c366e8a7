// blake3_kernels.hip -- BLAKE3 (hash / keyed_hash, 32-byte output) of byte strings and the pixel hash of decoded images
// (phdupes --pixel-hash: blake3::hash of to_rgba16() as little-endian bytes, reference scanner.rs:1393-1404), plus the C entry points.
//
// Layout: one lane per 1 KiB chunk.  A wave takes 64 consecutive chunks of one input (a "group"); each lane runs the 16 block
// compressions of its chunk in registers, then the wave folds its 64 chaining values across lanes into the value of the 64 KiB
// subtree (every 2^k-aligned run of chunks that lies fully inside the input and is not the whole input is a complete subtree of the
// BLAKE3 tree).  An input of more than one group leaves one value per group behind, and a second kernel folds those per input,
// pairwise, carrying an odd last node up a level: the same tree as BLAKE3's left-full one.  The last compression carries ROOT; for
// an input of one chunk that is the chunk's last block, for one group the wave's last fold.
//
// Pixel hash: one chunk is exactly 128 pixels of RGBA16 in raster order (8 bytes per pixel `r r g g b b a a`: each u8 sample v
// becomes the u16 v * 257, Luma8 is copied into R, G and B, alpha is 65535 unless the input is Rgba8).  The two message words of
// a pixel are built in registers from the u8 samples; the RGBA16 stream is never written anywhere.  PARITY: the v * 257 widening
// is the `image` crate's u8 -> u16 conversion as published (to_rgba16 of an 8-bit DynamicImage); the crate's source is not part of
// the reference tree, so agreement with the Rust binary's digest rests on that mapping.
// b3_pixels_ragged_kernel is the same for images of any mix of sizes and of the eight layouts of rph_image_hash_ragged (u8 or u16 samples,
// 1 to 4 channels): a wave finds its image in a prefix table of groups and takes its geometry and layout from a descriptor.
#include <algorithm>
#include <cstring>
#include <vector>

#include "blake3.h"
#include "rph_internal.h"

namespace {

constexpr uint32_t GROUP_CHUNKS = 64;               // chunks per wave
constexpr uint64_t GROUP_BYTES = 64 * 1024;          // bytes per group of a byte string
constexpr uint32_t PX_PER_CHUNK = B3_CHUNK_LEN / 8;  // RGBA16 pixels per chunk

struct Key {
    uint32_t w[8];
};

__device__ __forceinline__ uint32_t funnel(uint32_t lo, uint32_t hi, uint32_t sh)  // bytes sh .. sh+3 of {hi, lo}
{
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * sh));
}

// The wave's 64 chunk values (node i in lane i, `cnt` of them) folded pairwise into one, carrying an odd last node up a level.
// `root`: the group is the whole input, so its last fold is the root.  The result is in lane 0.
__device__ __forceinline__ void wave_fold(uint32_t cv[8], uint32_t cnt, bool root, const Key &key, uint32_t flags)
{
    const uint32_t lane = threadIdx.x & 63;
    while (cnt > 1) {
        uint32_t l[8], r[8];
        const int sl = (int)min(2 * lane, 63u), sr = (int)min(2 * lane + 1, 63u);
#pragma unroll
        for (int i = 0; i < 8; i++) l[i] = __shfl(cv[i], sl), r[i] = __shfl(cv[i], sr);
        uint32_t p[8];
        b3_parent(key.w, l, r, flags | ((root && cnt == 2) ? B3_ROOT : 0u), p);
        const bool pair = 2 * lane + 1 < cnt;
#pragma unroll
        for (int i = 0; i < 8; i++) cv[i] = pair ? p[i] : l[i];
        cnt = (cnt + 1) / 2;
    }
}

// the 16 words of one full 64-byte block at any byte address: aligned dword loads, realigned in registers
__device__ __forceinline__ void load_block(const uint8_t *p, uint32_t m[16])
{
    const uint32_t sh = (uint32_t)((uintptr_t)p & 3);
    const uint32_t *q = reinterpret_cast<const uint32_t *>(p - sh);
    uint32_t d[17];
#pragma unroll
    for (int i = 0; i < 16; i++) d[i] = q[i];
    d[16] = sh ? q[16] : 0u;  // only when the block's last byte lies in it
#pragma unroll
    for (int i = 0; i < 16; i++) m[i] = funnel(d[i], d[i + 1], sh);
}

// -------- byte strings --------

// group_first[s] = first group of string s (exclusive prefix of max(1, ceil(len / 64 KiB))), group_first[n] = total.  One block.
__global__ void __launch_bounds__(1024) b3_plan_kernel(const uint64_t *__restrict__ off, uint32_t n, uint32_t *__restrict__ group_first)
{
    __shared__ uint32_t wave_total[16];
    const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6, per = (n + 1023) / 1024, s0 = min(n, t * per), s1 = min(n, s0 + per);
    auto groups = [&](uint32_t s) -> uint32_t {
        const uint64_t a = off[s], b = off[s + 1], len = b > a ? b - a : 0;
        return len ? (uint32_t)((len + GROUP_BYTES - 1) / GROUP_BYTES) : 1u;
    };
    uint32_t sum = 0;
    for (uint32_t s = s0; s < s1; s++) sum += groups(s);
    uint32_t x = sum;  // inclusive scan of the threads' sums: across the lanes of a wave, then over the 16 wave totals
#pragma unroll
    for (int d = 1; d < 64; d *= 2) {
        const uint32_t y = __shfl_up(x, d);
        if (lane >= (uint32_t)d) x += y;
    }
    if (lane == 63) wave_total[wv] = x;
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t w = 0; w < wv; w++) before += wave_total[w];
    uint32_t acc = before + x - sum;
    for (uint32_t s = s0; s < s1; s++) group_first[s] = acc, acc += groups(s);
    if (t == 1023) group_first[n] = before + x;
}

// One wave per group (grid-stride over all groups of the call).  Groups past `cap` (scratch capacity) are skipped.
__global__ void __launch_bounds__(256) b3_bytes_kernel(const uint8_t *__restrict__ data, const uint64_t *__restrict__ off, uint32_t n,
                                                       const uint32_t *__restrict__ group_first, uint32_t cap, Key key, uint32_t flags,
                                                       uint32_t *__restrict__ cvs, uint8_t *__restrict__ digest)
{
    const uint32_t lane = threadIdx.x & 63, total = min(group_first[n], cap);
    const uint32_t waves = gridDim.x * (blockDim.x / 64);
    for (uint32_t g = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64; g < total; g += waves) {
        uint32_t lo = 0, hi = n;  // the string s with group_first[s] <= g < group_first[s + 1]
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) / 2;
            if (group_first[mid] <= g) lo = mid;
            else hi = mid;
        }
        const uint32_t s = lo, k = g - group_first[s];
        const uint64_t a = off[s], b = off[s + 1], len = b > a ? b - a : 0;
        const uint64_t nchunks = len ? (len + B3_CHUNK_LEN - 1) / B3_CHUNK_LEN : 1;
        const uint64_t c0 = (uint64_t)k * GROUP_CHUNKS;
        const uint32_t in_group = (uint32_t)min<uint64_t>(GROUP_CHUNKS, nchunks - c0);
        const uint64_t c = c0 + lane;
        uint32_t cv[8];
#pragma unroll
        for (int i = 0; i < 8; i++) cv[i] = key.w[i];
        if (lane < in_group) {
            const uint8_t *p = data + a + c * B3_CHUNK_LEN;
            const uint32_t clen = (uint32_t)min<uint64_t>(B3_CHUNK_LEN, len - min(len, c * B3_CHUNK_LEN));
            const uint32_t nb = clen ? (clen + B3_BLOCK_LEN - 1) / B3_BLOCK_LEN : 1;
            for (uint32_t bk = 0; bk < nb; bk++) {
                const uint32_t blen = min(B3_BLOCK_LEN, clen - bk * B3_BLOCK_LEN);
                uint32_t m[16];
                if (blen == B3_BLOCK_LEN) {
                    load_block(p + bk * B3_BLOCK_LEN, m);
                } else {  // the chunk's last, partial block, zero padded (constant word indices: no register indexing)
                    const uint8_t *q = p + bk * B3_BLOCK_LEN;
#pragma unroll
                    for (int i = 0; i < 16; i++) {
                        uint32_t w = 0;
#pragma unroll
                        for (int b = 0; b < 4; b++)
                            if ((uint32_t)(4 * i + b) < blen) w |= (uint32_t)q[4 * i + b] << (8 * b);
                        m[i] = w;
                    }
                }
                const uint32_t fl = flags | (bk == 0 ? B3_CHUNK_START : 0u) | (bk + 1 == nb ? B3_CHUNK_END : 0u) |
                                    ((bk + 1 == nb && nchunks == 1) ? B3_ROOT : 0u);
                b3_compress(cv, m, c, blen, fl, cv);
            }
        }
        const bool whole = nchunks <= GROUP_CHUNKS;
        wave_fold(cv, in_group, whole, key, flags);
        uint32_t v = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const uint32_t x = __shfl(cv[i], 0);  // the folded value is lane 0's: word i goes out from lane i
            v = lane == (uint32_t)i ? x : v;
        }
        if (lane < 8) {
            if (whole) reinterpret_cast<uint32_t *>(digest + (size_t)s * 32)[lane] = v;
            else cvs[(size_t)g * 8 + lane] = v;
        }
    }
}

// One wave per input with more than one group: its group values (level 6 of the tree, in cvs from group_first[s] or s * per_input)
// folded in place level by level; the last fold carries ROOT and goes to the digest.  The in-place levels go through L2 (agent-scope
// loads and stores, a fence between levels).
__global__ void __launch_bounds__(64) b3_fold_kernel(const uint32_t *__restrict__ group_first, uint32_t per_input, uint32_t cap, Key key, uint32_t flags,
                                                     uint32_t *cvs, uint8_t *__restrict__ digest)
{
    const uint32_t s = blockIdx.x, lane = threadIdx.x;
    const uint32_t g0 = group_first ? group_first[s] : s * per_input;
    uint32_t cnt = group_first ? group_first[s + 1] - g0 : per_input;
    if (cnt <= 1 || g0 + cnt > cap) return;
    uint32_t *nodes = cvs + (size_t)g0 * 8;
    while (cnt > 1) {
        const uint32_t next = (cnt + 1) / 2;
        for (uint32_t i = lane; i < next; i += 64) {
            uint32_t l[8], r[8], p[8];
#pragma unroll
            for (int q = 0; q < 8; q++) l[q] = __hip_atomic_load(nodes + (size_t)2 * i * 8 + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (2 * i + 1 < cnt) {
#pragma unroll
                for (int q = 0; q < 8; q++) r[q] = __hip_atomic_load(nodes + (size_t)(2 * i + 1) * 8 + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                b3_parent(key.w, l, r, flags | (next == 1 ? B3_ROOT : 0u), p);
            } else {
#pragma unroll
                for (int q = 0; q < 8; q++) p[q] = l[q];
            }
            if (next == 1) {
#pragma unroll
                for (int q = 0; q < 8; q++) reinterpret_cast<uint32_t *>(digest + (size_t)s * 32)[q] = p[q];
            } else {
#pragma unroll
                for (int q = 0; q < 8; q++) __hip_atomic_store(nodes + (size_t)i * 8 + q, p[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        __threadfence();
        __syncthreads();
        cnt = next;
    }
}

// -------- pixel hash --------

// the two RGBA16 message words of one pixel from its u8 samples
template <int CH>
__device__ __forceinline__ void px_words(uint32_t r, uint32_t g, uint32_t b, uint32_t a, uint32_t &w0, uint32_t &w1)
{
    if (CH == 1) {
        w0 = r * 0x01010101u;
        w1 = (r * 0x101u) | 0xFFFF0000u;
    } else if (CH == 3) {
        w0 = (r | (g << 16)) * 0x101u;
        w1 = (b * 0x101u) | 0xFFFF0000u;
    } else {
        w0 = (r | (g << 16)) * 0x101u;
        w1 = (b | (a << 16)) * 0x101u;
    }
}

// One wave per 64 chunks (8192 pixels) of one image: grid = n images x groups_per_image waves.
template <int CH>
__global__ void __launch_bounds__(256) b3_pixels_kernel(const uint8_t *__restrict__ px, uint32_t n, uint32_t w, uint32_t h, size_t row_stride,
                                                        size_t image_stride, uint32_t groups_per_image, uint32_t *__restrict__ cvs,
                                                        uint8_t *__restrict__ digest)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t g = (uint64_t)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
    if (g >= (uint64_t)n * groups_per_image) return;
    const uint32_t img = (uint32_t)(g / groups_per_image), k = (uint32_t)(g - (uint64_t)img * groups_per_image);
    const uint64_t npx = (uint64_t)w * h;
    const uint64_t nchunks = npx ? (npx + PX_PER_CHUNK - 1) / PX_PER_CHUNK : 1;
    const uint64_t c0 = (uint64_t)k * GROUP_CHUNKS, c = c0 + lane;
    const uint32_t in_group = (uint32_t)min<uint64_t>(GROUP_CHUNKS, nchunks - c0);
    Key iv;
#pragma unroll
    for (int i = 0; i < 8; i++) iv.w[i] = b3_iv(i);
    uint32_t cv[8];
#pragma unroll
    for (int i = 0; i < 8; i++) cv[i] = iv.w[i];
    if (lane < in_group) {
        const uint64_t p0 = c * PX_PER_CHUNK;
        const uint32_t cpx = (uint32_t)min<uint64_t>(PX_PER_CHUNK, npx - min(npx, p0));  // pixels of this chunk
        const uint32_t nb = cpx ? (cpx + 7) / 8 : 1;
        uint32_t y = w ? (uint32_t)(p0 / w) : 0, x = w ? (uint32_t)(p0 - (uint64_t)y * w) : 0;
        const uint8_t *row = px + (size_t)img * image_stride + (size_t)y * row_stride;
        for (uint32_t bk = 0; bk < nb; bk++) {
            const uint32_t bpx = min(8u, cpx - min(cpx, bk * 8));
            uint32_t m[16];
            if (bpx == 8 && x + 8 <= w) {  // 8 pixels of one row: 8 * CH bytes through aligned dwords, realigned in registers
                const uint8_t *p = row + (size_t)x * CH;
                const uint32_t sh = (uint32_t)((uintptr_t)p & 3);
                const uint32_t *q = reinterpret_cast<const uint32_t *>(p - sh);
                constexpr int ND = 2 * CH;  // dwords of the 8 pixels
                uint32_t d[ND + 1], u[ND];
#pragma unroll
                for (int i = 0; i < ND; i++) d[i] = q[i];
                d[ND] = sh ? q[ND] : 0u;
#pragma unroll
                for (int i = 0; i < ND; i++) u[i] = funnel(d[i], d[i + 1], sh);
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    auto byte = [&](int j) -> uint32_t { return (u[j >> 2] >> (8 * (j & 3))) & 0xFFu; };
                    const uint32_t r = byte(i * CH), gg = CH >= 3 ? byte(i * CH + 1) : r, bb = CH >= 3 ? byte(i * CH + 2) : r,
                                   aa = CH == 4 ? byte(i * CH + 3) : 255u;
                    px_words<CH>(r, gg, bb, aa, m[2 * i], m[2 * i + 1]);
                }
                x += 8;
                if (x == w) x = 0, row += row_stride;
            } else {  // a block that crosses a row end (or the image's last, partial block): pixel by pixel
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    m[2 * i] = m[2 * i + 1] = 0;
                    if ((uint32_t)i < bpx) {
                        const uint8_t *p = row + (size_t)x * CH;
                        const uint32_t r = p[0], gg = CH >= 3 ? p[1] : r, bb = CH >= 3 ? p[2] : r, aa = CH == 4 ? p[3] : 255u;
                        px_words<CH>(r, gg, bb, aa, m[2 * i], m[2 * i + 1]);
                        if (++x == w) x = 0, row += row_stride;
                    }
                }
            }
            const uint32_t fl = (bk == 0 ? B3_CHUNK_START : 0u) | (bk + 1 == nb ? B3_CHUNK_END : 0u) | ((bk + 1 == nb && nchunks == 1) ? B3_ROOT : 0u);
            b3_compress(cv, m, c, bpx * 8, fl, cv);
        }
    }
    const bool whole = nchunks <= GROUP_CHUNKS;
    wave_fold(cv, in_group, whole, iv, 0);
    uint32_t v = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint32_t x = __shfl(cv[i], 0);  // the folded value is lane 0's: word i goes out from lane i
        v = lane == (uint32_t)i ? x : v;
    }
    if (lane < 8) {
        if (whole) reinterpret_cast<uint32_t *>(digest + (size_t)img * 32)[lane] = v;
        else cvs[g * 8 + lane] = v;
    }
}

// -------- pixel hash, a geometry and a layout per image --------

// the two RGBA16 message words of one pixel of layout L (RPH_LAYOUT_*: channels + 16 for u16 samples) from its samples s[0 .. channels):
// u8 samples widen as v * 257, u16 samples stay, gray goes into R, G and B, a missing alpha is 65535
template <int L>
__device__ __forceinline__ void layout_words(const uint32_t s[4], uint32_t &w0, uint32_t &w1)
{
    constexpr int CH = L & 15;
    constexpr bool WIDE = L > 16;
    const uint32_t r = s[0], g = CH >= 3 ? s[1] : r, b = CH >= 3 ? s[2] : r, a = CH == 2 ? s[1] : CH == 4 ? s[3] : (WIDE ? 0xFFFFu : 0xFFu);
    w0 = (r | (g << 16)) * (WIDE ? 1u : 0x101u);
    w1 = (b | (a << 16)) * (WIDE ? 1u : 0x101u);
}

// The chaining value of chunk c (128 pixels from pixel c * 128) of one image of layout L: the chunk loop of b3_pixels_kernel with the
// sample width and count of the layout.  16-bit images lie at even addresses with even row strides (checked by the entry points).
template <int L>
__device__ __forceinline__ void layout_chunk(const uint8_t *__restrict__ img, uint32_t w, size_t row_stride, uint64_t npx, uint64_t nchunks, uint64_t c, uint32_t cv[8])
{
    constexpr int CH = L & 15, BPS = L > 16 ? 2 : 1, BPP = CH * BPS;
    const uint64_t p0 = c * PX_PER_CHUNK;
    const uint32_t cpx = (uint32_t)min<uint64_t>(PX_PER_CHUNK, npx - min(npx, p0));  // pixels of this chunk
    const uint32_t nb = cpx ? (cpx + 7) / 8 : 1;
    uint32_t y = w ? (uint32_t)(p0 / w) : 0, x = w ? (uint32_t)(p0 - (uint64_t)y * w) : 0;
    const uint8_t *row = img + (size_t)y * row_stride;
    for (uint32_t bk = 0; bk < nb; bk++) {
        const uint32_t bpx = min(8u, cpx - min(cpx, bk * 8));
        uint32_t m[16];
        if (bpx == 8 && x + 8 <= w) {  // 8 pixels of one row: 8 * BPP bytes through aligned dwords, realigned in registers
            const uint8_t *p = row + (size_t)x * BPP;
            const uint32_t sh = (uint32_t)((uintptr_t)p & 3);
            const uint32_t *q = reinterpret_cast<const uint32_t *>(p - sh);
            constexpr int ND = 2 * BPP;  // dwords of the 8 pixels
            uint32_t d[ND + 1], u[ND];
#pragma unroll
            for (int i = 0; i < ND; i++) d[i] = q[i];
            d[ND] = sh ? q[ND] : 0u;  // only when the block's last byte lies in it
#pragma unroll
            for (int i = 0; i < ND; i++) u[i] = funnel(d[i], d[i + 1], sh);
#pragma unroll
            for (int i = 0; i < 8; i++) {
                uint32_t s[4] = {0, 0, 0, 0};
#pragma unroll
                for (int k = 0; k < CH; k++) {
                    const int j = i * CH + k;  // sample j of the block (for Rgba16 the words below are u[2 i], u[2 i + 1]: the image's own bytes)
                    s[k] = BPS == 2 ? (u[j >> 1] >> (16 * (j & 1))) & 0xFFFFu : (u[j >> 2] >> (8 * (j & 3))) & 0xFFu;
                }
                layout_words<L>(s, m[2 * i], m[2 * i + 1]);
            }
            x += 8;
            if (x == w) x = 0, row += row_stride;
        } else {  // a block that crosses a row end (or the image's last, partial block): pixel by pixel
#pragma unroll
            for (int i = 0; i < 8; i++) {
                m[2 * i] = m[2 * i + 1] = 0;
                if ((uint32_t)i < bpx) {
                    const uint8_t *p = row + (size_t)x * BPP;
                    uint32_t s[4] = {0, 0, 0, 0};
#pragma unroll
                    for (int k = 0; k < CH; k++) s[k] = BPS == 2 ? (uint32_t) reinterpret_cast<const uint16_t *>(p)[k] : (uint32_t)p[k];
                    layout_words<L>(s, m[2 * i], m[2 * i + 1]);
                    if (++x == w) x = 0, row += row_stride;
                }
            }
        }
        const uint32_t fl = (bk == 0 ? B3_CHUNK_START : 0u) | (bk + 1 == nb ? B3_CHUNK_END : 0u) | ((bk + 1 == nb && nchunks == 1) ? B3_ROOT : 0u);
        b3_compress(cv, m, c, bpx * 8, fl, cv);
    }
}

// One wave per group (64 chunks, 8192 pixels) of one image; the wave finds its image in the prefix table of groups (group_first[i] =
// first group of image i, group_first[n] = the grid's waves).  The search and the descriptor are uniform: scalar loads; the layout is
// branched on once.  Images of one group write their digest, the others leave group values in cvs for b3_fold_kernel.
__global__ void __launch_bounds__(256) b3_pixels_ragged_kernel(const uint8_t *__restrict__ px, const RphPixelImage *__restrict__ desc,
                                                               const uint32_t *__restrict__ group_first, uint32_t n, uint32_t *__restrict__ cvs,
                                                               uint8_t *__restrict__ digest)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t g = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64);
    if (g >= group_first[n]) return;
    uint32_t lo = 0, hi = n;  // the image with group_first[img] <= g < group_first[img + 1]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) / 2;
        if (group_first[mid] <= g) lo = mid;
        else hi = mid;
    }
    const uint32_t img = lo, k = g - group_first[img];
    const RphPixelImage &d = desc[img];
    const uint32_t w = d.w, layout = d.layout;
    const size_t row_stride = (size_t)d.row_stride;
    const uint8_t *base = px + d.src_off;
    const uint64_t npx = (uint64_t)w * d.h;
    const uint64_t nchunks = npx ? (npx + PX_PER_CHUNK - 1) / PX_PER_CHUNK : 1;
    const uint64_t c0 = (uint64_t)k * GROUP_CHUNKS, c = c0 + lane;
    const uint32_t in_group = (uint32_t)min<uint64_t>(GROUP_CHUNKS, nchunks - c0);
    Key iv;
#pragma unroll
    for (int i = 0; i < 8; i++) iv.w[i] = b3_iv(i);
    uint32_t cv[8];
#pragma unroll
    for (int i = 0; i < 8; i++) cv[i] = iv.w[i];
    if (lane < in_group) {
        switch (layout) {  // (uniform)
        case RPH_LAYOUT_LUMA8: layout_chunk<RPH_LAYOUT_LUMA8>(base, w, row_stride, npx, nchunks, c, cv); break;
        case RPH_LAYOUT_LUMAA8: layout_chunk<RPH_LAYOUT_LUMAA8>(base, w, row_stride, npx, nchunks, c, cv); break;
        case RPH_LAYOUT_RGB8: layout_chunk<RPH_LAYOUT_RGB8>(base, w, row_stride, npx, nchunks, c, cv); break;
        case RPH_LAYOUT_RGBA8: layout_chunk<RPH_LAYOUT_RGBA8>(base, w, row_stride, npx, nchunks, c, cv); break;
        case RPH_LAYOUT_LUMA16: layout_chunk<RPH_LAYOUT_LUMA16>(base, w, row_stride, npx, nchunks, c, cv); break;
        case RPH_LAYOUT_LUMAA16: layout_chunk<RPH_LAYOUT_LUMAA16>(base, w, row_stride, npx, nchunks, c, cv); break;
        case RPH_LAYOUT_RGB16: layout_chunk<RPH_LAYOUT_RGB16>(base, w, row_stride, npx, nchunks, c, cv); break;
        default: layout_chunk<RPH_LAYOUT_RGBA16>(base, w, row_stride, npx, nchunks, c, cv); break;
        }
    }
    const bool whole = nchunks <= GROUP_CHUNKS;
    wave_fold(cv, in_group, whole, iv, 0);
    uint32_t v = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint32_t x = __shfl(cv[i], 0);  // the folded value is lane 0's: word i goes out from lane i
        v = lane == (uint32_t)i ? x : v;
    }
    if (lane < 8) {
        if (whole) reinterpret_cast<uint32_t *>(digest + (size_t)img * 32)[lane] = v;
        else cvs[(size_t)g * 8 + lane] = v;
    }
}

Key key_of(const uint8_t *key32)
{
    Key k;
    for (int i = 0; i < 8; i++) k.w[i] = key32 ? (uint32_t)key32[4 * i] | (uint32_t)key32[4 * i + 1] << 8 | (uint32_t)key32[4 * i + 2] << 16 |
                                                     (uint32_t)key32[4 * i + 3] << 24
                                               : b3_iv(i);
    return k;
}

bool pixel_geometry_ok(uint32_t n, uint32_t w, uint32_t h, uint32_t channels, size_t row_stride, size_t image_stride)
{
    if (channels != 1 && channels != 3 && channels != 4) return false;
    if (row_stride < (size_t)w * channels) return false;
    if ((uint64_t)w * h > ((uint64_t)1 << 40)) return false;  // chunk indices and groups per image stay 32-bit
    return n <= 1 || image_stride >= row_stride * (h ? h - 1 : 0) + (size_t)w * channels;
}

}  // namespace

size_t rph_pixel_hash_scratch_bytes(uint32_t n, uint32_t w, uint32_t h)
{
    const uint64_t npx = (uint64_t)w * h, nchunks = npx ? (npx + PX_PER_CHUNK - 1) / PX_PER_CHUNK : 1;
    const uint64_t G = (nchunks + GROUP_CHUNKS - 1) / GROUP_CHUNKS;
    return G > 1 ? (size_t)(n * G * 32) : 0;
}

// pixel hashes of n images of one geometry (already checked), asynchronous on `stream`; d_scratch: rph_pixel_hash_scratch_bytes() of
// device memory the launches may use in stream order
int rph_launch_pixel_hash(const uint8_t *d_px, uint32_t n, uint32_t w, uint32_t h, uint32_t channels, size_t row_stride, size_t image_stride,
                          uint8_t *d_hash32, hipStream_t stream, void *d_scratch)
{
    if (n == 0) return RPH_OK;
    const uint64_t npx = (uint64_t)w * h, nchunks = npx ? (npx + PX_PER_CHUNK - 1) / PX_PER_CHUNK : 1;
    const uint32_t G = (uint32_t)((nchunks + GROUP_CHUNKS - 1) / GROUP_CHUNKS);
    const uint64_t waves = (uint64_t)n * G;
    uint32_t *cvs = (uint32_t *)d_scratch;
    const dim3 grid((unsigned)((waves + 3) / 4)), block(256);
    if (channels == 1)
        hipLaunchKernelGGL(b3_pixels_kernel<1>, grid, block, 0, stream, d_px, n, w, h, row_stride, image_stride, G, cvs, d_hash32);
    else if (channels == 3)
        hipLaunchKernelGGL(b3_pixels_kernel<3>, grid, block, 0, stream, d_px, n, w, h, row_stride, image_stride, G, cvs, d_hash32);
    else
        hipLaunchKernelGGL(b3_pixels_kernel<4>, grid, block, 0, stream, d_px, n, w, h, row_stride, image_stride, G, cvs, d_hash32);
    RPH_HIP_CHECK(hipGetLastError());
    if (G > 1) {
        hipLaunchKernelGGL(b3_fold_kernel, dim3(n), dim3(64), 0, stream, (const uint32_t *)nullptr, G, (uint32_t)std::min<uint64_t>(waves, UINT32_MAX),
                           key_of(nullptr), 0u, cvs, d_hash32);
        RPH_HIP_CHECK(hipGetLastError());
    }
    return RPH_OK;
}

// The plan of a ragged pixel-hash call (images already checked): one descriptor per image and the prefix table of groups, n + 1 entries.
// false: more groups than the 32-bit tables hold.
bool rph_pixel_hash_ragged_plan(const uint64_t *offset, const uint32_t *w, const uint32_t *h, const uint32_t *layout, const size_t *row_stride, uint32_t n,
                                std::vector<RphPixelImage> &desc, std::vector<uint32_t> &group_first)
{
    desc.resize(n);
    group_first.resize((size_t)n + 1);
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; i++) {
        desc[i] = RphPixelImage{offset[i], (uint64_t)row_stride[i], w[i], h[i], layout[i], 0};
        group_first[i] = (uint32_t)total;
        const uint64_t npx = (uint64_t)w[i] * h[i], nchunks = npx ? (npx + PX_PER_CHUNK - 1) / PX_PER_CHUNK : 1;
        total += (nchunks + GROUP_CHUNKS - 1) / GROUP_CHUNKS;
        if (total > UINT32_MAX / 2) return false;
    }
    group_first[n] = (uint32_t)total;
    return true;
}

// pixel hashes of n images of any mix of geometries and layouts, asynchronous on `stream`.  d_desc, d_group_first: the plan on the device;
// d_cvs: 32 bytes per group (group_first[n] of them) the launches may use in stream order; multi_group: some image has more than one group
int rph_launch_pixel_hash_ragged(const uint8_t *d_px, const RphPixelImage *d_desc, const uint32_t *d_group_first, uint32_t n, uint32_t groups, bool multi_group,
                                 uint32_t *d_cvs, uint8_t *d_hash32, hipStream_t stream)
{
    if (n == 0) return RPH_OK;
    hipLaunchKernelGGL(b3_pixels_ragged_kernel, dim3((groups + 3) / 4), dim3(256), 0, stream, d_px, d_desc, d_group_first, n, d_cvs, d_hash32);
    RPH_HIP_CHECK(hipGetLastError());
    if (multi_group) {
        hipLaunchKernelGGL(b3_fold_kernel, dim3(n), dim3(64), 0, stream, d_group_first, 0u, groups, key_of(nullptr), 0u, d_cvs, d_hash32);
        RPH_HIP_CHECK(hipGetLastError());
    }
    return RPH_OK;
}

namespace {

// the API's pixel hash: group values in the context's scratch
int pixel_hash_on(rph_ctx *ctx, const uint8_t *d_px, uint32_t n, uint32_t w, uint32_t h, uint32_t channels, size_t row_stride, size_t image_stride,
                  uint8_t *d_hash32, hipStream_t s)
{
    const size_t need = rph_pixel_hash_scratch_bytes(n, w, h);
    if (!need) return rph_launch_pixel_hash(d_px, n, w, h, channels, row_stride, image_stride, d_hash32, s, nullptr);
    std::lock_guard<std::mutex> lock(ctx->mu);
    RPH_TRY(ctx->b3_scratch.acquire(s, need, need + need / 4));
    RPH_TRY(rph_launch_pixel_hash(d_px, n, w, h, channels, row_stride, image_stride, d_hash32, s, ctx->b3_scratch.data()));
    return ctx->b3_scratch.publish(s);
}
}  // namespace

extern "C" {

void rph_blake3_host(const uint8_t *data, size_t len, const uint8_t *key32, uint8_t *digest32_out)
{
    if (!digest32_out || (!data && len)) return;
    const Key key = key_of(key32);
    const uint32_t flags = key32 ? B3_KEYED_HASH : 0u;
    const uint64_t nchunks = len ? (len + B3_CHUNK_LEN - 1) / B3_CHUNK_LEN : 1;
    std::vector<uint32_t> nodes((size_t)nchunks * 8);
    for (uint64_t c = 0; c < nchunks; c++) {
        uint32_t *cv = &nodes[(size_t)c * 8];
        memcpy(cv, key.w, 32);
        const size_t clen = std::min<size_t>(B3_CHUNK_LEN, len - std::min<size_t>(len, c * B3_CHUNK_LEN));
        const uint32_t nb = clen ? (uint32_t)((clen + B3_BLOCK_LEN - 1) / B3_BLOCK_LEN) : 1;
        for (uint32_t bk = 0; bk < nb; bk++) {
            const uint32_t blen = (uint32_t)std::min<size_t>(B3_BLOCK_LEN, clen - bk * B3_BLOCK_LEN);
            uint8_t blk[64] = {};
            if (blen) memcpy(blk, data + c * B3_CHUNK_LEN + bk * B3_BLOCK_LEN, blen);
            uint32_t m[16];
            for (int i = 0; i < 16; i++) m[i] = (uint32_t)blk[4 * i] | (uint32_t)blk[4 * i + 1] << 8 | (uint32_t)blk[4 * i + 2] << 16 | (uint32_t)blk[4 * i + 3] << 24;
            const uint32_t fl = flags | (bk == 0 ? B3_CHUNK_START : 0u) | (bk + 1 == nb ? B3_CHUNK_END : 0u) | ((bk + 1 == nb && nchunks == 1) ? B3_ROOT : 0u);
            b3_compress(cv, m, c, blen, fl, cv);
        }
    }
    // the same pairwise fold with carry as the device kernels
    for (uint64_t cnt = nchunks; cnt > 1;) {
        const uint64_t next = (cnt + 1) / 2;
        for (uint64_t i = 0; i < next; i++) {
            uint32_t p[8];
            if (2 * i + 1 < cnt) b3_parent(key.w, &nodes[(size_t)2 * i * 8], &nodes[(size_t)(2 * i + 1) * 8], flags | (next == 1 ? B3_ROOT : 0u), p);
            else memcpy(p, &nodes[(size_t)2 * i * 8], 32);
            memcpy(&nodes[(size_t)i * 8], p, 32);
        }
        cnt = next;
    }
    for (int i = 0; i < 8; i++)
        for (int b = 0; b < 4; b++) digest32_out[4 * i + b] = (uint8_t)(nodes[i] >> (8 * b));
}

int rph_blake3_batch_dev(rph_ctx *ctx, const void *d_data, const void *d_offsets, uint32_t n, const uint8_t *key32, void *d_digest32, void *stream)
{
    return rph_guarded("rph_blake3_batch_dev", [&]() -> int {
        if (!ctx || (n && (!d_offsets || !d_digest32))) {
            rph_set_error("rph_blake3_batch: null argument");
            return RPH_ERR_INVALID_ARG;
        }
        if (n == 0) return RPH_OK;
        RPH_HIP_CHECK(hipSetDevice(ctx->device));
        hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
        // the scratch of the group values is sized by the call's bytes: offsets[0] and offsets[n] are read back (one synchronisation)
        const uint64_t *off = (const uint64_t *)d_offsets;
        uint64_t ends[2];
        RPH_HIP_CHECK(hipMemcpyAsync(&ends[0], off, 8, hipMemcpyDeviceToHost, s));
        RPH_HIP_CHECK(hipMemcpyAsync(&ends[1], off + n, 8, hipMemcpyDeviceToHost, s));
        RPH_HIP_CHECK(hipStreamSynchronize(s));
        if (ends[1] < ends[0] || (ends[1] > ends[0] && !d_data)) {
            rph_set_error("rph_blake3_batch: offsets must not decrease");
            return RPH_ERR_INVALID_ARG;
        }
        const uint64_t cap64 = (uint64_t)n + (ends[1] - ends[0]) / GROUP_BYTES + 1;  // sum of max(1, ceil(len / 64 KiB)) for non-decreasing offsets
        if (cap64 > UINT32_MAX / 2) {
            rph_set_error("rph_blake3_batch: call too large");
            return RPH_ERR_UNSUPPORTED;
        }
        const uint32_t cap = (uint32_t)cap64;
        const size_t first_bytes = align_up(((size_t)n + 1) * 4, 256);
        std::lock_guard<std::mutex> lock(ctx->mu);
        const size_t need = first_bytes + (size_t)cap * 32;
        RPH_TRY(ctx->b3_scratch.acquire(s, need, need + need / 4));
        uint32_t *d_first = ctx->b3_scratch.as<uint32_t>(), *d_cvs = (uint32_t *)(ctx->b3_scratch.data() + first_bytes);
        const Key key = key_of(key32);
        const uint32_t flags = key32 ? B3_KEYED_HASH : 0u;
        hipLaunchKernelGGL(b3_plan_kernel, dim3(1), dim3(1024), 0, s, off, n, d_first);
        RPH_HIP_CHECK(hipGetLastError());
        const uint32_t blocks = (uint32_t)std::min<uint64_t>((cap64 + 3) / 4, (uint64_t)ctx->compute_units * 16);
        hipLaunchKernelGGL(b3_bytes_kernel, dim3(std::max(1u, blocks)), dim3(256), 0, s, (const uint8_t *)d_data, off, n, d_first, cap, key,
                           flags, d_cvs, (uint8_t *)d_digest32);
        RPH_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(b3_fold_kernel, dim3(n), dim3(64), 0, s, d_first, 0u, cap, key, flags, d_cvs,
                           (uint8_t *)d_digest32);
        RPH_HIP_CHECK(hipGetLastError());
        return ctx->b3_scratch.publish(s);
    });
}

int rph_blake3_batch(rph_ctx *ctx, const uint8_t *const *data, const size_t *len, uint32_t n, const uint8_t *key32, uint8_t *digest32_out)
{
    return rph_guarded("rph_blake3_batch", [&]() -> int {
        if (!ctx || (n && (!data || !len || !digest32_out))) {
            rph_set_error("rph_blake3_batch: null argument");
            return RPH_ERR_INVALID_ARG;
        }
        if (n == 0) return RPH_OK;
        std::vector<uint64_t> off((size_t)n + 1, 0);
        for (uint32_t i = 0; i < n; i++) {
            if (!data[i] && len[i]) {
                rph_set_error("rph_blake3_batch: string %u is NULL", i);
                return RPH_ERR_INVALID_ARG;
            }
            off[i + 1] = off[i] + len[i];
        }
        RPH_HIP_CHECK(hipSetDevice(ctx->device));
        std::vector<uint8_t> packed(off[n]);
        for (uint32_t i = 0; i < n; i++)
            if (len[i]) memcpy(packed.data() + off[i], data[i], len[i]);
        DevBuf d_data, d_off, d_dig;
        RPH_TRY(d_data.alloc(off[n] ? off[n] : 4));
        RPH_TRY(d_off.alloc(off.size() * 8));
        RPH_TRY(d_dig.alloc((size_t)n * 32));
        hipStream_t s = ctx->stream;
        if (off[n]) RPH_HIP_CHECK(hipMemcpyAsync(d_data.data(), packed.data(), off[n], hipMemcpyHostToDevice, s));
        RPH_HIP_CHECK(hipMemcpyAsync(d_off.data(), off.data(), off.size() * 8, hipMemcpyHostToDevice, s));
        RPH_TRY(rph_blake3_batch_dev(ctx, d_data.data(), d_off.data(), n, key32, d_dig.data(), s));
        RPH_HIP_CHECK(hipMemcpyAsync(digest32_out, d_dig.data(), (size_t)n * 32, hipMemcpyDeviceToHost, s));
        RPH_HIP_CHECK(hipStreamSynchronize(s));
        return RPH_OK;
    });
}

int rph_pixel_hash_batch_dev(rph_ctx *ctx, const void *d_px, uint32_t n, uint32_t w, uint32_t h, uint32_t channels, size_t row_stride,
                             size_t image_stride, void *d_hash32, void *stream)
{
    return rph_guarded("rph_pixel_hash_batch_dev", [&]() -> int {
        if (!ctx || (n && (!d_hash32 || (!d_px && w && h))) || !pixel_geometry_ok(n, w, h, channels, row_stride, image_stride)) {
            rph_set_error("rph_pixel_hash_batch: invalid argument (n=%u %ux%ux%u row_stride=%zu image_stride=%zu)", n, w, h, channels, row_stride,
                          image_stride);
            return RPH_ERR_INVALID_ARG;
        }
        RPH_HIP_CHECK(hipSetDevice(ctx->device));
        return pixel_hash_on(ctx, (const uint8_t *)d_px, n, w, h, channels, row_stride, image_stride, (uint8_t *)d_hash32,
                             stream ? (hipStream_t)stream : ctx->stream);
    });
}

int rph_pixel_hash_batch(rph_ctx *ctx, const uint8_t *px, uint32_t n, uint32_t w, uint32_t h, uint32_t channels, size_t row_stride,
                         size_t image_stride, uint8_t *hash32_out)
{
    return rph_guarded("rph_pixel_hash_batch", [&]() -> int {
        if (!ctx || (n && (!hash32_out || (!px && w && h))) || !pixel_geometry_ok(n, w, h, channels, row_stride, image_stride)) {
            rph_set_error("rph_pixel_hash_batch: invalid argument (n=%u %ux%ux%u row_stride=%zu image_stride=%zu)", n, w, h, channels, row_stride,
                          image_stride);
            return RPH_ERR_INVALID_ARG;
        }
        if (n == 0) return RPH_OK;
        RPH_HIP_CHECK(hipSetDevice(ctx->device));
        const size_t one = h ? row_stride * (h - 1) + (size_t)w * channels : 0;
        const size_t bytes = w && h ? (size_t)(n - 1) * image_stride + one : 0;
        DevBuf d_px, d_h;
        RPH_TRY(d_px.alloc(bytes ? bytes : 4));
        RPH_TRY(d_h.alloc((size_t)n * 32));
        hipStream_t s = ctx->stream;
        if (bytes) RPH_HIP_CHECK(hipMemcpyAsync(d_px.data(), px, bytes, hipMemcpyHostToDevice, s));
        RPH_TRY(pixel_hash_on(ctx, d_px.data(), n, w, h, channels, row_stride, image_stride, d_h.data(), s));
        RPH_HIP_CHECK(hipMemcpyAsync(hash32_out, d_h.data(), (size_t)n * 32, hipMemcpyDeviceToHost, s));
        RPH_HIP_CHECK(hipStreamSynchronize(s));
        return RPH_OK;
    });
}

}  // extern "C"
