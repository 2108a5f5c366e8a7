// vp8l.h -- the VP8L (lossless WebP) entropy decoder and pixel rules, one statement for the host threads (webp_host.cpp) and the device
// kernels (webp_kernels.hip), as inflate.h is for zlib and tiff_lzw.h for LZW.  The decoder is written against a Sink that owns the ARGB
// output and the colour cache: the host sink keeps both in the caller's memory, the device sink keeps the pixels in global memory and the
// cache in LDS, and a whole wave performs each copy.  Every check of the damaged-stream rule of include/rupphash.h (WebP section) that
// concerns the pixel stream lives here, so the host and the device refuse exactly the same streams.  No dependency on libwebp.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "inflate.h"  // RPHZ_HD

namespace rphw {

// what went wrong (all of them mean RPH_ERR_INVALID_ARG to a caller; the codes only help a reader of a trace)
enum : int {
    W_OK = 0,
    W_CODES = -1,      // over-subscribed or incomplete prefix code, no symbol at all, a repeat past the alphabet, max_symbol above it
    W_SYMBOL = -2,     // a bit pattern the code does not assign, a literal/length symbol at or past the alphabet
    W_CACHE = -3,      // a colour-cache symbol without a cache
    W_DISTANCE = -4,   // a distance that reaches before the first pixel
    W_COPY = -5,       // a copy that runs past the last pixel
    W_TRUNCATED = -6,  // more bits consumed than the chunk holds
    W_HEADER = -7,     // signature, version, transform twice, cache size
};

constexpr uint32_t CACHE_MUL = 0x1e35a7bdu;
constexpr uint32_t FAST_BITS = 8;
constexpr uint16_t SLOW = 0xffff;  // fast-table entry of a pattern whose code is longer than FAST_BITS

// The prefix codes of one group as the decoders read them, in uint16 units: five direct tables of 256 entries (length << 12 | symbol
// for codes of up to 8 bits; a code of a single symbol has length 0 everywhere), five arrays of counts per length, then the symbols
// in code order: green / length / cache (280 + cache size), red, blue, alpha (256 each), distance (40).
constexpr uint32_t T_COUNT = 5 * 256, T_SYM = T_COUNT + 5 * 16;
RPHZ_HD uint32_t green_symbols(uint32_t cache_bits) { return 280 + (cache_bits ? 1u << cache_bits : 0); }
RPHZ_HD uint32_t group_stride(uint32_t cache_bits) { return T_SYM + green_symbols(cache_bits) + 3 * 256 + 40; }
RPHZ_HD uint32_t symbol_offset(uint32_t k, uint32_t green_n) { return k ? green_n + 256 * (k - 1) : 0; }
RPHZ_HD uint32_t subsample(uint32_t v, uint32_t bits) { return (v + (1u << bits) - 1) >> bits; }

// Bits least significant first.  `in` holds n bytes; what lies past them reads as zero, and `used` > 8 * n afterwards means the stream
// ran out (checked by the caller where it matters: libwebp's end-of-stream flag).  The device reads aligned dwords from a padded copy
// and keeps the next one loaded ahead of its use; the host assembles them from bytes.
struct Bits {
    const uint8_t *in;
    uint64_t n, pos;  // pos: next byte to load, a multiple of 4 from the (4-byte aligned on the device) start
    uint64_t bb;
    uint32_t nb;
    uint64_t used, total;  // bits consumed, bits there are
    uint32_t ahead;
    RPHZ_HD uint32_t load(uint64_t p) const
    {
#if defined(__HIP_DEVICE_COMPILE__)
        return *reinterpret_cast<const uint32_t *>(in + p);  // (the staging copy is padded with zero bytes)
#else
        uint32_t v = 0;
        if (p + 4 <= n)
            memcpy(&v, in + p, 4);
        else
            for (uint32_t k = 0; k < 4; k++)
                if (p + k < n) v |= (uint32_t)in[p + k] << (8 * k);
        return v;
#endif
    }
    // the stream begins `bit` bits into in[]
    RPHZ_HD void start(const uint8_t *data, uint64_t bytes, uint64_t bit)
    {
        in = data, n = bytes, total = bytes * 8, used = bit;
        pos = (bit >> 5) * 4;
        bb = load(pos);
        nb = 32 - (uint32_t)(bit & 31);
        bb >>= bit & 31;
        pos += 4;
        ahead = load(pos);
    }
    RPHZ_HD void refill()
    {
        if (nb <= 32) {
            bb |= (uint64_t)ahead << nb;
            nb += 32;
            pos += 4;
            ahead = load(pos);
        }
    }
    RPHZ_HD void drop(uint32_t k)
    {
        bb >>= k;
        nb -= k;
        used += k;
    }
    RPHZ_HD uint32_t take(uint32_t k)  // k <= 24
    {
        refill();
        const uint32_t v = (uint32_t)bb & ((1u << k) - 1);
        drop(k);
        return v;
    }
    RPHZ_HD bool out_of_bits() const { return used > total; }
};

// Lengths (0 .. 15) of n symbols -> tables.  libwebp's rule: no symbol at all is refused; a single symbol (of any length) is read with
// zero bits; every other code must be complete (neither over-subscribed nor incomplete).
inline bool build_code(const uint8_t *len, uint32_t n, uint16_t *fast, uint16_t *count, uint16_t *symbol)
{
    uint32_t used = 0, last = 0;
    for (uint32_t l = 0; l < 16; l++) count[l] = 0;
    for (uint32_t s = 0; s < n; s++)
        if (len[s]) count[len[s]]++, used++, last = s;
    if (!used) return false;
    if (used == 1) {
        for (uint32_t l = 0; l < 16; l++) count[l] = 0;
        for (uint32_t i = 0; i < 256; i++) fast[i] = (uint16_t)last;
        symbol[0] = (uint16_t)last;
        return true;
    }
    int left = 1;
    for (uint32_t l = 1; l < 16; l++) {
        left = 2 * left - count[l];
        if (left < 0) return false;
    }
    if (left) return false;
    uint16_t offs[16];
    offs[1] = 0;
    for (uint32_t l = 1; l < 15; l++) offs[l + 1] = offs[l] + count[l];
    for (uint32_t s = 0; s < n; s++)
        if (len[s]) symbol[offs[len[s]]++] = (uint16_t)s;
    for (uint32_t i = 0; i < 256; i++) fast[i] = SLOW;
    uint32_t code = 0, k = 0;
    for (uint32_t l = 1; l <= FAST_BITS; l++) {
        for (uint32_t c = 0; c < count[l]; c++, k++, code++) {
            uint32_t rev = 0;
            for (uint32_t b = 0; b < l; b++) rev |= ((code >> b) & 1u) << (l - 1 - b);
            for (uint32_t i = rev; i < 256; i += 1u << l) fast[i] = (uint16_t)((l << 12) | symbol[k]);
        }
        code <<= 1;
    }
    return true;
}

// one symbol of a code, or W_SYMBOL
RPHZ_HD int read_symbol(const uint16_t *fast, const uint16_t *count, const uint16_t *symbol, Bits &br)
{
    br.refill();
    const uint32_t e = fast[br.bb & 255];
    if (e != SLOW) {
        br.drop(e >> 12);
        return (int)(e & 0xfff);
    }
    int code = 0, first = 0, index = 0;
    for (uint32_t l = 1; l < 16; l++) {
        code |= (int)((br.bb >> (l - 1)) & 1u);
        const int c = count[l];
        if (code - c < first) {
            br.drop(l);
            return symbol[index + (code - first)];
        }
        index += c;
        first += c;
        first <<= 1;
        code <<= 1;
    }
    return W_SYMBOL;
}

// length or distance from its prefix symbol (0 .. 39) and up to 18 extra bits
RPHZ_HD uint32_t prefix_value(uint32_t sym, Bits &br)
{
    if (sym < 4) return sym + 1;
    const uint32_t extra = (sym - 2) >> 1, offset = (2 + (sym & 1)) << extra;
    return offset + br.take(extra) + 1;
}

// distance codes 1 .. 120 name a neighbour (dx, dy) in the plane: byte = dy << 4 | (8 - dx); larger codes are the distance + 120
RPHZ_HD uint32_t plane_distance(uint32_t xsize, uint32_t code)
{
    static constexpr uint8_t plane[120] = {
        0x18, 0x07, 0x17, 0x19, 0x28, 0x06, 0x27, 0x29, 0x16, 0x1a, 0x26, 0x2a, 0x38, 0x05, 0x37, 0x39, 0x15, 0x1b, 0x36, 0x3a,
        0x25, 0x2b, 0x48, 0x04, 0x47, 0x49, 0x14, 0x1c, 0x35, 0x3b, 0x46, 0x4a, 0x24, 0x2c, 0x58, 0x45, 0x4b, 0x34, 0x3c, 0x03,
        0x57, 0x59, 0x13, 0x1d, 0x56, 0x5a, 0x23, 0x2d, 0x44, 0x4c, 0x55, 0x5b, 0x33, 0x3d, 0x68, 0x02, 0x67, 0x69, 0x12, 0x1e,
        0x66, 0x6a, 0x22, 0x2e, 0x54, 0x5c, 0x43, 0x4d, 0x65, 0x6b, 0x32, 0x3e, 0x78, 0x01, 0x77, 0x79, 0x53, 0x5d, 0x11, 0x1f,
        0x64, 0x6c, 0x42, 0x4e, 0x76, 0x7a, 0x21, 0x2f, 0x75, 0x7b, 0x31, 0x3f, 0x63, 0x6d, 0x52, 0x5e, 0x00, 0x74, 0x7c, 0x41,
        0x4f, 0x10, 0x20, 0x62, 0x6e, 0x30, 0x73, 0x7d, 0x51, 0x5f, 0x40, 0x72, 0x7e, 0x61, 0x6f, 0x50, 0x71, 0x7f, 0x60, 0x70};
    if (code > 120) return code - 120;
    const uint32_t c = plane[code - 1];
    const int32_t d = (int32_t)(c >> 4) * (int32_t)xsize + 8 - (int32_t)(c & 15);
    return d < 1 ? 1u : (uint32_t)d;
}

// One coded image (the main one, or a sub-image read by the host): its geometry, colour cache, entropy image and tables
struct Stream {
    uint32_t xsize, ysize;
    uint32_t cache_bits;   // 0: none
    uint32_t meta_bits;    // block size of the entropy image (when ent != nullptr)
    const uint16_t *ent;   // group of every block, or nullptr: one group
    const uint16_t *tables;  // group g at tables + g * group_stride(cache_bits)
};

// Sink: group(tables, g, stride) returns where the decoder reads group g's tables from (the device keeps the groups in use in LDS);
// lit(argb), cached(key) (the pixel in slot `key` of the colour cache), copy(dist, len) with dist <= pixels so far and len <= pixels
// still to come; each of them also enters the pixels it writes into the colour cache, in pixel order.  A copy reads pixel
// pos - dist + (i % dist) for its pixel i: only pixels written before the copy began.
// Every turn of the loop writes at least one pixel, so it ends after xsize * ysize turns at the most whatever the bits say.
template <class Sink>
RPHZ_HD int decode_pixels(const Stream &s, Bits &br, Sink &out)
{
    const uint64_t total = (uint64_t)s.xsize * s.ysize;
    const uint32_t green_n = green_symbols(s.cache_bits), stride = group_stride(s.cache_bits);
    const uint32_t bw = subsample(s.xsize, s.meta_bits);
    const uint16_t *g = out.group(s.tables, 0, stride);
    uint32_t cur_block = ~0u, x = 0, y = 0;
    uint64_t pos = 0;
    while (pos < total) {
        if (br.out_of_bits()) return W_TRUNCATED;
        if (s.ent) {
            const uint32_t block = (y >> s.meta_bits) * bw + (x >> s.meta_bits);
            if (block != cur_block) {
                cur_block = block;
                g = out.group(s.tables + (size_t)s.ent[block] * stride, s.ent[block], stride);
            }
        }
        const uint16_t *cnt = g + T_COUNT, *sym = g + T_SYM;
        const int green = read_symbol(g, cnt, sym, br);
        if (green < 0) return green;
        if (green < 256) {
            const int red = read_symbol(g + 256, cnt + 16, sym + symbol_offset(1, green_n), br);
            const int blue = read_symbol(g + 512, cnt + 32, sym + symbol_offset(2, green_n), br);
            const int alpha = read_symbol(g + 768, cnt + 48, sym + symbol_offset(3, green_n), br);
            if ((red | blue | alpha) < 0) return W_SYMBOL;
            out.lit(((uint32_t)alpha << 24) | ((uint32_t)red << 16) | ((uint32_t)green << 8) | (uint32_t)blue);
            pos++;
            if (++x == s.xsize) x = 0, y++;
        } else if (green < 280) {
            const uint32_t len = prefix_value((uint32_t)green - 256, br);
            const int dsym = read_symbol(g + 1024, cnt + 64, sym + symbol_offset(4, green_n), br);
            if (dsym < 0) return dsym;
            const uint32_t dist = plane_distance(s.xsize, prefix_value((uint32_t)dsym, br));
            if (br.out_of_bits()) return W_TRUNCATED;
            if (dist > pos) return W_DISTANCE;
            if (len > total - pos) return W_COPY;
            out.copy(dist, len);
            pos += len;
            x += len;
            if (x >= s.xsize) y += x / s.xsize, x %= s.xsize;
        } else if ((uint32_t)green < green_n) {
            if (!s.cache_bits) return W_CACHE;
            out.cached((uint32_t)green - 280);
            pos++;
            if (++x == s.xsize) x = 0, y++;
        } else {
            return W_SYMBOL;
        }
    }
    return br.out_of_bits() ? W_TRUNCATED : W_OK;
}

// ---- the inverse transforms' pixel rules ----
RPHZ_HD uint32_t add_pixels(uint32_t a, uint32_t b)
{
    return (((a & 0xff00ff00u) + (b & 0xff00ff00u)) & 0xff00ff00u) | (((a & 0x00ff00ffu) + (b & 0x00ff00ffu)) & 0x00ff00ffu);
}
RPHZ_HD uint32_t avg2(uint32_t a, uint32_t b) { return (((a ^ b) & 0xfefefefeu) >> 1) + (a & b); }
RPHZ_HD uint32_t abs_diff_sum(uint32_t a, uint32_t b)
{
    uint32_t s = 0;
    for (uint32_t k = 0; k < 32; k += 8) {
        const int d = (int)((a >> k) & 255) - (int)((b >> k) & 255);
        s += (uint32_t)(d < 0 ? -d : d);
    }
    return s;
}
RPHZ_HD uint32_t clip255(int v) { return v < 0 ? 0u : v > 255 ? 255u : (uint32_t)v; }

// Predictor `mode` of the format text from L, T, TL, TR.  Written as values chosen by the mode, not as a switch: the lanes of a wave
// sit in different mode blocks, and a select costs every lane the same.  Modes 14 and 15 (which the text does not define) predict
// as mode 0, as libwebp does.
RPHZ_HD uint32_t predict(uint32_t mode, uint32_t L, uint32_t T, uint32_t TL, uint32_t TR)
{
    const uint32_t aLT = avg2(L, T), aLTL = avg2(L, TL), aTTR = avg2(T, TR);
    uint32_t full = 0, half = 0;
    for (uint32_t k = 0; k < 32; k += 8) {
        const int l = (int)((L >> k) & 255), t = (int)((T >> k) & 255), tl = (int)((TL >> k) & 255), a = (int)((aLT >> k) & 255);
        full |= clip255(l + t - tl) << k;
        half |= clip255(a + (a - tl) / 2) << k;
    }
    // Select: the one of L and T that lies nearer to L + T - TL (Manhattan distance over the four channels), T on a tie
    const uint32_t sel = (int)(abs_diff_sum(L, TL) - abs_diff_sum(T, TL)) <= 0 ? T : L;
    uint32_t p = 0xff000000u;
    p = mode == 1 ? L : p;
    p = mode == 2 ? T : p;
    p = mode == 3 ? TR : p;
    p = mode == 4 ? TL : p;
    p = mode == 5 ? avg2(avg2(L, TR), T) : p;
    p = mode == 6 ? aLTL : p;
    p = mode == 7 ? aLT : p;
    p = mode == 8 ? avg2(TL, T) : p;
    p = mode == 9 ? aTTR : p;
    p = mode == 10 ? avg2(aLTL, aTTR) : p;
    p = mode == 11 ? sel : p;
    p = mode == 12 ? full : p;
    p = mode == 13 ? half : p;
    return p;
}

// cross-colour: the block's word holds red_to_blue (bits 16-23), green_to_blue (8-15), green_to_red (0-7), signed, in 1/32 units
RPHZ_HD uint32_t cross_colour(uint32_t m, uint32_t argb)
{
    const int8_t green = (int8_t)(argb >> 8);
    uint32_t red = (argb >> 16) & 255, blue = argb & 255;
    red = (red + (uint32_t)(((int)(int8_t)m * green) >> 5)) & 255;
    blue = (blue + (uint32_t)(((int)(int8_t)(m >> 8) * green) >> 5)) & 255;
    blue = (blue + (uint32_t)(((int)(int8_t)(m >> 16) * (int8_t)red) >> 5)) & 255;
    return (argb & 0xff00ff00u) | (red << 16) | blue;
}
RPHZ_HD uint32_t add_green(uint32_t argb)
{
    const uint32_t g = (argb >> 8) & 255;
    return (argb & 0xff00ff00u) | ((((argb & 0x00ff00ffu) + (g << 16 | g))) & 0x00ff00ffu);
}
// colour indexing with `bits` (0 .. 3): 2^bits pixels in the green byte of a coded pixel, lowest bits first
RPHZ_HD uint32_t bundled_index(uint32_t coded, uint32_t x, uint32_t bits)
{
    const uint32_t bpp = 8u >> bits;
    return ((coded >> 8) & 255) >> ((x & ((1u << bits) - 1)) * bpp) & ((1u << bpp) - 1);
}

enum : uint32_t { TR_PREDICTOR = 0, TR_CROSS_COLOUR = 1, TR_SUBTRACT_GREEN = 2, TR_COLOUR_INDEXING = 3 };

}  // namespace rphw
