// tiff_lzw.h -- the two byte-oriented TIFF decompressors, LZW (Compression 5) and PackBits (32773), one statement each for the host
// threads (tiff_host.cpp) and the device kernels (tiff_kernels.hip), as inflate.h is for Deflate.  Both are written against a Sink that
// owns the output of one strip or tile, so the host and the device refuse exactly the same streams (include/rupphash.h, TIFF section).
//
// LZW: codes most significant bit first, 9 to 12 bits, "early change" (the width grows one code early), Clear 256, EOI 257.  A table
// entry is not a (prefix, byte) pair but (position of its string in the segment's output, length): the string of the entry made by
// code k is the string of code k-1 plus the first byte of k's, and those bytes lie next to each other in the output.  Every code then
// decodes to one copy of bytes that are already out, which a wave performs 64 bytes per step; the KwKwK case (a code equal to the
// next free entry) is the copy that overlaps its own output.
//
// Sink: pos() = bytes produced, cap() = the segment's bytes; lit(byte); copy(from, len): out[pos + i] = out[from + i % (pos - from)]
// for i < len, from < pos (bytes produced before the copy began); span(ptr, len): len input bytes as they are; fill(byte, len).
// The decoders never ask for more than cap() - pos() bytes.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#if defined(__HIP__) || defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RPHT_HD __host__ __device__ __attribute__((always_inline)) inline
#else
#define RPHT_HD inline
#endif

namespace rpht {

// what went wrong (all of them RPH_ERR_INVALID_ARG to a caller)
enum : int {
    L_OK = 0,
    L_FIRST = -1,      // the first code after a Clear (or of the stream) is 256 or above
    L_CODE = -2,       // a code above the next free entry
    L_TRUNCATED = -3,  // the input runs out of bits, or sends EOI, before the segment is full
    L_TABLE = -4,      // the table would grow past 4096 entries
    L_PACKBITS = -5,   // a run or literal cut off by the end of the input
};

constexpr uint32_t LZW_CLEAR = 256, LZW_EOI = 257, LZW_FIRST = 258, LZW_ENTRIES = 4096;
// The longest string an entry can hold: entry k is one byte longer than the string before it, the first entry (258) holds 2 bytes and
// the last (4095) therefore at most 4095 - 258 + 2 = 3839; a KwKwK code is one such entry too.  Every code takes at least 9 bits, so n
// input bytes decode to at most 3839 * floor(8 n / 9) bytes: the plausibility bound of a strip (tiff_host.cpp).
constexpr uint64_t LZW_MAX_STRING = LZW_ENTRIES - 1 - LZW_FIRST + 2;

// the string table, wherever it lives (stack on the host, LDS on the device): 24 KiB
struct LzwTable {
    uint32_t pos[LZW_ENTRIES];
    uint16_t len[LZW_ENTRIES];
};

// Most-significant-bit-first reader.  It refills four bytes at a time: the device hands in a 4-byte aligned pointer and loads dwords,
// the host copies them; the last 1-3 bytes are read one by one, so nothing past in[n) is touched.
struct MsbBits {
    const uint8_t *in;
    size_t n, pos;
    uint64_t bb;  // the unread bits in the low nb bits, oldest on top
    int nb;
    RPHT_HD void refill()
    {
        if (nb > 32) return;
        if (n - pos >= 4) {
            uint32_t v;
#if defined(__HIP_DEVICE_COMPILE__)
            v = __builtin_bswap32(*reinterpret_cast<const uint32_t *>(in + pos));
#else
            v = ((uint32_t)in[pos] << 24) | ((uint32_t)in[pos + 1] << 16) | ((uint32_t)in[pos + 2] << 8) | in[pos + 3];
#endif
            bb = (bb << 32) | v;
            nb += 32;
            pos += 4;
            return;
        }
        while (pos < n) {
            bb = (bb << 8) | in[pos++];
            nb += 8;
        }
    }
    // false when the input holds fewer than k bits (k <= 16)
    RPHT_HD bool take(int k, uint32_t &v)
    {
        if (nb < k) refill();
        if (nb < k) return false;
        nb -= k;
        v = (uint32_t)(bb >> nb) & ((1u << k) - 1);
        return true;
    }
};

template <class Sink>
RPHT_HD int lzw_decode(const uint8_t *in, size_t n, LzwTable &t, Sink &out)
{
    MsbBits br{in, n, 0, 0, 0};
    const uint64_t cap = out.cap();
    uint32_t next = LZW_FIRST;
    int width = 9;
    bool have_prev = false, after_clear = false;
    uint64_t prev_pos = 0;
    uint32_t prev_len = 0;
    // every turn consumes at least 9 input bits, and every turn but a Clear produces a byte: bounded by both
    while (out.pos() < cap) {
        uint32_t code;
        if (!br.take(width, code)) return L_TRUNCATED;
        if (code == LZW_CLEAR) {
            if (after_clear) return L_FIRST;
            after_clear = true;
            have_prev = false;
            next = LZW_FIRST;
            width = 9;
            continue;
        }
        if (code == LZW_EOI) return have_prev ? L_TRUNCATED : L_FIRST;
        const uint64_t at = out.pos(), room = cap - at;
        uint32_t len;
        if (!have_prev) {
            if (code >= 256) return L_FIRST;
            out.lit(code);
            len = 1;
        } else if (code < 256) {
            out.lit(code);
            len = 1;
        } else if (code < next) {
            len = t.len[code];
            out.copy(t.pos[code], (uint32_t)(len < room ? len : room));
        } else if (code == next) {
            len = prev_len + 1;  // the string before, and its first byte again
            out.copy(prev_pos, (uint32_t)(len < room ? len : room));
        } else {
            return L_CODE;
        }
        after_clear = false;
        if (len >= room) break;  // the segment is full: what follows is not examined
        if (have_prev) {
            if (next >= LZW_ENTRIES) return L_TABLE;
            t.pos[next] = (uint32_t)prev_pos;
            t.len[next] = (uint16_t)(prev_len + 1);
            next++;
            if (next + 1 >= (1u << width) && width < 12) width++;  // early change: 511 -> 10 bits, 1023 -> 11, 2047 -> 12
        }
        have_prev = true;
        prev_pos = at;
        prev_len = len;
    }
    return L_OK;
}

// PackBits: n in 0..127 copies n + 1 bytes, n in 129..255 repeats the next byte 257 - n times, 128 does nothing
template <class Sink>
RPHT_HD int packbits_decode(const uint8_t *in, size_t n, Sink &out)
{
    const uint64_t cap = out.cap();
    size_t pos = 0;
    // every turn consumes at least one input byte
    while (out.pos() < cap) {
        if (pos >= n) return L_PACKBITS;
        const uint32_t c = in[pos++];
        if (c == 128) continue;
        const uint64_t room = cap - out.pos();
        if (c < 128) {
            const uint32_t len = c + 1;
            if (n - pos < len) return L_PACKBITS;
            out.span(in + pos, (uint32_t)(len < room ? len : room));
            pos += len;
        } else {
            if (pos >= n) return L_PACKBITS;
            const uint32_t len = 257 - c;
            out.fill(in[pos++], (uint32_t)(len < room ? len : room));
        }
    }
    return L_OK;
}

// Host sink: the segment's bytes in plain memory
struct HostSegSink {
    uint8_t *out;
    uint64_t cap_, n = 0;
    uint64_t pos() const { return n; }
    uint64_t cap() const { return cap_; }
    void lit(uint32_t b) { out[n++] = (uint8_t)b; }
    void copy(uint64_t from, uint32_t len)
    {
        for (uint32_t i = 0; i < len; i++) out[n + i] = out[from + i];  // (forward, byte by byte: an overlapping copy repeats its period)
        n += len;
    }
    void span(const uint8_t *p, uint32_t len)
    {
        memcpy(out + n, p, len);
        n += len;
    }
    void fill(uint8_t b, uint32_t len)
    {
        memset(out + n, b, len);
        n += len;
    }
};

}  // namespace rpht
