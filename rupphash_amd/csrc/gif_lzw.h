// gif_lzw.h -- the GIF flavour of LZW, one statement for the host threads (gif_host.cpp) and the device kernel (gif_kernels.hip), written
// against the Sink of tiff_lzw.h so that the host and the device refuse exactly the same streams (include/rupphash.h, GIF section).
//
// Where it departs from the TIFF decoder: codes least significant bit first; a minimum code size m of 2..8 with Clear = 1 << m,
// EOI = Clear + 1 and the first free entry Clear + 2; the width starts at m + 1 and grows when the next free entry reaches 1 << width
// (no early change), up to 12; a table of 4096 entries is simply full: no entry is added and the width stays 12 until a Clear arrives
// ("deferred clear"), and the stream stays valid; a stream whose first code is not a Clear starts from the initial table.
// What it keeps: a table entry is (position of its string in the frame's indices, length), so every code is one copy of bytes that are
// already out, which a wave performs 64 bytes per step, and the KwKwK code (equal to the next free entry) is the copy that overlaps its
// own output.
//
// Sink: pos() = bytes produced, cap() = the frame's bytes; lit(byte); copy(from, len): out[pos + i] = out[from + i % (pos - from)]
// for i < len, from < pos.  The decoder never asks for more than cap() - pos() bytes.
#pragma once
#include <stddef.h>
#include <stdint.h>
#if defined(__HIP__) || defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RPHG_HD __host__ __device__ __attribute__((always_inline)) inline
#else
#define RPHG_HD inline
#endif

namespace rphg {

// what went wrong (all of them RPH_ERR_INVALID_ARG to a caller)
enum : int {
    L_OK = 0,
    L_FIRST = -1,      // the first code after a Clear (or of the stream) is above Clear
    L_CODE = -2,       // a code above the next free entry
    L_TRUNCATED = -3,  // the input runs out of bits, or sends EOI, before the frame is full
};

constexpr uint32_t LZW_ENTRIES = 4096, LZW_MIN_CODE_SIZE = 2, LZW_MAX_CODE_SIZE = 8;

// The longest string an entry can hold: entry k is one byte longer than the string before it, the first free entry (Clear + 2) holds 2
// bytes and the last (4095) therefore at most 4095 - (Clear + 2) + 2 = 4095 - Clear; a KwKwK code is one such entry too, and a full
// table adds none.  Every code takes at least m + 1 bits, so n input bytes decode to at most (4095 - (1 << m)) * floor(8 n / (m + 1))
// indices: the plausibility bound of a frame (gif_host.cpp).
RPHG_HD uint64_t lzw_max_string(uint32_t m) { return LZW_ENTRIES - 1 - (1u << m); }
RPHG_HD uint64_t lzw_max_expansion(uint32_t m, uint64_t n) { return lzw_max_string(m) * (n * 8 / (m + 1)); }

// the string table, wherever it lives (stack on the host, LDS on the device): 24 KiB
struct LzwTable {
    uint32_t pos[LZW_ENTRIES];
    uint16_t len[LZW_ENTRIES];
};

// Least-significant-bit-first reader.  It refills four bytes at a time: the device hands in a 4-byte aligned pointer and loads dwords,
// the host assembles them; the last 1-3 bytes are read one by one, so nothing past in[n) is touched.
struct LsbBits {
    const uint8_t *in;
    size_t n, pos;
    uint64_t bb;  // the unread bits in the low nb bits, oldest at the bottom
    int nb;
    RPHG_HD void refill()
    {
        if (nb > 32) return;
        if (n - pos >= 4) {
            uint32_t v;
#if defined(__HIP_DEVICE_COMPILE__)
            v = *reinterpret_cast<const uint32_t *>(in + pos);
#else
            v = (uint32_t)in[pos] | ((uint32_t)in[pos + 1] << 8) | ((uint32_t)in[pos + 2] << 16) | ((uint32_t)in[pos + 3] << 24);
#endif
            bb |= (uint64_t)v << nb;
            nb += 32;
            pos += 4;
            return;
        }
        while (pos < n) {
            bb |= (uint64_t)in[pos++] << nb;
            nb += 8;
        }
    }
    // false when the input holds fewer than k bits (k <= 12)
    RPHG_HD bool take(int k, uint32_t &v)
    {
        if (nb < k) refill();
        if (nb < k) return false;
        v = (uint32_t)bb & ((1u << k) - 1);
        bb >>= k;
        nb -= k;
        return true;
    }
};

// m: the minimum code size, LZW_MIN_CODE_SIZE .. LZW_MAX_CODE_SIZE (checked by the caller)
template <class Sink>
RPHG_HD int lzw_decode(const uint8_t *in, size_t n, uint32_t m, LzwTable &t, Sink &out)
{
    LsbBits br{in, n, 0, 0, 0};
    const uint32_t clear = 1u << m, eoi = clear + 1, first = clear + 2;
    const uint64_t cap = out.cap();
    uint32_t next = first;
    int width = (int)m + 1;
    bool have_prev = false;
    uint64_t prev_pos = 0;
    uint32_t prev_len = 0;
    // every turn consumes at least m + 1 input bits, and every turn but a Clear produces a byte: bounded by both
    while (out.pos() < cap) {
        uint32_t code;
        if (!br.take(width, code)) return L_TRUNCATED;
        if (code == clear) {  // (a Clear behind a Clear does again what the first one did)
            have_prev = false;
            next = first;
            width = (int)m + 1;
            continue;
        }
        if (code == eoi) return L_TRUNCATED;
        const uint64_t at = out.pos(), room = cap - at;
        uint32_t len;
        if (code < clear) {
            out.lit(code);
            len = 1;
        } else if (!have_prev) {
            return L_FIRST;
        } else if (code < next) {
            len = t.len[code];
            out.copy(t.pos[code], (uint32_t)(len < room ? len : room));
        } else if (code == next) {  // (next < 4096 here: a code has at most 12 bits)
            len = prev_len + 1;     // the string before, and its first byte again
            out.copy(prev_pos, (uint32_t)(len < room ? len : room));
        } else {
            return L_CODE;
        }
        if (len >= room) break;  // the frame is full: what follows is not examined
        if (have_prev && next < LZW_ENTRIES) {  // a full table stays as it is until a Clear
            t.pos[next] = (uint32_t)prev_pos;
            t.len[next] = (uint16_t)(prev_len + 1);
            next++;
            if (next == (1u << width) && width < 12) width++;
        }
        have_prev = true;
        prev_pos = at;
        prev_len = len;
    }
    return L_OK;
}

// Host sink: the frame's indices in plain memory
struct HostSink {
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
};

}  // namespace rphg
