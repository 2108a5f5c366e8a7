// inflate.h -- zlib (RFC 1950) + deflate (RFC 1951) decoding, one statement for the host threads (png_host.cpp) and the device kernel
// (png_kernels.hip), as blake3.h is for BLAKE3.  The decoder is written against a Sink that owns the output and the 32 KiB history:
// the host sink keeps it in the caller's buffer, the device sink in LDS, where a whole wave performs each copy.  Every check of the
// damaged-stream rule of include/rupphash.h (PNG section) lives here, so the host and the device refuse exactly the same streams.
#pragma once
#include <stddef.h>
#include <stdint.h>
#if defined(__HIP__) || defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RPHZ_HD __host__ __device__ __attribute__((always_inline)) inline
#else
#define RPHZ_HD inline
#endif

namespace rphz {

// what went wrong (all of them mean RPH_ERR_INVALID_ARG to a caller; the codes only help a reader of a trace)
enum : int {
    Z_OK = 0,
    Z_HEADER = -1,      // CM != 8, CINFO > 7, FCHECK, FDICT
    Z_BTYPE = -2,       // block type 3
    Z_STORED = -3,      // stored LEN / NLEN mismatch
    Z_CODES = -4,       // over-subscribed or incomplete code, HLIT > 286, HDIST > 30, a repeat with nothing to repeat or past the end, no end-of-block code
    Z_SYMBOL = -5,      // literal/length 286-287, distance 30-31, or a bit pattern the code does not assign
    Z_DISTANCE = -6,    // a distance that reaches before the start of the output
    Z_TRUNCATED = -7,   // the input ends before the stream does
    Z_ADLER = -8,       // Adler-32 mismatch
    Z_SHORT = -9,       // the stream ends before the image's last byte (reported by the caller)
};

constexpr int FAST_BITS = 9;
constexpr uint32_t ADLER_MOD = 65521u;

// Canonical Huffman code: counts per length + symbols in code order (the slow walk, RFC 1951 3.2.2), and a 9-bit direct table for
// the short codes: entry = (length << 9) | symbol, 0 = longer than FAST_BITS (or unassigned).
struct Huff {
    uint16_t count[16];
    uint16_t symbol[288];
    uint16_t fast[1 << FAST_BITS];
    uint16_t offs[16];  // (build scratch: kept here so that the device build indexes LDS, not private memory)
};

// kind: 0 = the code-length code (must be complete), 1 = literal/length, 2 = distance.  An incomplete literal/length or distance code
// is accepted only when it is a single code of length 1 (zlib's inftrees.c rule); using its unassigned pattern is then Z_SYMBOL.
RPHZ_HD int huff_build(Huff &h, const uint8_t *len, int n, int kind)
{
    for (int i = 0; i < 16; i++) h.count[i] = 0;
    for (int s = 0; s < n; s++) h.count[len[s]]++;
    int max = 0;
    for (int l = 1; l < 16; l++)
        if (h.count[l]) max = l;
    int left = 1;
    for (int l = 1; l < 16; l++) {
        left <<= 1;
        left -= h.count[l];
        if (left < 0) return Z_CODES;
    }
    if (max != 0 && left > 0 && (kind == 0 || max != 1)) return Z_CODES;
    h.offs[1] = 0;
    for (int l = 1; l < 15; l++) h.offs[l + 1] = h.offs[l] + h.count[l];
    for (int s = 0; s < n; s++)
        if (len[s]) h.symbol[h.offs[len[s]]++] = (uint16_t)s;
    for (int i = 0; i < (1 << FAST_BITS); i++) h.fast[i] = 0;
    // canonical codes in symbol order per length; the stream holds them most significant bit first, so the table index is reversed
    uint32_t code = 0;
    int k = 0;
    for (int l = 1; l <= FAST_BITS; l++) {
        for (int c = 0; c < h.count[l]; c++, k++, code++) {
            uint32_t rev = 0;
            for (int b = 0; b < l; b++) rev |= ((code >> b) & 1u) << (l - 1 - b);
            for (uint32_t i = rev; i < (1u << FAST_BITS); i += 1u << l) h.fast[i] = (uint16_t)((l << 9) | h.symbol[k]);
        }
        code <<= 1;
    }
    return Z_OK;
}

struct Bits {
    const uint8_t *in;
    size_t n, pos;  // next byte to load
    uint64_t bb;    // bits not yet consumed, least significant first
    int nb;
    RPHZ_HD void refill()
    {
        while (nb <= 56 && pos < n) {
            bb |= (uint64_t)in[pos++] << nb;
            nb += 8;
        }
    }
    // false when the input holds fewer than k bits
    RPHZ_HD bool need(int k)
    {
        if (nb < k) refill();
        return nb >= k;
    }
    RPHZ_HD uint32_t take(int k)
    {
        uint32_t v = (uint32_t)(bb & ((1ull << k) - 1));
        bb >>= k;
        nb -= k;
        return v;
    }
};

// one symbol, or Z_SYMBOL / Z_TRUNCATED
RPHZ_HD int huff_decode(const Huff &h, Bits &br)
{
    br.refill();
    const uint32_t e = h.fast[br.bb & ((1u << FAST_BITS) - 1)];
    if (e) {
        const int l = (int)(e >> 9);
        if (l > br.nb) return Z_TRUNCATED;
        br.bb >>= l;
        br.nb -= l;
        return (int)(e & 511);
    }
    int code = 0, first = 0, index = 0;
    for (int l = 1; l < 16; l++) {
        if (l > br.nb) return Z_TRUNCATED;
        code |= (int)((br.bb >> (l - 1)) & 1u);
        const int c = h.count[l];
        if (code - c < first) {
            br.bb >>= l;
            br.nb -= l;
            return h.symbol[index + (code - first)];
        }
        index += c;
        first += c;
        first <<= 1;
        code <<= 1;
    }
    return Z_SYMBOL;
}

// RFC 1951 3.2.5 tables as arithmetic (no table in private memory on the device)
RPHZ_HD uint32_t len_base(int s) { return s < 8 ? 3 + s : s == 28 ? 258 : ((4u + ((s - 4) & 3)) << ((s - 4) >> 2)) + 3; }
RPHZ_HD int len_extra(int s) { return (s < 8 || s == 28) ? 0 : (s - 4) >> 2; }
RPHZ_HD uint32_t dist_base(int s) { return s < 4 ? s + 1 : ((2u + (s & 1)) << ((s - 2) >> 1)) + 1; }
RPHZ_HD int dist_extra(int s) { return s < 4 ? 0 : (s - 2) >> 1; }

// Tables a stream needs, wherever they live (stack on the host, LDS on the device)
struct Tables {
    Huff lit, dist, cl;
    uint8_t lens[288 + 32];
};

RPHZ_HD int build_fixed(Tables &t)
{
    for (int i = 0; i < 288; i++) t.lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8;
    int rc = huff_build(t.lit, t.lens, 288, 1);
    for (int i = 0; i < 32; i++) t.lens[i] = 5;  // (32 codes: 30 and 31 are assigned and refused when met, Z_SYMBOL)
    return rc ? rc : huff_build(t.dist, t.lens, 32, 2);
}

RPHZ_HD int build_dynamic(Tables &t, Bits &br)
{
    if (!br.need(14)) return Z_TRUNCATED;
    const int nlen = (int)br.take(5) + 257, ndist = (int)br.take(5) + 1, ncode = (int)br.take(4) + 4;
    if (nlen > 286 || ndist > 30) return Z_CODES;
    for (int i = 0; i < 19; i++) t.lens[i] = 0;
    for (int i = 0; i < ncode; i++) {
        if (!br.need(3)) return Z_TRUNCATED;
        // the code-length order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
        const int j = i - 3, o = i < 3 ? 16 + i : j == 0 ? 0 : (j & 1) ? 8 + (j >> 1) : 8 - (j >> 1);
        t.lens[o] = (uint8_t)br.take(3);
    }
    int rc = huff_build(t.cl, t.lens, 19, 0);
    if (rc) return rc;
    int i = 0;
    while (i < nlen + ndist) {
        int s = huff_decode(t.cl, br);
        if (s < 0) return s;
        if (s < 16) {
            t.lens[i++] = (uint8_t)s;
            continue;
        }
        uint8_t v = 0;
        int rep;
        if (s == 16) {
            if (i == 0) return Z_CODES;
            v = t.lens[i - 1];
            if (!br.need(2)) return Z_TRUNCATED;
            rep = 3 + (int)br.take(2);
        } else if (s == 17) {
            if (!br.need(3)) return Z_TRUNCATED;
            rep = 3 + (int)br.take(3);
        } else {
            if (!br.need(7)) return Z_TRUNCATED;
            rep = 11 + (int)br.take(7);
        }
        if (i + rep > nlen + ndist) return Z_CODES;
        while (rep--) t.lens[i++] = v;
    }
    if (t.lens[256] == 0) return Z_CODES;
    rc = huff_build(t.lit, t.lens, nlen, 1);
    return rc ? rc : huff_build(t.dist, t.lens + nlen, ndist, 2);
}

// Sink: pos() = bytes produced so far, lit(byte), copy(len, dist) with dist <= pos(), stored(ptr, n), adler() after the last byte.
// A copy reads out[pos - dist + (i % dist)] for byte i: only bytes produced before the copy began (an overlapping copy repeats its
// period), which lets a wave write all of a copy's bytes at once.
template <class Sink>
RPHZ_HD int inflate_zlib(const uint8_t *in, size_t n, Tables &t, Sink &out)
{
    Bits br{in, n, 0, 0, 0};
    if (!br.need(16)) return Z_TRUNCATED;
    const uint32_t cmf = br.take(8), flg = br.take(8);
    if ((cmf & 15) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31 != 0 || (flg & 0x20)) return Z_HEADER;
    for (;;) {
        if (!br.need(3)) return Z_TRUNCATED;
        const uint32_t final = br.take(1), type = br.take(2);
        if (type == 3) return Z_BTYPE;
        if (type == 0) {
            br.take(br.nb & 7);  // to the byte boundary: the buffer holds whole bytes from here
            if (!br.need(32)) return Z_TRUNCATED;
            const uint32_t len = br.take(16), nlen = br.take(16);
            if (len != (~nlen & 0xFFFFu)) return Z_STORED;
            // the bytes still in the bit buffer come first, then the input itself
            uint32_t left = len;
            while (left && br.nb >= 8) {
                out.lit(br.take(8));
                left--;
            }
            if (left) {
                if (br.n - br.pos < left) return Z_TRUNCATED;
                out.stored(br.in + br.pos, left);
                br.pos += left;
            }
        } else {
            int rc = type == 1 ? build_fixed(t) : build_dynamic(t, br);
            if (rc) return rc;
            for (;;) {
                int s = huff_decode(t.lit, br);
                if (s < 0) return s;
                if (s < 256) {
                    out.lit((uint32_t)s);
                    continue;
                }
                if (s == 256) break;
                s -= 257;
                if (s >= 29) return Z_SYMBOL;
                int eb = len_extra(s);
                if (!br.need(eb)) return Z_TRUNCATED;
                const uint32_t len = len_base(s) + br.take(eb);
                int d = huff_decode(t.dist, br);
                if (d < 0) return d;
                if (d >= 30) return Z_SYMBOL;
                eb = dist_extra(d);
                if (!br.need(eb)) return Z_TRUNCATED;
                const uint32_t dist = dist_base(d) + br.take(eb);
                if ((uint64_t)dist > out.pos()) return Z_DISTANCE;
                out.copy(len, dist);
            }
        }
        if (final) break;
    }
    br.take(br.nb & 7);
    if (!br.need(32)) return Z_TRUNCATED;
    uint32_t a = 0;
    for (int k = 0; k < 4; k++) a = (a << 8) | br.take(8);
    return a == out.adler() ? Z_OK : Z_ADLER;
}

// Adler-32 of bytes appended to a running (s1, s2); n <= 5552 keeps the sums below 2^32 between reductions (zlib's NMAX)
RPHZ_HD void adler_update(uint32_t &s1, uint32_t &s2, const uint8_t *p, size_t n)
{
    while (n) {
        size_t m = n < 5552 ? n : 5552;
        n -= m;
        while (m--) {
            s1 += *p++;
            s2 += s1;
        }
        s1 %= ADLER_MOD;
        s2 %= ADLER_MOD;
    }
}

// Host sink: bytes below `cap` go to out[], later ones (bytes after the image inside the stream) to a 32 KiB ring that serves their copies
struct HostSink {
    uint8_t *out;
    uint64_t cap, n = 0, summed = 0;
    uint32_t s1 = 1, s2 = 0;
    uint8_t *ring;  // 32 KiB, only touched past cap
    uint8_t at(uint64_t q) const { return q < cap ? out[q] : ring[q & 32767]; }
    void put(uint64_t q, uint8_t v)
    {
        if (q < cap)
            out[q] = v;
        else
            ring[q & 32767] = v;
    }
    void sum_to(uint64_t end)
    {
        while (summed < end) {
            if (summed < cap) {
                uint64_t e = end < cap ? end : cap;
                adler_update(s1, s2, out + summed, (size_t)(e - summed));
                summed = e;
            } else {
                uint8_t v = ring[summed & 32767];
                adler_update(s1, s2, &v, 1);
                summed++;
            }
        }
    }
    void settle()
    {
        if (n - summed >= 16384) sum_to(n);  // bytes past cap are summed before the ring wraps over them
    }
    uint64_t pos() const { return n; }
    void lit(uint32_t b)
    {
        put(n++, (uint8_t)b);
        settle();
    }
    void copy(uint32_t len, uint32_t dist)
    {
        uint64_t src = n - dist;
        if (n + len <= cap) {
            for (uint32_t i = 0; i < len; i++) out[n + i] = out[src + i];
        } else {
            for (uint32_t i = 0; i < len; i++) put(n + i, at(src + i));
        }
        n += len;
        settle();
    }
    void stored(const uint8_t *p, uint32_t len)
    {
        for (uint32_t i = 0; i < len; i++) {
            put(n++, p[i]);
            if ((i & 8191) == 8191) settle();
        }
        settle();
    }
    uint32_t adler()
    {
        sum_to(n);
        return (s2 << 16) | s1;
    }
};

// The whole stream into out[0 .. cap): Z_OK only if it verifies and produced at least cap bytes
inline int inflate_host(const uint8_t *in, size_t n, uint8_t *out, uint64_t cap)
{
    Tables t;
    uint8_t ring[32768];
    HostSink s{out, cap};
    s.ring = ring;
    int rc = inflate_zlib(in, n, t, s);
    if (rc) return rc;
    return s.n < cap ? Z_SHORT : Z_OK;
}

}  // namespace rphz
