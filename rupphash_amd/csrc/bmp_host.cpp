// bmp_host.cpp -- the host half of the BMP path: file header, DIB header, masks, palette, the placement and size of the pixel array, the
// RLE8 / RLE4 walk, what the pipeline stages for the expand kernel, and the whole decoder on the CPU for rph_bmp_decode_host.  No HIP:
// tools/fuzz_bmp_host.cpp builds this file with g++ under ASan + UBSan.
#include "bmp_host.h"

#include <string.h>

#include "../../include/rupphash.h"

namespace rphb {

namespace {

inline uint32_t u16(const uint8_t *d, size_t o) { return (uint32_t)d[o] | ((uint32_t)d[o + 1] << 8); }
inline uint32_t u32(const uint8_t *d, size_t o) { return u16(d, o) | (u16(d, o + 2) << 16); }
inline uint32_t align4(uint32_t v) { return (v + 3) & ~3u; }

// a mask as (shift, len) with len <= 8; false: its bits are not one run, or lie above the pixel
bool field_of(uint32_t mask, uint32_t bits, uint8_t &shift, uint8_t &len)
{
    shift = len = 0;
    if (!mask) return true;
    if (bits == 16 && mask > 0xffffu) return false;
    uint32_t s = 0;
    while (!((mask >> s) & 1)) s++;
    const uint32_t run = mask >> s;
    if (run & (run + 1)) return false;
    uint32_t l = 0;
    while (l < 32 && ((run >> l) & 1)) l++;
    if (l > 8) s += l - 8, l = 8;
    shift = (uint8_t)s, len = (uint8_t)l;
    return true;
}

// The one RLE decoder.  put(x, y, index) for every pixel the stream sets, y counted from the bottom row; covered: how many it set (a
// position never moves back, so none is set twice).  false: the stream leaves the bitmap or ends without end-of-bitmap.
template <class Put>
bool rle_walk(const uint8_t *s, size_t n, uint32_t w, uint32_t h, bool four, uint64_t &covered, Put &&put)
{
    size_t pos = 0;
    uint32_t x = 0, y = 0;
    covered = 0;
    for (;;) {
        if (n - pos < 2) return false;
        const uint32_t a = s[pos], b = s[pos + 1];
        pos += 2;
        if (a) {  // encoded run: a pixels of b (RLE4: of b's two nibbles in turn)
            if (y >= h || a > w - x) return false;
            for (uint32_t k = 0; k < a; k++) put(x + k, y, four ? ((k & 1) ? (b & 15u) : (b >> 4)) : b);
            x += a;
            covered += a;
        } else if (b == 0) {  // end of line
            x = 0;
            if (++y > h) return false;
        } else if (b == 1) {  // end of bitmap
            return true;
        } else if (b == 2) {  // delta
            if (n - pos < 2) return false;
            x += s[pos], y += s[pos + 1];
            pos += 2;
            if (x > w || y > h) return false;
        } else {  // absolute run: b pixels, padded to 16 bits
            const size_t bytes = four ? (b + 1) / 2 : b, padded = (bytes + 1) & ~(size_t)1;
            if (n - pos < padded) return false;
            if (y >= h || b > w - x) return false;
            for (uint32_t k = 0; k < b; k++) {
                const uint32_t v = four ? s[pos + k / 2] : s[pos + k];
                put(x + k, y, four ? ((k & 1) ? (v & 15u) : (v >> 4)) : v);
            }
            x += b;
            covered += b;
            pos += padded;
        }
    }
}

}  // namespace

// The checks run in this order, and the first that fails decides the status (include/rupphash.h, BMP section)
int parse(const uint8_t *data, size_t len, Parsed &p)
{
    Image &im = p.im;
    memset(&im, 0, sizeof im);
    p.data_off = p.data_len = 0;
    p.rle = 0;
    p.rle_skips = false;
    if (len < 18 || data[0] != 'B' || data[1] != 'M') return RPH_ERR_INVALID_ARG;
    const uint32_t hdr = u32(data, 14);
    if (hdr != 12 && hdr != 40 && hdr != 52 && hdr != 56 && hdr != 108 && hdr != 124) return RPH_ERR_UNSUPPORTED;
    if (len - 14 < hdr) return RPH_ERR_INVALID_ARG;
    int64_t w, h;
    uint32_t planes, bits, comp = 0, clr_used = 0;
    if (hdr == 12) {
        w = u16(data, 18), h = u16(data, 20), planes = u16(data, 22), bits = u16(data, 24);
    } else {
        w = (int32_t)u32(data, 18), h = (int32_t)u32(data, 22), planes = u16(data, 26), bits = u16(data, 28), comp = u32(data, 30), clr_used = u32(data, 46);
    }
    if (planes != 1) return RPH_ERR_INVALID_ARG;
    if (w <= 0 || h == 0) return RPH_ERR_INVALID_ARG;
    im.top_down = h < 0;
    if (h < 0) h = -h;
    if (w > MAX_SIDE || h > MAX_SIDE) return RPH_ERR_UNSUPPORTED;
    if ((uint64_t)w * (uint64_t)h > MAX_PIXELS) return RPH_ERR_UNSUPPORTED;
    im.w = (uint32_t)w, im.h = (uint32_t)h;
    bool ok = false;
    switch (comp) {
    case 0: ok = bits == 1 || bits == 2 || bits == 4 || bits == 8 || bits == 16 || bits == 24 || bits == 32; break;
    case 1: ok = bits == 8; break;
    case 2: ok = bits == 4; break;
    case 3:
    case 6: ok = bits == 16 || bits == 32; break;
    default: break;
    }
    if (!ok) return RPH_ERR_UNSUPPORTED;
    if ((comp == 1 || comp == 2) && im.top_down) return RPH_ERR_INVALID_ARG;
    size_t headers_end = 14 + (size_t)hdr;
    im.out_ch = 3;
    im.bits = (uint8_t)bits;
    if (bits <= 8) {
        im.kind = K_PAL;
        const uint32_t n = clr_used ? clr_used : 1u << bits, entry = hdr == 12 ? 3 : 4;
        if (n > 1u << bits) return RPH_ERR_INVALID_ARG;
        if (len - headers_end < (size_t)n * entry) return RPH_ERR_INVALID_ARG;
        for (uint32_t i = 0; i < n; i++) {
            const uint8_t *e = data + headers_end + (size_t)i * entry;
            p.pal[i] = (uint32_t)e[2] | ((uint32_t)e[1] << 8) | ((uint32_t)e[0] << 16);
        }
        im.pal_n = (uint16_t)n;
        headers_end += (size_t)n * entry;
    } else if (bits == 24) {
        im.kind = K_BGR24;
    } else {
        im.kind = K_FIELDS;
        uint32_t mask[4] = {0xff0000u, 0xff00u, 0xffu, 0};
        if (bits == 16) mask[0] = 0x7c00u, mask[1] = 0x3e0u, mask[2] = 0x1fu;
        if (comp == 3 || comp == 6) {
            uint32_t n_masks;
            if (hdr == 40) {  // the masks follow the header
                n_masks = comp == 3 ? 3 : 4;
                if (len - headers_end < n_masks * 4) return RPH_ERR_INVALID_ARG;
                headers_end += n_masks * 4;
            } else {  // they are part of it
                n_masks = hdr == 52 ? 3 : 4;
            }
            for (uint32_t c = 0; c < 4; c++) mask[c] = c < n_masks ? u32(data, 54 + 4 * c) : 0;
        }
        for (uint32_t c = 0; c < 4; c++)
            if (!field_of(mask[c], bits, im.shift[c], im.len[c])) return RPH_ERR_INVALID_ARG;
        if (im.len[3]) im.out_ch = 4;
        im.bytes8 = bits == 32;
        for (uint32_t c = 0; c < 4; c++)
            if (im.len[c] && (im.len[c] != 8 || (im.shift[c] & 7))) im.bytes8 = 0;
    }
    const uint32_t off = u32(data, 10);
    if (off < headers_end || off >= len) return RPH_ERR_INVALID_ARG;
    p.data_off = off;
    im.src_stride = align4((im.w * bits + 7) / 8);
    im.out_stride = align4(im.w * im.out_ch);
    im.band = GROUPS_PER_ITEM / ((im.w + 3) / 4);
    if (!im.band) im.band = 1;
    if (comp == 1 || comp == 2) {
        p.rle = (uint8_t)bits;
        p.data_len = len - off;
        uint64_t covered = 0;
        if (!rle_walk(data + off, p.data_len, im.w, im.h, comp == 2, covered, [](uint32_t, uint32_t, uint32_t) {})) return RPH_ERR_INVALID_ARG;
        p.rle_skips = covered != (uint64_t)im.w * im.h;
        // the plane the host threads decode: 8-bit indices, skipped pixels as index 255; when the palette has a colour there, B G R rows
        im.bits = 8;
        im.src_stride = align4(im.w);
        if (p.rle_skips && im.pal_n == 256) im.kind = K_BGR24, im.bits = 24, im.src_stride = align4(im.w * 3);
    } else {
        p.data_len = (size_t)im.src_stride * im.h;
        if (len - off < p.data_len) return RPH_ERR_INVALID_ARG;
    }
    return RPH_OK;
}

void stage(const uint8_t *data, const Parsed &p, uint8_t *dst)
{
    const Image &im = p.im;
    const size_t stride = im.src_stride;
    if (!p.rle) {
        memcpy(dst, data + p.data_off, p.data_len);
        return;
    }
    uint64_t covered;
    if (im.kind == K_PAL) {
        memset(dst, 255, stride * im.h);
        rle_walk(data + p.data_off, p.data_len, im.w, im.h, p.rle == 4, covered, [&](uint32_t x, uint32_t y, uint32_t i) { dst[y * stride + x] = (uint8_t)i; });
    } else {
        memset(dst, 0, stride * im.h);
        rle_walk(data + p.data_off, p.data_len, im.w, im.h, p.rle == 4, covered, [&](uint32_t x, uint32_t y, uint32_t i) {
            const uint32_t c = i < im.pal_n ? p.pal[i] : 0;
            uint8_t *d = dst + y * stride + (size_t)x * 3;
            d[0] = (uint8_t)(c >> 16), d[1] = (uint8_t)(c >> 8), d[2] = (uint8_t)c;
        });
    }
}

int decode_host(const uint8_t *data, size_t len, Parsed &p, std::vector<uint8_t> &native)
{
    const int rc = parse(data, len, p);
    if (rc) return rc;
    const Image &im = p.im;
    const uint32_t ch = im.out_ch;
    native.assign((size_t)im.w * im.h * ch, 0);
    auto at = [&](uint32_t x, uint32_t y) { return native.data() + ((size_t)y * im.w + x) * ch; };
    auto put_rgb = [](uint8_t *d, uint32_t c) { d[0] = (uint8_t)c, d[1] = (uint8_t)(c >> 8), d[2] = (uint8_t)(c >> 16); };
    if (p.rle) {  // skipped pixels stay (0, 0, 0)
        uint64_t covered;
        rle_walk(data + p.data_off, p.data_len, im.w, im.h, p.rle == 4, covered,
                 [&](uint32_t x, uint32_t y, uint32_t i) { put_rgb(at(x, im.h - 1 - y), i < im.pal_n ? p.pal[i] : 0); });
        return RPH_OK;
    }
    const uint32_t bits = im.bits;
    for (uint32_t y = 0; y < im.h; y++) {
        const uint8_t *row = data + p.data_off + (size_t)(im.top_down ? y : im.h - 1 - y) * im.src_stride;
        for (uint32_t x = 0; x < im.w; x++) {
            uint8_t *d = at(x, y);
            if (im.kind == K_PAL) {
                const uint32_t bit = x * bits, i = (row[bit >> 3] >> (8 - bits - (bit & 7))) & ((1u << bits) - 1);
                put_rgb(d, i < im.pal_n ? p.pal[i] : 0);
            } else if (im.kind == K_BGR24) {
                d[0] = row[3 * x + 2], d[1] = row[3 * x + 1], d[2] = row[3 * x];
            } else {
                const uint32_t v = bits == 16 ? u16(row, 2 * (size_t)x) : u32(row, 4 * (size_t)x);
                for (uint32_t c = 0; c < ch; c++) d[c] = im.len[c] ? (uint8_t)scale_sample((v >> im.shift[c]) & ((1u << im.len[c]) - 1), im.len[c]) : 0;
            }
        }
    }
    return RPH_OK;
}

}  // namespace rphb
