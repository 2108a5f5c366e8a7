// gif_host.cpp -- the host half of the GIF path: signature, logical screen, colour tables, the blocks before the first image descriptor,
// the sub-block chain of the first frame's data, the plausibility bounds, and the whole decoder on the CPU (gif_lzw.h, the pixel rule of
// gif_host.h) for rph_gif_decode_host and the HOST decompress mode.  No giflib, no HIP: tools/fuzz_gif_host.cpp builds this file with g++
// under ASan + UBSan.
#include "gif_host.h"

#include <string.h>

#include "../../include/rupphash.h"

namespace rphg {

namespace {

inline uint32_t u16(const uint8_t *d, size_t o) { return (uint32_t)d[o] | ((uint32_t)d[o + 1] << 8); }

// a colour table of n entries at d: R | G << 8 | B << 16
void read_table(const uint8_t *d, uint32_t n, uint32_t *pal)
{
    for (uint32_t i = 0; i < n; i++) pal[i] = (uint32_t)d[3 * i] | ((uint32_t)d[3 * i + 1] << 8) | ((uint32_t)d[3 * i + 2] << 16);
}

}  // namespace

// The checks run in file order, and the first that fails decides the status (include/rupphash.h, GIF section)
int parse(const uint8_t *data, size_t len, Parsed &p)
{
    Image &im = p.im;
    memset(&im, 0, sizeof im);
    im.out_ch = 4, im.out_depth = 8, im.hc = 4;
    im.hp_off = im.x16_off = im.nat_off = NONE;
    if (len < 6 || (memcmp(data, "GIF87a", 6) != 0 && memcmp(data, "GIF89a", 6) != 0)) return RPH_ERR_INVALID_ARG;
    if (len < 13) return RPH_ERR_INVALID_ARG;
    im.w = u16(data, 6), im.h = u16(data, 8);
    if (!im.w || !im.h) return RPH_ERR_INVALID_ARG;
    if ((uint64_t)im.w * im.h > MAX_PIXELS) return RPH_ERR_UNSUPPORTED;
    size_t pos = 13;
    bool have_table = false;
    if (data[10] & 0x80) {
        const uint32_t n = 2u << (data[10] & 7);
        if (len - pos < 3 * (size_t)n) return RPH_ERR_INVALID_ARG;
        read_table(data + pos, n, p.pal);
        im.pal_n = (uint16_t)n;
        have_table = true;
        pos += 3 * (size_t)n;
    }
    // blocks before the first image descriptor: extensions are skipped by their sub-blocks, the last Graphic Control Extension counts
    for (;;) {
        if (pos >= len) return RPH_ERR_INVALID_ARG;  // no image descriptor before the end of the file
        const uint8_t intro = data[pos++];
        if (intro == 0x2c) break;
        if (intro != 0x21) return RPH_ERR_INVALID_ARG;  // the trailer (0x3b), or no block at all
        if (pos >= len) return RPH_ERR_INVALID_ARG;
        const uint8_t label = data[pos++];
        for (bool first = true;; first = false) {
            if (pos >= len) return RPH_ERR_INVALID_ARG;
            const size_t sz = data[pos++];
            if (!sz) break;
            if (len - pos < sz) return RPH_ERR_INVALID_ARG;
            if (label == 0xf9 && first && sz == 4) {
                im.has_trans = data[pos] & 1;
                im.trans = data[pos + 3];
            }
            pos += sz;
        }
    }
    if (len - pos < 9) return RPH_ERR_INVALID_ARG;
    im.fx = u16(data, pos), im.fy = u16(data, pos + 2), im.fw = u16(data, pos + 4), im.fh = u16(data, pos + 6);
    const uint8_t flags = data[pos + 8];
    pos += 9;
    if (!im.fw || !im.fh) return RPH_ERR_INVALID_ARG;
    im.interlaced = (flags & 0x40) != 0;
    if (flags & 0x80) {
        const uint32_t n = 2u << (flags & 7);
        if (len - pos < 3 * (size_t)n) return RPH_ERR_INVALID_ARG;
        read_table(data + pos, n, p.pal);
        im.pal_n = (uint16_t)n;
        have_table = true;
        pos += 3 * (size_t)n;
    }
    if (!have_table) return RPH_ERR_INVALID_ARG;
    if (pos >= len) return RPH_ERR_INVALID_ARG;  // (the code size byte opens the sub-block chain)
    im.m = data[pos++];
    if (im.m < LZW_MIN_CODE_SIZE || im.m > LZW_MAX_CODE_SIZE) return RPH_ERR_UNSUPPORTED;
    // the data sub-blocks up to the zero-length one; a file that ends on a sub-block boundary ends the chain as well
    p.data_off = pos;
    p.stream_len = 0;
    while (pos < len) {
        const size_t sz = data[pos++];
        if (!sz) break;
        if (len - pos < sz) return RPH_ERR_INVALID_ARG;
        p.stream_len += sz;
        pos += sz;
    }
    const uint64_t indices = (uint64_t)im.fw * im.fh;
    if (indices > MAX_PIXELS || indices > lzw_max_expansion(im.m, p.stream_len)) return RPH_ERR_UNSUPPORTED;
    im.comp_len = p.stream_len;
    return RPH_OK;
}

void join(const uint8_t *data, const Parsed &p, uint8_t *dst)
{
    size_t pos = p.data_off;
    for (uint64_t done = 0; done < p.stream_len;) {
        const size_t sz = data[pos++];
        memcpy(dst + done, data + pos, sz);
        done += sz;
        pos += sz;
    }
}

bool decode_indices_host(const uint8_t *stream, size_t n, const Image &im, uint8_t *out)
{
    LzwTable t;
    HostSink s{out, (uint64_t)im.fw * im.fh};
    return lzw_decode(stream, n, im.m, t, s) == L_OK;
}

int decode_host(const uint8_t *data, size_t len, Parsed &p, std::vector<uint8_t> &native)
{
    const int rc = parse(data, len, p);
    if (rc) return rc;
    const Image &im = p.im;
    std::vector<uint8_t> stream(p.stream_len), idx((size_t)im.fw * im.fh);
    join(data, p, stream.data());
    if (!decode_indices_host(stream.data(), stream.size(), im, idx.data())) return RPH_ERR_INVALID_ARG;
    native.resize((size_t)im.w * im.h * 4);
    for (uint32_t y = 0; y < im.h; y++)
        for (uint32_t x = 0; x < im.w; x++) {
            const uint32_t v = screen_pixel(im, p.pal, idx.data(), x, y);
            uint8_t *d = native.data() + ((size_t)y * im.w + x) * 4;
            d[0] = (uint8_t)v, d[1] = (uint8_t)(v >> 8), d[2] = (uint8_t)(v >> 16), d[3] = (uint8_t)(v >> 24);
        }
    return RPH_OK;
}

}  // namespace rphg
