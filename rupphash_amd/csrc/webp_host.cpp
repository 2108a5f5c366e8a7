// webp_host.cpp -- the host half of the WebP path: the RIFF container, the VP8L header, the serial front of the stream (transforms and
// their sub-images, colour table, colour cache, entropy image, the prefix codes of every group) and the whole decoder on the CPU
// (vp8l.h, the inverse transforms) for rph_webp_decode_host and the HOST entropy mode.  No libwebp, no HIP: tools/fuzz_webp_host.cpp
// builds this file with g++ under ASan + UBSan.
#include "webp_host.h"

#include <string.h>

#include <algorithm>

#include "../../include/rupphash.h"

namespace rphw {

namespace {

inline uint32_t le32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
inline uint32_t le24(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16); }

struct HostSink {
    uint32_t *out;
    uint64_t n;
    uint32_t *cache;  // nullptr: none
    uint32_t shift;
    void enter(uint32_t v)
    {
        if (cache) cache[(v * CACHE_MUL) >> shift] = v;
    }
    const uint16_t *group(const uint16_t *g, uint32_t, uint32_t) { return g; }
    void lit(uint32_t v)
    {
        out[n++] = v;
        enter(v);
    }
    void cached(uint32_t key) { lit(cache[key]); }
    void copy(uint32_t dist, uint32_t len)
    {
        for (uint32_t i = 0; i < len; i++, n++) {
            out[n] = out[n - dist];
            enter(out[n]);
        }
    }
};

bool run_stream(const Stream &s, Bits &br, uint32_t *out)
{
    std::vector<uint32_t> cache(s.cache_bits ? (size_t)1 << s.cache_bits : 0);
    HostSink sink{out, 0, s.cache_bits ? cache.data() : nullptr, 32 - s.cache_bits};
    return decode_pixels(s, br, sink) == W_OK;
}

// one prefix code of an alphabet of n symbols (n <= 2328) into the tables of a group
bool read_code(Bits &br, uint32_t n, uint16_t *fast, uint16_t *count, uint16_t *symbol)
{
    uint8_t lens[280 + 2048];
    memset(lens, 0, sizeof lens);
    if (br.take(1)) {  // simple: one or two symbols of 1 or 8 bits; a symbol at or past the alphabet is not part of the code
        const uint32_t two = br.take(1), first8 = br.take(1);
        lens[br.take(first8 ? 8 : 1)] = 1;
        if (two) lens[br.take(8)] = 1;
    } else {
        static const uint8_t order[19] = {17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};
        uint8_t cl[19] = {0};
        const uint32_t ncl = 4 + br.take(4);
        for (uint32_t i = 0; i < ncl; i++) cl[order[i]] = (uint8_t)br.take(3);
        uint16_t cfast[256], ccount[16], csym[19];
        if (!build_code(cl, 19, cfast, ccount, csym)) return false;
        uint32_t max_symbol = n;
        if (br.take(1)) {
            const uint32_t nbits = 2 + 2 * br.take(3);
            max_symbol = 2 + br.take(nbits);
            if (max_symbol > n) return false;
        }
        uint32_t s = 0, prev = 8;
        while (s < n && max_symbol--) {
            if (br.out_of_bits()) return false;
            const int c = read_symbol(cfast, ccount, csym, br);
            if (c < 0) return false;
            if (c < 16) {
                lens[s++] = (uint8_t)c;
                if (c) prev = (uint32_t)c;
                continue;
            }
            // 16: the last non-zero length (8 when there was none yet: the format's rule) 3-6 times; 17 / 18: zero 3-10 / 11-138 times
            const uint32_t rep = c == 16 ? 3 + br.take(2) : c == 17 ? 3 + br.take(3) : 11 + br.take(7);
            if (s + rep > n) return false;
            for (uint32_t k = 0; k < rep; k++) lens[s++] = (uint8_t)(c == 16 ? prev : 0);
        }
    }
    if (br.out_of_bits()) return false;
    return build_code(lens, n, fast, count, symbol);
}

// the five codes of a group into g[0 .. group_stride)
bool read_group(Bits &br, uint32_t cache_bits, uint16_t *g)
{
    const uint32_t green_n = green_symbols(cache_bits);
    for (uint32_t k = 0; k < 5; k++) {
        const uint32_t n = k == 0 ? green_n : k == 4 ? 40 : 256;
        if (!read_code(br, n, g + 256 * k, g + T_COUNT + 16 * k, g + T_SYM + symbol_offset(k, green_n))) return false;
    }
    return true;
}

bool read_cache_bits(Bits &br, uint32_t &cache_bits)
{
    cache_bits = 0;
    if (br.take(1)) {
        cache_bits = br.take(4);
        if (cache_bits < 1 || cache_bits > 11) return false;
    }
    return true;
}

// a sub-image (transform data, colour table, entropy image): optional colour cache, one group, the pixels
bool read_sub_image(Bits &br, uint32_t xsize, uint32_t ysize, uint32_t *out)
{
    uint32_t cache_bits;
    if (!read_cache_bits(br, cache_bits)) return false;
    std::vector<uint16_t> g(group_stride(cache_bits));
    if (!read_group(br, cache_bits, g.data())) return false;
    const Stream s{xsize, ysize, cache_bits, 0, nullptr, g.data()};
    return run_stream(s, br, out);
}

void inverse_predictor(const Xform &t, const uint32_t *modes, uint32_t h, uint32_t *px)
{
    const uint32_t w = t.xsize, bw = subsample(w, t.bits);
    for (uint32_t y = 0; y < h; y++) {
        uint32_t *row = px + (size_t)y * w;
        const uint32_t *up = row - w;
        for (uint32_t x = 0; x < w; x++) {
            uint32_t p;
            if (y == 0)
                p = x == 0 ? 0xff000000u : row[x - 1];
            else if (x == 0)
                p = up[0];
            else
                p = predict((modes[(size_t)(y >> t.bits) * bw + (x >> t.bits)] >> 8) & 15, row[x - 1], up[x], up[x - 1], x + 1 < w ? up[x + 1] : row[0]);
            row[x] = add_pixels(row[x], p);
        }
    }
}

}  // namespace

int parse(const uint8_t *data, size_t len, Parsed &p)
{
    p = Parsed();
    if (len < 12 || memcmp(data, "RIFF", 4) || memcmp(data + 8, "WEBP", 4)) return RPH_ERR_INVALID_ARG;
    // the RIFF size rules where it is smaller than the file (what lies behind it is not read); one that reaches past the file is refused
    const uint64_t riff_end = (uint64_t)le32(data + 4) + 8;
    if (riff_end > len || riff_end < 12) return RPH_ERR_INVALID_ARG;
    size_t o = 12;
    bool vp8x = false;
    uint32_t canvas_w = 0, canvas_h = 0;
    for (;;) {
        if (o == riff_end) return RPH_ERR_INVALID_ARG;  // no image chunk
        if (riff_end - o < 8) return RPH_ERR_INVALID_ARG;
        const uint8_t *tag = data + o;
        const uint64_t size = le32(data + o + 4);
        if (size > riff_end - o - 8) return RPH_ERR_INVALID_ARG;
        if (!memcmp(tag, "VP8 ", 4) || !memcmp(tag, "ALPH", 4) || !memcmp(tag, "ANIM", 4) || !memcmp(tag, "ANMF", 4)) return RPH_ERR_UNSUPPORTED;
        if (!memcmp(tag, "VP8X", 4) && o == 12) {
            if (size < 10) return RPH_ERR_INVALID_ARG;
            if (data[o + 8] & 0x02) return RPH_ERR_UNSUPPORTED;  // animation
            vp8x = true;
            canvas_w = le24(data + o + 12) + 1;
            canvas_h = le24(data + o + 15) + 1;
        }
        if (!memcmp(tag, "VP8L", 4)) {
            p.chunk = data + o + 8;
            p.chunk_len = (size_t)size;
            break;
        }
        o += 8 + (size_t)((size + 1) & ~(uint64_t)1);
        if (o > riff_end) return RPH_ERR_INVALID_ARG;
    }
    if (p.chunk_len < 5 || p.chunk[0] != 0x2f) return RPH_ERR_INVALID_ARG;
    const uint32_t v = le32(p.chunk + 1);
    if (v >> 29) return RPH_ERR_INVALID_ARG;  // version
    Image &im = p.im;
    memset(&im, 0, sizeof im);
    im.w = (v & 0x3fff) + 1;
    im.h = ((v >> 14) & 0x3fff) + 1;
    if (vp8x && (canvas_w != im.w || canvas_h != im.h)) return RPH_ERR_INVALID_ARG;
    if ((uint64_t)im.w * im.h > MAX_PIXELS) return RPH_ERR_UNSUPPORTED;
    // the VP8L header's alpha_is_used bit rules in both container forms (libwebp: VP8LGetInfo has the last word)
    im.out_ch = ((v >> 28) & 1) ? 4 : 3;
    im.hc = im.out_ch;
    im.out_depth = 8;
    im.xw = im.w;
    im.hp_off = im.x16_off = im.nat_off = im.a_off = im.b_off = NONE;
    return RPH_OK;
}

int front(const uint8_t *data, size_t len, Parsed &p)
{
    const int rc = parse(data, len, p);
    if (rc) return rc;
    Image &im = p.im;
    Bits br;
    br.start(p.chunk, p.chunk_len, 40);
    uint32_t seen = 0, xsize = im.w;
    while (br.take(1)) {
        const uint32_t type = br.take(2);
        if (seen & (1u << type)) return RPH_ERR_INVALID_ARG;
        seen |= 1u << type;
        Xform t{type, 0, xsize, (uint32_t)p.words.size()};
        if (type == TR_PREDICTOR || type == TR_CROSS_COLOUR) {
            t.bits = br.take(3) + 2;
            const uint32_t bw = subsample(xsize, t.bits), bh = subsample(im.h, t.bits);
            p.words.resize(p.words.size() + (size_t)bw * bh);
            if (!read_sub_image(br, bw, bh, p.words.data() + t.off)) return RPH_ERR_INVALID_ARG;
        } else if (type == TR_COLOUR_INDEXING) {
            const uint32_t n = br.take(8) + 1;
            t.bits = n > 16 ? 0 : n > 4 ? 1 : n > 2 ? 2 : 3;
            p.words.resize(p.words.size() + 256, 0);
            uint32_t *pal = p.words.data() + t.off;
            if (!read_sub_image(br, n, 1, pal)) return RPH_ERR_INVALID_ARG;
            for (uint32_t k = 1; k < n; k++) pal[k] = add_pixels(pal[k], pal[k - 1]);
            xsize = subsample(xsize, t.bits);
        }
        if (br.out_of_bits()) return RPH_ERR_INVALID_ARG;
        im.tr[im.n_tr++] = t;
    }
    im.xw = xsize;
    if (!read_cache_bits(br, im.cache_bits)) return RPH_ERR_INVALID_ARG;
    const uint32_t stride = group_stride(im.cache_bits);
    std::vector<uint32_t> map;  // group named by the stream -> its tables here (only groups that a block uses are kept), or ~0
    im.n_groups = 1;
    if (br.take(1)) {
        im.meta_bits = br.take(3) + 2;
        im.has_ent = 1;
        const uint32_t bw = subsample(xsize, im.meta_bits), bh = subsample(im.h, im.meta_bits);
        std::vector<uint32_t> ent((size_t)bw * bh);
        if (!read_sub_image(br, bw, bh, ent.data())) return RPH_ERR_INVALID_ARG;
        uint32_t top = 0;
        for (uint32_t &e : ent) e = (e >> 8) & 0xffff, top = std::max(top, e);
        map.assign((size_t)top + 1, ~0u);
        for (uint32_t e : ent) map[e] = 0;
        uint32_t used = 0;
        for (uint32_t &m : map)
            if (m == 0) m = used++;
        im.n_groups = used;
        if ((uint64_t)used * stride * 2 > MAX_TABLE_BYTES) return RPH_ERR_UNSUPPORTED;
        im.ent_off = 0;
        p.codes.resize(ent.size());
        for (size_t k = 0; k < ent.size(); k++) p.codes[k] = (uint16_t)map[ent[k]];
    } else {
        map.assign(1, 0);
    }
    if (br.out_of_bits()) return RPH_ERR_INVALID_ARG;
    im.tab_off = (p.codes.size() + 1) & ~(size_t)1;
    p.codes.resize(im.tab_off + (size_t)im.n_groups * stride);
    std::vector<uint16_t> unused(stride);
    for (size_t g = 0; g < map.size(); g++)  // every group the stream holds is read and checked, used or not
        if (!read_group(br, im.cache_bits, map[g] == ~0u ? unused.data() : p.codes.data() + im.tab_off + (size_t)map[g] * stride)) return RPH_ERR_INVALID_ARG;
    im.bit_start = br.used;
    return RPH_OK;
}

bool decode_main_host(const Parsed &p, uint32_t *argb)
{
    const Image &im = p.im;
    const Stream s{im.xw, im.h, im.cache_bits, im.meta_bits, im.has_ent ? p.codes.data() + im.ent_off : nullptr, p.codes.data() + im.tab_off};
    Bits br;
    br.start(p.chunk, p.chunk_len, im.bit_start);
    return run_stream(s, br, argb);
}

int decode_host(const uint8_t *data, size_t len, Parsed &p, std::vector<uint8_t> &native)
{
    const int rc = front(data, len, p);
    if (rc) return rc;
    const Image &im = p.im;
    std::vector<uint32_t> px((size_t)im.xw * im.h), tmp;
    if (!decode_main_host(p, px.data())) return RPH_ERR_INVALID_ARG;
    for (int k = (int)im.n_tr - 1; k >= 0; k--) {
        const Xform &t = im.tr[k];
        const uint32_t *aux = p.words.data() + t.off;
        const uint32_t bw = subsample(t.xsize, t.bits);
        if (t.type == TR_PREDICTOR) {
            inverse_predictor(t, aux, im.h, px.data());
        } else if (t.type == TR_CROSS_COLOUR) {
            for (uint32_t y = 0; y < im.h; y++)
                for (uint32_t x = 0; x < t.xsize; x++) {
                    uint32_t &v = px[(size_t)y * t.xsize + x];
                    v = cross_colour(aux[(size_t)(y >> t.bits) * bw + (x >> t.bits)], v);
                }
        } else if (t.type == TR_SUBTRACT_GREEN) {
            for (uint32_t &v : px) v = add_green(v);
        } else {
            tmp.resize((size_t)t.xsize * im.h);
            for (uint32_t y = 0; y < im.h; y++)
                for (uint32_t x = 0; x < t.xsize; x++) tmp[(size_t)y * t.xsize + x] = aux[bundled_index(px[(size_t)y * bw + (x >> t.bits)], x, t.bits)];
            px.swap(tmp);
        }
    }
    native.resize((size_t)im.w * im.h * im.out_ch);
    uint8_t *o = native.data();
    for (uint32_t v : px) {
        *o++ = (uint8_t)(v >> 16);
        *o++ = (uint8_t)(v >> 8);
        *o++ = (uint8_t)v;
        if (im.out_ch == 4) *o++ = (uint8_t)(v >> 24);
    }
    return RPH_OK;
}

}  // namespace rphw
