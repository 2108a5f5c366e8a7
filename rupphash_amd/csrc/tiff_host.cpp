// tiff_host.cpp -- the host half of the TIFF path: header and first IFD, validation of every offset and size into a table of segments
// (strips or tiles), the plausibility bounds, and the whole decoder on the CPU (tiff_lzw.h, inflate.h, predictor, expansion) for
// rph_tiff_decode_host and the HOST decompress mode.  No libtiff, no zlib, no HIP: tools/fuzz_tiff_host.cpp builds this file with g++
// under ASan + UBSan.
#include "tiff_host.h"

#include <string.h>

#include "../../include/rupphash.h"

namespace rpht {

namespace {

struct Field {
    bool present = false;
    std::vector<uint64_t> v;
};

struct Reader {
    const uint8_t *d;
    size_t len;
    bool be;
    uint32_t u16(size_t o) const { return be ? ((uint32_t)d[o] << 8) | d[o + 1] : ((uint32_t)d[o + 1] << 8) | d[o]; }
    uint32_t u32(size_t o) const
    {
        return be ? ((uint32_t)d[o] << 24) | ((uint32_t)d[o + 1] << 16) | ((uint32_t)d[o + 2] << 8) | d[o + 3]
                  : ((uint32_t)d[o + 3] << 24) | ((uint32_t)d[o + 2] << 16) | ((uint32_t)d[o + 1] << 8) | d[o];
    }
};

// the tags that are read; every other tag (ExtraSamples, Orientation, ...) is ignored
enum : uint32_t {
    T_WIDTH = 256, T_LENGTH = 257, T_BPS = 258, T_COMPRESSION = 259, T_PHOTOMETRIC = 262, T_FILLORDER = 266, T_STRIPOFFSETS = 273, T_SPP = 277,
    T_ROWSPERSTRIP = 278, T_STRIPBYTECOUNTS = 279, T_PLANAR = 284, T_PREDICTOR = 317, T_TILEWIDTH = 322, T_TILELENGTH = 323, T_TILEOFFSETS = 324,
    T_TILEBYTECOUNTS = 325, T_SAMPLEFORMAT = 339,
};
constexpr uint32_t TAGS[] = {T_WIDTH, T_LENGTH, T_BPS, T_COMPRESSION, T_PHOTOMETRIC, T_FILLORDER, T_STRIPOFFSETS, T_SPP, T_ROWSPERSTRIP, T_STRIPBYTECOUNTS,
                             T_PLANAR, T_PREDICTOR, T_TILEWIDTH, T_TILELENGTH, T_TILEOFFSETS, T_TILEBYTECOUNTS, T_SAMPLEFORMAT};
constexpr int N_TAGS = sizeof TAGS / sizeof TAGS[0];
inline bool is_array_tag(uint32_t t)
{
    return t == T_BPS || t == T_STRIPOFFSETS || t == T_STRIPBYTECOUNTS || t == T_TILEOFFSETS || t == T_TILEBYTECOUNTS || t == T_SAMPLEFORMAT;
}

}  // namespace

int parse(const uint8_t *d, size_t len, Parsed &p)
{
    Image &im = p.im;
    memset(&im, 0, sizeof im);
    p.segs.clear();
    p.comp_bytes = 0;
    if (!d || len < 8) return RPH_ERR_INVALID_ARG;
    Reader r{d, len, false};
    if (d[0] == 'M' && d[1] == 'M')
        r.be = true;
    else if (!(d[0] == 'I' && d[1] == 'I'))
        return RPH_ERR_INVALID_ARG;
    const uint32_t version = r.u16(2);
    if (version == 43) return RPH_ERR_UNSUPPORTED;  // BigTIFF
    if (version != 42) return RPH_ERR_INVALID_ARG;
    const size_t ifd = r.u32(4);
    if (ifd > len || len - ifd < 2) return RPH_ERR_INVALID_ARG;
    const size_t n_entries = r.u16(ifd);
    if ((len - ifd - 2) / 12 < n_entries) return RPH_ERR_INVALID_ARG;
    Field f[N_TAGS];
    auto field = [&](uint32_t tag) -> Field & {
        int k = 0;
        while (TAGS[k] != tag) k++;
        return f[k];
    };
    for (size_t e = 0; e < n_entries; e++) {
        const size_t at = ifd + 2 + 12 * e;
        const uint32_t tag = r.u16(at), type = r.u16(at + 2), count = r.u32(at + 4);
        bool read = false;
        for (int k = 0; k < N_TAGS; k++) read |= TAGS[k] == tag;
        if (!read) continue;
        if ((type != 3 && type != 4) || count == 0 || (!is_array_tag(tag) && count != 1)) return RPH_ERR_INVALID_ARG;
        const size_t size = (size_t)count * (type == 3 ? 2 : 4);
        size_t off = at + 8;
        if (size > 4) {
            off = r.u32(at + 8);
            if (off > len || len - off < size) return RPH_ERR_INVALID_ARG;
        }
        Field &fl = field(tag);  // (a tag that comes twice: the last one counts)
        fl.present = true;
        fl.v.resize(count);
        for (uint32_t k = 0; k < count; k++) fl.v[k] = type == 3 ? r.u16(off + 2 * (size_t)k) : r.u32(off + 4 * (size_t)k);
    }
    auto scalar = [&](uint32_t tag, uint64_t dflt) { return field(tag).present ? field(tag).v[0] : dflt; };
    if (!field(T_WIDTH).present || !field(T_LENGTH).present) return RPH_ERR_INVALID_ARG;
    const uint64_t w = scalar(T_WIDTH, 0), h = scalar(T_LENGTH, 0);
    if (w == 0 || h == 0) return RPH_ERR_INVALID_ARG;
    const uint64_t spp = scalar(T_SPP, 1), comp = scalar(T_COMPRESSION, 1), planar = scalar(T_PLANAR, 1), fill = scalar(T_FILLORDER, 1),
                   pred = scalar(T_PREDICTOR, 1);
    std::vector<uint64_t> bps = field(T_BPS).present ? field(T_BPS).v : std::vector<uint64_t>{1};
    if (spp == 0 || bps.size() != spp) return RPH_ERR_INVALID_ARG;
    const uint64_t photo = scalar(T_PHOTOMETRIC, spp <= 2 ? 1 : 2);
    // what is left to the caller's decoders
    if (comp != 1 && comp != 5 && comp != 8 && comp != 32946 && comp != 32773) return RPH_ERR_UNSUPPORTED;
    if (fill != 1) return RPH_ERR_UNSUPPORTED;
    if (planar != 1 && spp > 1) return RPH_ERR_UNSUPPORTED;
    if (photo > 2) return RPH_ERR_UNSUPPORTED;
    for (uint64_t b : bps)
        if (b != bps[0]) return RPH_ERR_UNSUPPORTED;
    if (field(T_SAMPLEFORMAT).present)
        for (uint64_t s : field(T_SAMPLEFORMAT).v)
            if (s != 1) return RPH_ERR_UNSUPPORTED;
    if (photo == 2 ? (spp != 3 && spp != 4) : (spp != 1 && spp != 2)) return RPH_ERR_UNSUPPORTED;
    const uint64_t b = bps[0];
    if (spp == 1 ? !(b == 1 || b == 2 || b == 4 || b == 8 || b == 16) : !(b == 8 || b == 16)) return RPH_ERR_UNSUPPORTED;
    if (pred != 1 && (pred != 2 || comp == 1 || comp == 32773 || b < 8)) return RPH_ERR_UNSUPPORTED;
    // geometry
    const bool tiled = field(T_TILEWIDTH).present || field(T_TILELENGTH).present || field(T_TILEOFFSETS).present;
    uint64_t seg_w, seg_h;
    if (tiled) {
        if (!field(T_TILEWIDTH).present || !field(T_TILELENGTH).present || !field(T_TILEOFFSETS).present) return RPH_ERR_INVALID_ARG;
        seg_w = scalar(T_TILEWIDTH, 0);
        seg_h = scalar(T_TILELENGTH, 0);
        if (seg_w == 0 || seg_h == 0) return RPH_ERR_INVALID_ARG;
    } else {
        if (!field(T_STRIPOFFSETS).present) return RPH_ERR_INVALID_ARG;
        seg_w = w;
        seg_h = scalar(T_ROWSPERSTRIP, h);
        if (seg_h == 0) return RPH_ERR_INVALID_ARG;
        if (seg_h > h) seg_h = h;
    }
    const uint64_t segs_x = (w + seg_w - 1) / seg_w, segs_y = (h + seg_h - 1) / seg_h;
    // the size limits, before anything is allocated
    if (w * h > MAX_PIXELS) return RPH_ERR_UNSUPPORTED;
    const uint64_t seg_rb = (seg_w * spp * b + 7) / 8;  // (seg_w < 2^32, spp <= 4, b <= 16: below 2^38)
    if (seg_rb > MAX_DEC_BYTES) return RPH_ERR_UNSUPPORTED;
    const uint64_t seg_bytes = seg_h * seg_rb;          // (below 2^62)
    if (seg_bytes > MAX_DEC_BYTES) return RPH_ERR_UNSUPPORTED;
    const uint64_t n_segs = segs_x * segs_y;            // (at most w * h)
    if ((tiled ? n_segs * seg_bytes : h * seg_rb) > MAX_DEC_BYTES) return RPH_ERR_UNSUPPORTED;
    const Field &offs = field(tiled ? T_TILEOFFSETS : T_STRIPOFFSETS), &cnts = field(tiled ? T_TILEBYTECOUNTS : T_STRIPBYTECOUNTS);
    if (offs.v.size() != n_segs) return RPH_ERR_INVALID_ARG;
    if (cnts.present ? cnts.v.size() != n_segs : comp != 1) return RPH_ERR_INVALID_ARG;
    im.w = (uint32_t)w;
    im.h = (uint32_t)h;
    im.comp = (uint16_t)(comp == 32946 ? 8 : comp);
    im.photo = (uint8_t)photo;
    im.spp = (uint8_t)spp;
    im.bps = (uint8_t)b;
    im.predictor = (uint8_t)pred;
    im.big_endian = r.be;
    im.tiled = tiled;
    im.out_ch = (uint8_t)spp;
    im.out_depth = b == 16 ? 16 : 8;
    im.hc = rphx::hasher_channels(im.out_ch, im.out_depth);
    im.seg_w = (uint32_t)seg_w;
    im.seg_h = (uint32_t)seg_h;
    im.segs_x = (uint32_t)segs_x;
    im.segs_y = (uint32_t)segs_y;
    im.seg_rb = (uint32_t)seg_rb;
    im.n_segs = (uint32_t)n_segs;
    im.seg_slot = (seg_bytes + 15) / 16 * 16;
    im.dec_bytes = n_segs * im.seg_slot;
    im.hp_off = im.x16_off = im.nat_off = NONE;
    p.segs.resize(n_segs);
    for (uint64_t k = 0; k < n_segs; k++) {
        Segment &s = p.segs[k];
        const uint64_t rows = tiled ? seg_h : (k + 1 == n_segs ? h - k * seg_h : seg_h);
        s.dec_bytes = rows * seg_rb;
        s.dec_off = k * im.seg_slot;
        s.src_off = offs.v[k];
        s.src_len = cnts.present ? cnts.v[k] : s.dec_bytes;
        s.comp_off = p.comp_bytes;
        s.image = s.pad = 0;
        if (s.src_off > len || s.src_len > len - s.src_off) return RPH_ERR_INVALID_ARG;
        p.comp_bytes += (s.src_len + 3) / 4 * 4;
    }
    for (const Segment &s : p.segs)
        if (s.dec_bytes > max_expansion(im.comp, s.src_len)) return RPH_ERR_UNSUPPORTED;
    return RPH_OK;
}

bool decompress_host(uint32_t comp, const uint8_t *in, size_t n, uint8_t *out, uint64_t dec_bytes)
{
    switch (comp) {
    case 1: memcpy(out, in, dec_bytes); return true;  // (parse: n >= dec_bytes)
    case 5: {
        LzwTable t;
        HostSegSink s{out, dec_bytes};
        return lzw_decode(in, n, t, s) == L_OK;
    }
    case 8: return rphz::inflate_host(in, n, out, dec_bytes) == rphz::Z_OK;
    default: {
        HostSegSink s{out, dec_bytes};
        return packbits_decode(in, n, s) == L_OK;
    }
    }
}

int decode_host(const uint8_t *data, size_t len, Parsed &p, std::vector<uint8_t> &native)
{
    int rc = parse(data, len, p);
    if (rc) return rc;
    const Image &im = p.im;
    std::vector<uint8_t> dec(im.dec_bytes);
    for (const Segment &s : p.segs)
        if (!decompress_host(im.comp, data + s.src_off, s.src_len, dec.data() + s.dec_off, s.dec_bytes)) return RPH_ERR_INVALID_ARG;
    const size_t bytes = im.out_depth / 8;
    const uint32_t mask = (1u << im.bps) - 1;
    native.assign((size_t)im.w * im.h * im.out_ch * bytes, 0);
    for (uint32_t y = 0; y < im.h; y++)
        for (uint32_t sx = 0; sx < im.segs_x; sx++) {
            const uint8_t *row = dec.data() + ((uint64_t)(y / im.seg_h) * im.segs_x + sx) * im.seg_slot + (uint64_t)(y % im.seg_h) * im.seg_rb;
            uint32_t acc[4] = {0, 0, 0, 0};
            for (uint32_t px = 0; px < im.seg_w; px++) {
                const uint32_t x = sx * im.seg_w + px;
                if (x >= im.w) break;
                for (uint32_t c = 0; c < im.spp; c++) {
                    uint32_t v = stored_sample(im, row, px, c);
                    if (im.predictor == 2) v = acc[c] = (acc[c] + v) & mask;
                    v = native_sample(im, v);
                    const size_t o = ((size_t)y * im.w + x) * im.out_ch + c;
                    if (bytes == 1)
                        native[o] = (uint8_t)v;
                    else {
                        const uint16_t s = (uint16_t)v;
                        memcpy(&native[o * 2], &s, 2);
                    }
                }
            }
        }
    return RPH_OK;
}

}  // namespace rpht
