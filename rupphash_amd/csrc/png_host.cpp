// png_host.cpp -- the host half of the PNG path: chunk parsing (signature, CRC-32, IHDR / PLTE / tRNS, the IDAT payloads), the
// plausibility bound, and the whole decoder on the CPU (inflate.h + unfilter + EXPAND) for rph_png_decode_host and the HOST inflate
// mode.  No zlib, no HIP: tools/fuzz_png_host.cpp builds this file with g++ under ASan + UBSan.
#include "png_host.h"

#include <string.h>

#include "../../include/rupphash.h"

namespace rphp {

namespace {
struct CrcTable {
    uint32_t t[8][256];
    CrcTable()
    {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            t[0][i] = c;
        }
        for (uint32_t i = 0; i < 256; i++)
            for (int k = 1; k < 8; k++) t[k][i] = (t[k - 1][i] >> 8) ^ t[0][t[k - 1][i] & 0xFF];
    }
};
const CrcTable &crc_table()
{
    static const CrcTable t;
    return t;
}
inline uint32_t be32(const uint8_t *p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }
inline bool is_type(const uint8_t *p, const char *s) { return memcmp(p, s, 4) == 0; }
}  // namespace

uint32_t crc32(const uint8_t *p, size_t n, uint32_t c)
{
    const CrcTable &T = crc_table();
    c = ~c;
    while (n >= 8) {  // slicing by eight
        const uint32_t a = c ^ ((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24));
        c = T.t[7][a & 0xFF] ^ T.t[6][(a >> 8) & 0xFF] ^ T.t[5][(a >> 16) & 0xFF] ^ T.t[4][a >> 24] ^ T.t[3][p[4]] ^ T.t[2][p[5]] ^ T.t[1][p[6]] ^
            T.t[0][p[7]];
        p += 8;
        n -= 8;
    }
    while (n--) c = T.t[0][(c ^ *p++) & 0xFF] ^ (c >> 8);
    return ~c;
}

static bool ihdr_ok(uint32_t depth, uint32_t ctype)
{
    switch (ctype) {
    case 0: return depth == 1 || depth == 2 || depth == 4 || depth == 8 || depth == 16;
    case 3: return depth == 1 || depth == 2 || depth == 4 || depth == 8;
    case 2:
    case 4:
    case 6: return depth == 8 || depth == 16;
    default: return false;
    }
}

int parse(const uint8_t *d, size_t len, Parsed &p)
{
    static const uint8_t sig[8] = {137, 80, 78, 71, 13, 10, 26, 10};
    if (!d || len < 8 || memcmp(d, sig, 8) != 0) return RPH_ERR_INVALID_ARG;
    Image &im = p.im;
    memset(&im, 0, sizeof im);
    memset(p.palette, 0, sizeof p.palette);
    p.idat.clear();
    p.idat_bytes = 0;
    bool have_ihdr = false, have_plte = false, seen_idat = false;
    size_t pos = 8;
    // a chunk that runs past the end of the file ends the parse like IEND: whatever the IDAT payloads hold must then verify
    while (len - pos >= 12) {
        const uint32_t n = be32(d + pos);
        const uint8_t *type = d + pos + 4;
        if (n > 0x7FFFFFFFu || (size_t)n > len - pos - 12) break;
        const uint8_t *body = d + pos + 8;
        if (is_type(type, "IEND")) break;
        if (crc32(type, (size_t)n + 4) != be32(body + n)) return RPH_ERR_INVALID_ARG;
        if (!have_ihdr) {
            if (!is_type(type, "IHDR") || n != 13) return RPH_ERR_INVALID_ARG;
            im.w = be32(body);
            im.h = be32(body + 4);
            im.depth = body[8];
            im.ctype = body[9];
            im.interlace = body[12];
            if (im.w == 0 || im.h == 0 || im.w > 0x7FFFFFFFu || im.h > 0x7FFFFFFFu || !ihdr_ok(im.depth, im.ctype) || body[10] != 0 || body[11] != 0 ||
                im.interlace > 1)
                return RPH_ERR_INVALID_ARG;
            have_ihdr = true;
        } else if (is_type(type, "IHDR")) {
            return RPH_ERR_INVALID_ARG;
        } else if (is_type(type, "PLTE")) {
            if (have_plte || n == 0 || n % 3 || n > 768) return RPH_ERR_INVALID_ARG;
            have_plte = true;
            if (im.ctype == 2 || im.ctype == 3 || im.ctype == 6) {  // (a suggested palette of a truecolour image is not used)
                memcpy(p.palette, body, n);
                im.plte_n = (uint16_t)(n / 3);
            }
        } else if (is_type(type, "tRNS")) {
            // a tRNS of the wrong size for its colour type (or in types 4 / 6, which have alpha) is ignored
            if (im.ctype == 0 && n == 2) {
                im.has_trns = 1;
                im.key[0] = (uint16_t)((body[0] << 8) | body[1]);
            } else if (im.ctype == 2 && n == 6) {
                im.has_trns = 1;
                for (int c = 0; c < 3; c++) im.key[c] = (uint16_t)((body[2 * c] << 8) | body[2 * c + 1]);
            } else if (im.ctype == 3 && n >= 1 && n <= 256) {
                im.has_trns = 1;
                im.trns_n = (uint16_t)n;
                memcpy(p.palette + 768, body, n);
            }
        } else if (is_type(type, "IDAT")) {
            seen_idat = true;
            if (n) p.idat.emplace_back(pos + 8, (size_t)n);
            p.idat_bytes += n;
        } else if (!(type[0] & 0x20)) {
            return RPH_ERR_INVALID_ARG;  // an unknown critical chunk
        }
        pos += (size_t)n + 12;
    }
    (void)seen_idat;
    if (!have_ihdr) return RPH_ERR_INVALID_ARG;
    if (im.ctype == 3 && !have_plte) return RPH_ERR_INVALID_ARG;
    if (im.ctype == 3 && im.trns_n > im.plte_n) im.trns_n = im.plte_n;  // entries past the palette have nothing to apply to
    const uint32_t nch = im.ctype == 0 || im.ctype == 3 ? 1 : im.ctype == 2 ? 3 : im.ctype == 4 ? 2 : 4;
    im.bpp_bits = nch * im.depth;
    im.unit = (uint8_t)(im.bpp_bits < 8 ? 1 : im.bpp_bits / 8);
    uint64_t raw = 0;
    for (int k = 0; k < 7; k++) {
        uint32_t x0 = 0, y0 = 0, dx = 1, dy = 1;
        if (im.interlace) adam7(k, x0, y0, dx, dy);
        const bool used = im.interlace || k == 0;
        const uint32_t pw = used && im.w > x0 ? (im.w - x0 + dx - 1) / dx : 0, ph = used && im.h > y0 ? (im.h - y0 + dy - 1) / dy : 0;
        im.pass_w[k] = pw && ph ? pw : 0;
        im.pass_h[k] = pw && ph ? ph : 0;
        im.pass_rb[k] = (uint32_t)(((uint64_t)im.pass_w[k] * im.bpp_bits + 7) / 8);
        im.pass_off[k] = raw;
        raw += (uint64_t)im.pass_h[k] * (1 + im.pass_rb[k]);
    }
    im.raw_bytes = raw;
    switch (im.ctype) {
    case 0: im.out_ch = im.has_trns ? 2 : 1; break;
    case 2: im.out_ch = im.has_trns ? 4 : 3; break;
    case 3: im.out_ch = im.has_trns ? 4 : 3; break;
    case 4: im.out_ch = 2; break;
    default: im.out_ch = 4; break;
    }
    im.out_depth = im.depth == 16 ? 16 : 8;
    im.hc = im.out_depth == 16 ? 3 : im.out_ch == 1 ? 1 : im.out_ch == 3 ? 3 : 4;
    im.hp_off = im.x16_off = im.nat_off = NONE;
    // the plausibility bound (before anything is allocated) and the size limit
    if (raw > INFLATE_RATIO * (uint64_t)p.idat_bytes) return RPH_ERR_UNSUPPORTED;
    if (raw > MAX_RAW_BYTES || (uint64_t)im.w * im.h > MAX_PIXELS) return RPH_ERR_UNSUPPORTED;
    return RPH_OK;
}

void gather(const uint8_t *d, const Parsed &p, uint8_t *dst)
{
    for (const auto &s : p.idat) {
        memcpy(dst, d + s.first, s.second);
        dst += s.second;
    }
}

bool unfilter_host(const Image &im, uint8_t *raw)
{
    for (int k = 0; k < 7; k++) {
        const uint32_t rb = im.pass_rb[k], u = im.unit;
        uint8_t *prev = nullptr;
        for (uint32_t y = 0; y < im.pass_h[k]; y++) {
            uint8_t *row = raw + im.pass_off[k] + (uint64_t)y * (1 + rb);
            const uint32_t f = row[0];
            if (f > 4) return false;
            uint8_t *r = row + 1, *q = prev ? prev + 1 : nullptr;
            for (uint32_t i = 0; i < rb; i++) {
                const uint8_t a = i >= u ? r[i - u] : 0, b = q ? q[i] : 0, c = (q && i >= u) ? q[i - u] : 0;
                r[i] = unfilter_byte(f, r[i], a, b, c);
            }
            prev = row;
        }
    }
    return true;
}

int decode_host(const uint8_t *data, size_t len, Parsed &p, std::vector<uint8_t> &native)
{
    int rc = parse(data, len, p);
    if (rc) return rc;
    const Image &im = p.im;
    std::vector<uint8_t> z(p.idat_bytes), raw(im.raw_bytes);
    gather(data, p, z.data());
    if (rphz::inflate_host(z.data(), z.size(), raw.data(), im.raw_bytes) != rphz::Z_OK) return RPH_ERR_INVALID_ARG;
    if (!unfilter_host(im, raw.data())) return RPH_ERR_INVALID_ARG;
    const size_t bps = im.out_depth / 8;
    native.assign((size_t)im.w * im.h * im.out_ch * bps, 0);
    for (uint32_t y = 0; y < im.h; y++)
        for (uint32_t x = 0; x < im.w; x++) {
            uint32_t v[4];
            pixel(im, raw.data(), p.palette, x, y, v);
            const size_t o = ((size_t)y * im.w + x) * im.out_ch;
            for (uint32_t c = 0; c < im.out_ch; c++) {
                if (bps == 1)
                    native[o + c] = (uint8_t)v[c];
                else {
                    const uint16_t s = (uint16_t)v[c];
                    memcpy(&native[(o + c) * 2], &s, 2);
                }
            }
        }
    return RPH_OK;
}

}  // namespace rphp
