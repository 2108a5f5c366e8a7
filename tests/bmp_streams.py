"""BMP files for the tests of the BMP path (include/rupphash.h, BMP section): a writer for every header size, depth, compression, mask set
and row order the section names, RLE8 / RLE4 streams built code by code, one damaged file per line of the damaged-file rule, and a numpy
statement of the native-pixel rule (rule_palette, rule_fields, rle_decode) that does not read the files it judges: every builder returns
the file together with the pixels the rule gives for what was put into it.

    python tests/bmp_streams.py DIR     dumps the valid, the Pillow and the damaged corpus as DIR/*.bmp (tools/fuzz_bmp_host.cpp)
"""
import functools
import io
import struct

import numpy as np

INVALID, UNSUPPORTED = -1, -5
BI_RGB, BI_RLE8, BI_RLE4, BI_BITFIELDS, BI_JPEG, BI_PNG, BI_ALPHABITFIELDS = 0, 1, 2, 3, 4, 5, 6

# mask sets: (bits, (R, G, B, A))
MASKS = {
    "565": (16, (0xF800, 0x07E0, 0x001F, 0)),
    "555": (16, (0x7C00, 0x03E0, 0x001F, 0)),
    "4444a": (16, (0x0F00, 0x00F0, 0x000F, 0xF000)),
    "8888a": (32, (0x00FF0000, 0x0000FF00, 0x000000FF, 0xFF000000)),
    "888x": (32, (0x00FF0000, 0x0000FF00, 0x000000FF, 0)),
    "rgba_order": (32, (0x000000FF, 0x0000FF00, 0x00FF0000, 0xFF000000)),
    "odd_10_3_10": (32, (0xFFC00000, 0x00001C00, 0x000003FF, 0)),       # 10-bit R and B keep their top 8, G has 3 bits
    "odd_3_10_2a": (32, (0x00000007, 0x00FFC000, 0x00000300, 0x70000000)),  # alpha of 3 bits
    "zero_green_16": (16, (0xF800, 0, 0x001F, 0)),
    "1_bit_channels_16": (16, (0x0004, 0x0002, 0x0001, 0x0008)),
}


# ---- the rule, in numpy ----

def rule_palette(idx, pal):
    """(h, w, 3): the palette's colour, black for an index past it (idx < 0: a pixel an RLE stream skipped, black too)"""
    pal = np.asarray(pal, np.uint8).reshape(-1, 3)
    idx = np.asarray(idx, np.int64)
    out = np.zeros(idx.shape + (3,), np.uint8)
    ok = (idx >= 0) & (idx < len(pal))
    out[ok] = pal[idx[ok]]
    return out


def field(mask):
    """(shift, len) of a contiguous mask; (0, 0) for a zero mask"""
    if not mask:
        return 0, 0
    shift = (mask & -mask).bit_length() - 1
    return shift, (mask >> shift).bit_length()


def rule_fields(v, masks):
    """v: (h, w) raw pixel values.  A channel of len bits (its top 8 when wider) scales by (s * 255 + max // 2) // max, max = 2^len - 1;
    a zero colour mask gives 0; Rgba8 when the alpha mask is non-zero, else Rgb8"""
    v = np.asarray(v, np.uint64)
    ch = 4 if masks[3] else 3
    out = np.zeros(v.shape + (ch,), np.uint8)
    for c in range(ch):
        shift, n = field(masks[c])
        if not n:
            continue
        s = (v >> np.uint64(shift)) & np.uint64((1 << n) - 1)
        if n > 8:
            s, n = s >> np.uint64(n - 8), 8
        mx = (1 << n) - 1
        out[..., c] = ((s * np.uint64(255) + np.uint64(mx // 2)) // np.uint64(mx)).astype(np.uint8)
    return out


def rle_decode(stream, w, h, four):
    """The RLE rule: (h, w) int array of palette indices, top-down, -1 where the stream sets nothing; None for a stream the rule refuses
    (a run or delta that leaves the bitmap, no end-of-bitmap)"""
    out = np.full((h, w), -1, np.int64)
    pos = x = y = 0
    n = len(stream)
    while True:
        if n - pos < 2:
            return None
        a, b = stream[pos], stream[pos + 1]
        pos += 2
        if a:
            if y >= h or x + a > w:
                return None
            for k in range(a):
                out[h - 1 - y, x + k] = ((b & 15) if k & 1 else (b >> 4)) if four else b
            x += a
        elif b == 0:
            x, y = 0, y + 1
            if y > h:
                return None
        elif b == 1:
            return out
        elif b == 2:
            if n - pos < 2:
                return None
            x, y = x + stream[pos], y + stream[pos + 1]
            pos += 2
            if x > w or y > h:
                return None
        else:
            nbytes = (b + 1) // 2 if four else b
            padded = (nbytes + 1) & ~1
            if n - pos < padded or y >= h or x + b > w:
                return None
            for k in range(b):
                byte = stream[pos + k // 2] if four else stream[pos + k]
                out[h - 1 - y, x + k] = ((byte & 15) if k & 1 else (byte >> 4)) if four else byte
            x += b
            pos += padded


# ---- the writer ----

def pack_rows(rows, top_down):
    """rows: list of bytes, top row first; padded to 4 bytes, bottom-up unless top_down"""
    rows = [r + b"\0" * (-len(r) % 4) for r in rows]
    return b"".join(rows if top_down else rows[::-1])


def index_rows(idx, bits):
    """(h, w) indices -> rows of packed bytes, most significant bits first"""
    idx = np.asarray(idx, np.uint8)
    h, w = idx.shape
    per = 8 // bits
    padded = np.zeros((h, (w + per - 1) // per * per), np.uint8)
    padded[:, :w] = idx
    acc = np.zeros((h, padded.shape[1] // per), np.uint8)
    for k in range(per):
        acc |= padded[:, k::per] << np.uint8(8 - bits * (k + 1))
    return [r.tobytes() for r in acc]


def value_rows(v, bits):
    v = np.asarray(v)
    return [r.astype("<u2" if bits == 16 else "<u4").tobytes() for r in v]


def bmp_file(hdr, w, h, bits, comp, array, palette=None, masks=None, clr_used=0, planes=1, off=None, gap=0, header_masks=None):
    """h: signed (negative: top-down).  palette: (n, 3) RGB.  masks: written behind a 40-byte header (as many as given) or inside a longer
    one.  off: the pixel-array offset to declare (default: where the array is put: behind headers, masks, palette and `gap` bytes)"""
    if hdr == 12:
        dib = struct.pack("<IHHHH", 12, w & 0xFFFF, h & 0xFFFF, planes, bits)
    else:
        dib = struct.pack("<IiiHHIIiiII", hdr, w, h, planes, bits, comp, 0, 2835, 2835, clr_used, 0)
        if hdr > 40:
            inside = list(header_masks if header_masks is not None else (masks or (0, 0, 0, 0)))[:(hdr - 40) // 4]
            dib += b"".join(struct.pack("<I", m) for m in inside)
            dib += b"\0" * (hdr - len(dib))
        elif masks:
            dib += b"".join(struct.pack("<I", m) for m in masks)
    pal = b""
    if palette is not None:
        for r, g, b in np.asarray(palette, np.uint8).reshape(-1, 3).tolist():
            pal += bytes([b, g, r]) if hdr == 12 else bytes([b, g, r, 0])
    body = dib + pal + b"\xAA" * gap
    real_off = 14 + len(body)
    head = b"BM" + struct.pack("<IHHI", real_off + len(array), 0, 0, real_off if off is None else off)
    return head + body + array


def colour_palette(n, seed=1):
    return np.random.default_rng(seed).integers(0, 256, (n, 3)).astype(np.uint8)


def rle_encode(idx, four, eol_last=True, literal_only=False, even_absolute=False):
    """rows bottom-up; runs of >= 2 equal pixels as encoded runs, other stretches of >= 3 as absolute runs (odd lengths among them, padded
    to 16 bits), shorter ones as encoded runs of 1; end-of-line behind every row (the last one: eol_last), end-of-bitmap.
    even_absolute: an odd stretch gives its last pixel to an encoded run of 1 (Pillow reads n // 2 bytes of an RLE4 absolute run of n
    pixels and so loses the last pixel of an odd one)"""
    idx = np.asarray(idx)
    h, w = idx.shape
    out = bytearray()

    def absolute(vals):
        while vals:
            part, vals = vals[:254 if even_absolute else 255], vals[254 if even_absolute else 255:]
            if even_absolute and len(part) > 3 and len(part) & 1:
                part, vals = part[:-1], part[-1:] + vals
            if len(part) < 4 if even_absolute else len(part) < 3:
                for v in part:
                    out.extend((1, (v << 4 | v) if four else v))
                continue
            out.extend((0, len(part)))
            if four:
                part = part + [0] * (len(part) & 1)
                data = bytes(part[k] << 4 | part[k + 1] for k in range(0, len(part), 2))
            else:
                data = bytes(part)
            out.extend(data + b"\0" * (len(data) & 1))

    for y in range(h - 1, -1, -1):
        row = idx[y].tolist()
        x, lit = 0, []
        while x < w:
            e = x
            while e < w and row[e] == row[x] and e - x < 255:
                e += 1
            if e - x >= 2 and not literal_only:
                absolute(lit)
                lit = []
                out.extend((e - x, (row[x] << 4 | row[x]) if four else row[x]))
            else:
                lit.extend(row[x:e])
            x = e
        absolute(lit)
        if y > 0 or eol_last:
            out.extend((0, 0))
    out.extend((0, 1))
    return bytes(out)


def rle_bmp(stream, w, h, four, pal, hdr=40, top_down=False, **kw):
    return bmp_file(hdr, w, -h if top_down else h, 4 if four else 8, BI_RLE4 if four else BI_RLE8, bytes(stream), palette=pal,
                    clr_used=0 if len(pal) == (16 if four else 256) else len(pal), **kw)


VARIANTS = ("pal1", "pal2", "pal4", "pal8", "rgb16", "bf565", "bf555", "bf4444a", "bf8888a", "bf888x", "bf_odd", "bf_odd_a", "rgb24", "rgb32", "rle8", "rle4")
ROW_ORDERS = (False, True)


def make(variant, w, h, top_down=False, seed=0, hdr=None, even_absolute=False):
    """(file, pixels by the rule) of one variant at one size; RLE files are bottom-up whatever top_down says"""
    rng = np.random.default_rng([seed, w, h, VARIANTS.index(variant)])
    hs = -h if top_down else h
    if variant.startswith("pal"):
        bits = int(variant[3:])
        pal = colour_palette(1 << bits, seed + bits)
        idx = rng.integers(0, 1 << bits, (h, w))
        return bmp_file(hdr or 40, w, hs, bits, BI_RGB, pack_rows(index_rows(idx, bits), top_down), palette=pal), rule_palette(idx, pal)
    if variant in ("rle8", "rle4"):
        four = variant == "rle4"
        pal = colour_palette(16 if four else 256, seed + 40)
        idx = rng.integers(0, len(pal), (h, w))
        flat = rng.integers(0, 3, (h, (w + 4) // 5)).repeat(5, axis=1)[:, :w] > 0  # stretches of equal pixels between the noise
        idx = np.where(flat, idx[:, :1], idx)
        return rle_bmp(rle_encode(idx, four, even_absolute=even_absolute), w, h, four, pal, hdr=hdr or 40), rule_palette(idx, pal)
    if variant == "rgb24":
        px = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        return bmp_file(hdr or 40, w, hs, 24, BI_RGB, pack_rows([r[:, ::-1].tobytes() for r in px], top_down)), px
    name = {"rgb16": "555", "rgb32": "888x", "bf565": "565", "bf555": "555", "bf4444a": "4444a", "bf8888a": "8888a", "bf888x": "888x",
            "bf_odd": "odd_10_3_10", "bf_odd_a": "odd_3_10_2a"}[variant]
    bits, masks = MASKS[name]
    v = rng.integers(0, 1 << bits, (h, w), dtype=np.uint64)  # (the bits no mask covers are set as well)
    array = pack_rows(value_rows(v, bits), top_down)
    if variant in ("rgb16", "rgb32"):
        return bmp_file(hdr or 40, w, hs, bits, BI_RGB, array), rule_fields(v, masks)
    hdr = hdr or (56 if masks[3] else 40)
    written = masks if hdr != 40 or masks[3] else masks[:3]
    comp = BI_ALPHABITFIELDS if hdr == 40 and masks[3] else BI_BITFIELDS
    return bmp_file(hdr, w, hs, bits, comp, array, masks=written), rule_fields(v, masks)


def _fields_file(name, hdr, comp, w=11, h=6, seed=3, top_down=False, n_masks=None):
    bits, masks = MASKS[name]
    v = np.random.default_rng(seed).integers(0, 1 << bits, (h, w), dtype=np.uint64)
    written = masks[:n_masks] if n_masks else masks
    seen = tuple(written) + (0,) * (4 - len(written))
    if hdr > 40:
        seen = tuple(seen[:(hdr - 40) // 4]) + (0,) * (4 - min(4, (hdr - 40) // 4))
    return bmp_file(hdr, w, -h if top_down else h, bits, comp, pack_rows(value_rows(v, bits), top_down), masks=written), rule_fields(v, seen)


@functools.lru_cache(maxsize=None)
def valid_files():
    """(name, file, pixels by the rule)"""
    out = []

    def add(name, pair):
        out.append((name, pair[0], pair[1]))

    for v in VARIANTS:
        for td in ROW_ORDERS:
            if td and v.startswith("rle"):
                continue
            add(f"{v}_13x7_{'top_down' if td else 'bottom_up'}", make(v, 13, 7, td, seed=1))
    # header sizes
    for hdr in (12, 40, 52, 56, 108, 124):
        add(f"rgb24_header_{hdr}", make("rgb24", 9, 5, seed=hdr, hdr=hdr))
        add(f"pal8_header_{hdr}", make("pal8", 10, 4, seed=hdr, hdr=hdr))
        add(f"pal4_header_{hdr}", make("pal4", 7, 3, top_down=hdr != 12, seed=hdr, hdr=hdr))
        if hdr != 12:
            add(f"rle8_header_{hdr}", make("rle8", 17, 5, seed=hdr, hdr=hdr))
            add(f"rgb32_header_{hdr}", make("rgb32", 6, 5, seed=hdr, hdr=hdr))
            add(f"bf565_header_{hdr}", _fields_file("565", hdr, BI_BITFIELDS, seed=hdr, n_masks=3 if hdr == 40 else None))
            add(f"bf8888a_header_{hdr}_compression_3", _fields_file("8888a", hdr, BI_BITFIELDS, seed=hdr, n_masks=3 if hdr == 40 else None))
            add(f"bf4444a_header_{hdr}_compression_6", _fields_file("4444a", hdr, BI_ALPHABITFIELDS, seed=hdr))
    # masks in a long header are not read under BI_RGB
    bits, masks = MASKS["555"]
    v = np.random.default_rng(8).integers(0, 1 << 16, (4, 9), dtype=np.uint64)
    add("rgb16_ignores_header_masks", (bmp_file(108, 9, 4, 16, BI_RGB, pack_rows(value_rows(v, 16), False), header_masks=MASKS["4444a"][1]), rule_fields(v, masks)))
    for name in ("rgba_order", "zero_green_16", "1_bit_channels_16", "odd_10_3_10", "odd_3_10_2a"):
        add(f"masks_{name}", _fields_file(name, 124, BI_BITFIELDS, w=19, h=5, seed=11))
    # widths around the row padding
    for w in range(1, 10):
        add(f"rgb24_width_{w}", make("rgb24", w, 3, seed=w))
        add(f"pal1_width_{w}", make("pal1", w, 2, top_down=bool(w & 1), seed=w))
        add(f"pal4_width_{w}", make("pal4", w, 2, seed=w))
        add(f"bf565_width_{w}", make("bf565", w, 2, seed=w))
    add("pal1_33x3", make("pal1", 33, 3, seed=2))
    add("pal2_17x3", make("pal2", 17, 3, seed=2))
    # short palettes: indices past the palette are black
    for bits, n in ((8, 17), (4, 5), (2, 3), (1, 1)):
        pal = colour_palette(n, 50 + bits)
        idx = np.random.default_rng(bits).integers(0, 1 << bits, (5, 12))
        add(f"pal{bits}_short_palette_{n}", (bmp_file(40, 12, 5, bits, BI_RGB, pack_rows(index_rows(idx, bits), False), palette=pal, clr_used=n), rule_palette(idx, pal)))
    # a gap between the headers and the array; bytes behind the array
    f, px = make("rgb24", 5, 4, seed=77)
    array = f[54:]
    add("gap_before_the_array", (bmp_file(40, 5, 4, 24, BI_RGB, array, gap=10), px))
    add("bytes_behind_the_array", (f + b"trailing", px))
    # RLE
    pal256, pal16, pal9 = colour_palette(256, 60), colour_palette(16, 61), colour_palette(9, 62)
    rng = np.random.default_rng(9)
    for four, pal in ((False, pal256), (True, pal16)):
        t = "rle4" if four else "rle8"
        noise = rng.integers(0, len(pal), (6, 7))
        add(f"{t}_absolute_runs_of_7", (rle_bmp(rle_encode(noise, four, literal_only=True), 7, 6, four, pal), rule_palette(noise, pal)))
        for wd in (3, 4, 5, 6):  # absolute runs of odd and even lengths: 16-bit padding
            n2 = rng.integers(0, len(pal), (2, wd))
            add(f"{t}_absolute_runs_of_{wd}", (rle_bmp(rle_encode(n2, four, literal_only=True), wd, 2, four, pal), rule_palette(n2, pal)))
        flat = np.full((3, 300), 5)
        add(f"{t}_runs_longer_than_255", (rle_bmp(rle_encode(flat, four), 300, 3, four, pal), rule_palette(flat, pal)))
        wide = rng.integers(0, len(pal), (2, 300))
        add(f"{t}_absolute_longer_than_255", (rle_bmp(rle_encode(wide, four, literal_only=True), 300, 2, four, pal), rule_palette(wide, pal)))
        mixed = rng.integers(0, len(pal), (5, 21))
        mixed[:, 4:13] = mixed[:, 4:5]
        add(f"{t}_no_eol_behind_the_last_row", (rle_bmp(rle_encode(mixed, four, eol_last=False), 21, 5, four, pal), rule_palette(mixed, pal)))
        add(f"{t}_bytes_behind_end_of_bitmap", (rle_bmp(rle_encode(mixed, four) + b"\x05\x05junk", 21, 5, four, pal), rule_palette(mixed, pal)))
        # by hand: run, delta, absolute, end-of-line in the middle of a row, early end-of-bitmap: skipped pixels are black
        if four:  # 1 2 1 | delta (2, 1) | absolute 3 4 5 | end-of-line | 7 7 | delta (0, 2) | 2 1 2 1 | end-of-bitmap
            s = bytes([3, 0x12, 0, 2, 2, 1, 0, 3, 0x34, 0x50, 0, 0, 2, 0x77, 0, 2, 0, 2, 4, 0x21, 0, 1])
        else:  # 2 2 2 | delta (2, 1) | absolute 4 5 7 + padding | end-of-line | 8 8 | delta (0, 2) | 200 x 4 | end-of-bitmap
            s = bytes([3, 2, 0, 2, 2, 1, 0, 3, 4, 5, 7, 0, 0, 0, 2, 8, 0, 2, 0, 2, 4, 200, 0, 1])
        for p, pn in ((pal, "full_palette"), (pal9, "palette_of_9")):
            idx = rle_decode(s, 10, 6, four)
            assert idx is not None and (idx < 0).any() and (idx >= 0).any()
            add(f"{t}_delta_and_skipped_pixels_{pn}", (rle_bmp(s, 10, 6, four, p), rule_palette(idx, p)))
        add(f"{t}_only_end_of_bitmap", (rle_bmp(b"\0\1", 6, 6, four, pal), np.zeros((6, 6, 3), np.uint8)))
        add(f"{t}_delta_to_the_corner", (rle_bmp(bytes([0, 2, 6, 6, 0, 1]), 6, 6, four, pal), np.zeros((6, 6, 3), np.uint8)))
    # the skipped pixels of a file whose whole palette is white stay black
    white = np.full((256, 3), 255, np.uint8)
    s = bytes([2, 9, 0, 2, 3, 0, 2, 9, 0, 1])
    add("rle8_skipped_pixels_are_not_entry_0", (rle_bmp(s, 8, 2, False, white), rule_palette(rle_decode(s, 8, 2, False), white)))
    return out


@functools.lru_cache(maxsize=None)
def pillow_written():
    """(name, file) written by Pillow: 1-, 8-, 24- and 32-bit"""
    from PIL import Image

    rng = np.random.default_rng(21)
    out = []
    for name, im in (("pillow_1", Image.fromarray(rng.integers(0, 2, (9, 21)).astype(bool))),
                     ("pillow_L", Image.fromarray(rng.integers(0, 256, (9, 21)).astype(np.uint8), "L")),
                     ("pillow_P", Image.fromarray(rng.integers(0, 256, (7, 13, 3)).astype(np.uint8), "RGB").quantize(37)),
                     ("pillow_RGB", Image.fromarray(rng.integers(0, 256, (7, 13, 3)).astype(np.uint8), "RGB")),
                     ("pillow_RGBA", Image.fromarray(rng.integers(0, 256, (7, 13, 4)).astype(np.uint8), "RGBA"))):
        b = io.BytesIO()
        im.save(b, "BMP")
        out.append((name, b.getvalue()))
    return out


def pillow_exact_files():
    """(name, file) that Pillow and the rule must decode alike, byte for byte: the list is fixed here"""
    out = list(pillow_written())
    for v in ("pal1", "pal4", "pal8", "rgb24", "rgb32", "bf888x"):
        for td in ROW_ORDERS:
            out.append((f"{v}_{'top_down' if td else 'bottom_up'}", make(v, 23, 9, td, seed=5)[0]))
    for v in ("rle8", "rle4"):
        # (RLE4: absolute runs of even lengths only, the ones Pillow reads whole; odd ones are held to the rule in valid_files)
        out.append((f"{v}_covers_every_pixel", make(v, 37, 9, seed=5, even_absolute=v == "rle4")[0]))
        out.append((f"{v}_wide", make(v, 300, 4, seed=6, even_absolute=v == "rle4")[0]))
    return out


def pillow_16_bit_files():
    """(name, file): Pillow floors where the rule rounds to nearest: within 1 per sample"""
    return [(v, make(v, 64, 33, td, seed=5)[0]) for v in ("rgb16", "bf565", "bf555") for td in ROW_ORDERS]


@functools.lru_cache(maxsize=None)
def damaged_files():
    """(name, file, status): one file per line of the damaged-file rule, and pairs that show the order of the checks"""
    out = []

    def add(name, data, status):
        out.append((name, bytes(data), status))

    good, _ = make("rgb24", 6, 4, seed=1)  # 40-byte header, array at 54, rows of 20 bytes

    def patch(at, fmt, *vals, base=good):
        b = bytearray(base)
        b[at:at + struct.calcsize(fmt)] = struct.pack(fmt, *vals)
        return b

    add("empty_but_for_the_signature", b"BM", INVALID)
    add("seventeen_bytes", good[:17], INVALID)
    add("not_bm", b"MB" + good[2:], INVALID)
    add("header_cut", good[:40], INVALID)
    for size in (16, 64, 0, 41):
        add(f"header_size_{size}", patch(14, "<I", size), UNSUPPORTED)
    add("planes_0", patch(26, "<H", 0), INVALID)
    add("planes_2", patch(26, "<H", 2), INVALID)
    add("width_0", patch(18, "<i", 0), INVALID)
    add("width_negative", patch(18, "<i", -6), INVALID)
    add("height_0", patch(22, "<i", 0), INVALID)
    add("width_65536", patch(18, "<i", 65536), UNSUPPORTED)
    add("height_minus_65536", patch(22, "<i", -65536), UNSUPPORTED)
    add("more_than_2_28_pixels", patch(18, "<ii", 20000, 20000), UNSUPPORTED)
    add("compression_jpeg", patch(30, "<I", BI_JPEG), UNSUPPORTED)
    add("compression_png", patch(30, "<I", BI_PNG), UNSUPPORTED)
    add("compression_7", patch(30, "<I", 7), UNSUPPORTED)
    add("depth_3", patch(28, "<H", 3), UNSUPPORTED)
    add("depth_0", patch(28, "<H", 0), UNSUPPORTED)
    add("depth_64", patch(28, "<H", 64), UNSUPPORTED)
    add("bitfields_at_24_bits", patch(30, "<I", BI_BITFIELDS), UNSUPPORTED)
    add("rle8_at_4_bits", patch(30, "<I", BI_RLE8, base=make("pal4", 6, 4)[0]), UNSUPPORTED)
    add("rle4_at_8_bits", patch(30, "<I", BI_RLE4, base=make("pal8", 6, 4)[0]), UNSUPPORTED)
    add("array_one_byte_short", good[:-1], INVALID)
    add("array_one_row_short", good[:-20], INVALID)
    add("offset_into_the_header", patch(10, "<I", 20), INVALID)
    add("offset_zero", patch(10, "<I", 0), INVALID)
    add("offset_at_the_end_of_the_file", patch(10, "<I", len(good)), INVALID)
    add("offset_past_the_file", patch(10, "<I", len(good) + 100), INVALID)
    add("offset_leaves_too_little", patch(10, "<I", 55), INVALID)
    pal8, _ = make("pal8", 6, 4, seed=2)
    add("offset_into_the_palette", patch(10, "<I", 54 + 100, base=pal8), INVALID)
    add("palette_of_300_at_8_bits", patch(46, "<I", 300, base=pal8), INVALID)
    add("palette_of_3_at_1_bit", patch(46, "<I", 3, base=make("pal1", 6, 4)[0]), INVALID)
    add("palette_cut_by_the_end", pal8[:54 + 500], INVALID)
    bf, _ = make("bf565", 6, 4, seed=2)  # 40-byte header, three masks behind it
    add("masks_cut_by_the_end", bf[:60], INVALID)
    add("mask_not_contiguous", patch(54, "<I", 0xA800, base=bf), INVALID)
    add("mask_with_a_hole", patch(58, "<I", 0x07A0, base=bf), INVALID)
    add("mask_above_bit_15_at_16_bits", patch(54, "<I", 0x1F0000, base=bf), INVALID)
    add("alpha_mask_not_contiguous", patch(66, "<I", 0xA0000000, base=make("bf8888a", 6, 4)[0]), INVALID)
    add("offset_into_the_masks", patch(10, "<I", 58, base=bf), INVALID)
    # RLE streams
    pal256, pal16 = colour_palette(256, 60), colour_palette(16, 61)
    for four, pal in ((False, pal256), (True, pal16)):
        t = "rle4" if four else "rle8"
        row = bytes([6, 0x11, 0, 0])
        ok = row * 4 + b"\0\1"
        assert rle_decode(ok, 6, 4, four) is not None
        cases = {
            "run_past_the_row": bytes([7, 0x11, 0, 0]) + row * 3 + b"\0\1",
            "run_past_the_row_in_two": bytes([4, 0x11, 3, 0x22, 0, 0]) + b"\0\1",
            "absolute_past_the_row": bytes([4, 0x11, 0, 3, 1, 2, 3, 0, 0, 0, 0, 1]),
            "run_above_the_top_row": row * 4 + bytes([1, 0x11, 0, 1]),
            "absolute_above_the_top_row": row * 4 + bytes([0, 3, 1, 2, 3, 0, 0, 1]),
            "end_of_line_above_the_top_row": row * 4 + b"\0\0\0\1",
            "delta_past_the_width": bytes([0, 2, 7, 0, 0, 1]),
            "delta_past_the_height": bytes([0, 2, 0, 5, 0, 1]),
            "delta_cut_by_the_end": bytes([0, 2, 1]),
            "no_end_of_bitmap": row * 4,
            "no_end_of_bitmap_half_way": row * 2,
            "empty_stream": b"\0",
            "absolute_cut_by_the_end": bytes([0, 5, 1, 2]),
            "absolute_without_its_padding": bytes([0, 3, 1, 2, 3]) if not four else bytes([0, 5, 0x12, 0x34, 0x50]),
        }
        for name, s in cases.items():
            assert rle_decode(s, 6, 4, four) is None, name
            add(f"{t}_{name}", rle_bmp(s, 6, 4, four, pal), INVALID)
        add(f"{t}_top_down", rle_bmp(ok, 6, 4, four, pal, top_down=True), INVALID)
    # where two apply, the first in the stated order decides
    add("order_header_size_before_planes", patch(14, "<I", 64, base=patch(26, "<H", 0)), UNSUPPORTED)
    add("order_planes_before_the_side_limit", patch(26, "<H", 0, base=patch(18, "<i", 70000)), INVALID)
    add("order_zero_height_before_the_side_limit", patch(22, "<i", 0, base=patch(18, "<i", 70000)), INVALID)
    add("order_side_limit_before_compression", patch(30, "<I", BI_JPEG, base=patch(18, "<i", 70000)), UNSUPPORTED)
    add("order_compression_before_the_array", patch(30, "<I", BI_PNG)[:-30], UNSUPPORTED)
    add("order_pixel_limit_before_the_array", patch(18, "<ii", 30000, 30000), UNSUPPORTED)
    add("order_palette_count_before_the_offset", patch(10, "<I", 3, base=patch(46, "<I", 300, base=pal8)), INVALID)
    return out


def dump(directory):
    import os

    os.makedirs(directory, exist_ok=True)
    files = [(n, d) for n, d, _ in valid_files()] + [(n, d) for n, d, _ in damaged_files()] + pillow_exact_files() + pillow_16_bit_files()
    for name, data in files:
        with open(os.path.join(directory, name + ".bmp"), "wb") as f:
            f.write(data)
    return len(files)


if __name__ == "__main__":
    import sys

    print(dump(sys.argv[1]), "files")
