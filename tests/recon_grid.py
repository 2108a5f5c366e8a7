"""Grids of files for the stages behind the entropy decoders: the PNG unfilter kernel, the TIFF expand kernel and the WebP inverse
transforms and table slots.  Every grid puts the sizes where wave-shaped code goes wrong (rows and pixels 63 / 64 / 65 and 127 / 128 /
129, units of 1 to 8 bytes, every sample layout, every filter or predictor mode) under noise, so that running sums wrap, Paeth takes
all three branches, the clamping modes saturate at both ends and select meets ties (a share of every image holds only 0 and the
maximum).  Seeded, built once per process, (name, bytes) lists per group; references() decodes each file once with the plain Python
decoders and hashes what the pixel hash hashes.

GIF and BMP have no stage behind an entropy decoder; their grids put the device kernels they do have on their seams: the GIF expand
kernel's row loop past one trip of its grid and its frame edges on the 64-pixel steps, the GIF LZW kernel's switch between LDS and
global memory and its 64-byte copies under noise, the BMP expand kernel's walk through a band of rows.  Their references are the
pixels gif_streams and bmp_streams state for what they write."""
import os
import re

import numpy as np

import blake3_util as b3
import bmp_streams as bs
import gif_streams as gs
import png_util as pu
import tiff_util as tu
import webp_util as wu

_CACHE = {}
_REFS = {}


def _noise(rng, shape, top):
    """uniform noise in 0 .. top; rows 5-7 of every 8 hold 0 and top only (ties, saturation)"""
    v = rng.integers(0, top + 1, shape).astype(np.int64)
    two = rng.integers(0, 2, shape) * top
    band = (np.arange(shape[0]) % 8 >= 5).reshape((-1,) + (1,) * (len(shape) - 1))
    return np.where(band, two, v)


# ------------------------------------------------------------------ PNG
# (layout, colour type, depth): filter units of 1, 1, 1, 1, 1, 2, 2, 3, 4, 4, 6 and 8 bytes
PNG_LAYOUTS = [("gray8", 0, 8), ("gray1", 0, 1), ("gray2", 0, 2), ("gray4", 0, 4), ("palette8", 3, 8), ("graya8", 4, 8), ("gray16", 0, 16), ("rgb8", 2, 8),
               ("rgba8", 6, 8), ("graya16", 4, 16), ("rgb16", 2, 16), ("rgba16", 6, 16)]
PNG_ROWS, PNG_WIDTHS = (1, 63, 64, 65, 129), (1, 3, 65)
FILTER_CYCLE = [0, 1, 2, 3, 4, 4, 3]


def _png(rng, layout, w, h, content="noise", **kw):
    _, ct, d = next(l for l in PNG_LAYOUTS if l[0] == layout)
    top = (1 << d) - 1
    shape = (h, w, pu.CHANNELS[ct])
    s = _noise(rng, shape, top) if content == "noise" else np.full(shape, top if content == "ones" else 0, np.int64)
    palette = rng.integers(0, 256, (256, 3)) if ct == 3 else None
    return pu.encode(s, ct, d, palette=palette, level=1, **kw)


def png_grid():
    """{'filters': one filter type on every row; 'pairs': every ordered pair of filter types across rows 63 | 64 and 127 | 128 at units
    of 3 and 8 bytes; 'adam7': interlaced files whose passes have 65, 33, 17 ... rows, some of them empty}"""
    if "png" not in _CACHE:
        rng = np.random.default_rng(2101)
        filters, pairs, adam7 = [], [], []
        for layout, _, _ in PNG_LAYOUTS:
            for f in range(5):
                for h in PNG_ROWS:
                    for w in PNG_WIDTHS:
                        filters.append((f"{layout}-f{f}-{w}x{h}", _png(rng, layout, w, h, filters=f)))
        for content in ("ones", "zeros"):
            for layout in ("gray1", "rgb8", "rgba16"):
                filters.append((f"{layout}-cycle-{content}-65x65", _png(rng, layout, 65, 65, content, filters=FILTER_CYCLE)))
        for layout in ("rgb8", "rgba16"):
            for edge, h in ((64, 66), (128, 130)):
                for fa in range(5):
                    for fb in range(5):
                        rows = [FILTER_CYCLE[(y + fa) % 7] for y in range(h)]
                        rows[edge - 1], rows[edge] = fa, fb
                        pairs.append((f"{layout}-row{edge - 1}f{fa}-row{edge}f{fb}", _png(rng, layout, 5, h, filters=rows)))
        for layout in ("gray2", "rgb8", "rgba16"):
            for h in (129, 130, 257):
                for w in range(1, 9):
                    adam7.append((f"{layout}-adam7-{w}x{h}", _png(rng, layout, w, h, interlace=True, filters=FILTER_CYCLE)))
        adam7.append(("rgba16-adam7-ones-8x257", _png(rng, "rgba16", 8, 257, "ones", interlace=True, filters=FILTER_CYCLE)))
        adam7.append(("rgb8-adam7-zeros-8x257", _png(rng, "rgb8", 8, 257, "zeros", interlace=True, filters=FILTER_CYCLE)))
        _CACHE["png"] = dict(filters=filters, pairs=pairs, adam7=adam7)
    return _CACHE["png"]


# ------------------------------------------------------------------ TIFF
TIFF_WIDTHS = (1, 2, 63, 64, 65, 127, 128, 129, 193)
TIFF_NAMES = {1: "gray", 2: "graya", 3: "rgb", 4: "rgba"}


def tiff_layout(name):
    """the sample layout and byte order a grid file's name begins with, e.g. 'rgba16-MM'"""
    return "-".join(name.split("-")[:2])


def _tiff(rng, w, h, spp, bps, bo, content="noise", photometric=None, compression=8, **kw):
    top = (1 << bps) - 1
    s = _noise(rng, (h, w, spp), top) if content == "noise" else np.full((h, w, spp), top if content == "ones" else 0, np.int64)
    return tu.encode(s, photometric, bps, bo="<" if bo == "II" else ">", compression=compression, level=1, **kw)


def tiff_grid():
    """{'pred2_strips', 'pred2_tiles': predictor 2 for every sample count, depth and byte order at the widths around one, two and three
    steps of 64 pixels, in strips and in tiles narrower than, equal to and wider than a step with a cropped edge tile; 'pred1': packed
    gray of 1, 2 and 4 bits in both photometrics, and 16-bit gray and RGB in both byte orders}.  Deflate level 1 carries them; a few
    LZW files ride along."""
    if "tiff" not in _CACHE:
        rng = np.random.default_rng(2102)
        strips, tiles, pred1 = [], [], []
        for spp in (1, 2, 3, 4):
            for bps in (8, 16):
                for bo in ("II", "MM"):
                    lay = f"{TIFF_NAMES[spp]}{bps}-{bo}"
                    for w in TIFF_WIDTHS:
                        for rps in (1, 2):
                            strips.append((f"{lay}-pred2-rps{rps}-{w}x3", _tiff(rng, w, 3, spp, bps, bo, predictor=2, rows_per_strip=rps)))
                    if spp in (1, 4):
                        for tw in (16, 64, 80, 128, 144):
                            for w in (tw - 1, tw + 1, 2 * tw + 1):
                                tiles.append((f"{lay}-pred2-tile{tw}-{w}x17", _tiff(rng, w, 17, spp, bps, bo, predictor=2, tile=(tw, 16))))
        for content in ("ones", "zeros"):
            strips.append((f"rgba16-MM-pred2-{content}-129x3", _tiff(rng, 129, 3, 4, 16, "MM", content, predictor=2, rows_per_strip=2)))
            tiles.append((f"rgba8-II-pred2-{content}-tile80-161x17", _tiff(rng, 161, 17, 4, 8, "II", content, predictor=2, tile=(80, 16))))
        for spp, bps, bo, w in ((4, 16, "MM", 129), (1, 8, "II", 193), (2, 16, "II", 65)):
            strips.append((f"{TIFF_NAMES[spp]}{bps}-{bo}-pred2-lzw-{w}x3", _tiff(rng, w, 3, spp, bps, bo, compression=5, predictor=2, rows_per_strip=2)))
        tiles.append(("rgba16-II-pred2-lzw-tile80-161x17", _tiff(rng, 161, 17, 4, 16, "II", compression=5, predictor=2, tile=(80, 16))))
        for w in (1, 7, 8, 9, 63, 64, 65, 127, 129):
            for bps in (1, 2, 4):
                for photo, pname in ((0, "wiz"), (1, "biz")):
                    pred1.append((f"gray{bps}{pname}-II-{w}x3", _tiff(rng, w, 3, 1, bps, "II", photometric=photo, rows_per_strip=2)))
            for spp in (1, 3):
                for bo in ("II", "MM"):
                    pred1.append((f"{TIFF_NAMES[spp]}16-{bo}-pred1-{w}x3", _tiff(rng, w, 3, spp, 16, bo, rows_per_strip=2)))
        for content in ("ones", "zeros"):
            pred1.append((f"gray1wiz-II-{content}-65x3", _tiff(rng, 65, 3, 1, 1, "II", content, photometric=0)))
        _CACHE["tiff"] = dict(pred2_strips=strips, pred2_tiles=tiles, pred1=pred1)
    return _CACHE["tiff"]


# ------------------------------------------------------------------ WebP
WEBP_KEPT = ((2, 66), (64, 66), (65, 66), (129, 66), (65, 65), (65, 129))  # every mode (65 x 65: a second group of one row)
WEBP_THINNED = ((1, 66), (3, 66), (63, 66), (127, 66), (128, 66), (65, 1), (65, 2), (65, 64))  # size k: the modes with (k + mode) % 4 == 0
CROSS_VALUES = (-128, -1, 0, 1, 127)


def webp_slot_counts():
    """cache bits -> table slots of the entropy kernel: LDS_TABLE_U16 / group_stride(), at most MAX_SLOTS, read from the kernel's source"""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rupphash_amd", "csrc")
    kernels, vp8l = open(os.path.join(csrc, "webp_kernels.hip")).read(), open(os.path.join(csrc, "vp8l.h")).read()

    def find(text, pattern, what):
        m = re.search(pattern, text)
        assert m, f"{what}: the line this reads has changed, restate its pattern here"
        return m.group(1)

    arith = lambda expr, names: int(eval(expr, {"__builtins__": {}}, names))  # (sums and products of integers and earlier constants)
    names = {}
    names["T_COUNT"] = arith(find(vp8l, r"T_COUNT = ([\w +*]+),", "T_COUNT in vp8l.h"), names)
    names["T_SYM"] = arith(find(vp8l, r"T_SYM = ([\w +*]+);", "T_SYM in vp8l.h"), names)
    green = int(find(vp8l, r"green_symbols\(uint32_t cache_bits\) \{ return (\d+) \+ \(cache_bits \? 1u << cache_bits : 0\); \}", "green_symbols() in vp8l.h"))
    stride = find(vp8l, r"group_stride\(uint32_t cache_bits\) \{ return ([\w +*()]+); \}", "group_stride() in vp8l.h")
    assert "green_symbols(cache_bits)" in stride, stride
    lds = int(find(kernels, r"LDS_TABLE_U16 = (\d+);", "LDS_TABLE_U16 in webp_kernels.hip"))
    most = int(find(kernels, r"MAX_SLOTS = (\d+);", "MAX_SLOTS in webp_kernels.hip"))
    out = {}
    for cb in (0, 9, 10, 11):
        names["GREEN"] = green + ((1 << cb) if cb else 0)
        out[cb] = min(most, lds // arith(stride.replace("green_symbols(cache_bits)", "GREEN"), names))
    return out


def slot_map(n_groups, n_slots, blocks):
    """group of every block: the groups of one slot (equal modulo n_slots) take turns twice over, slot after slot"""
    seq = []
    for r in range(min(n_slots, n_groups)):
        seq += list(range(r, n_groups, n_slots)) * 2
    return [seq[k % len(seq)] for k in range(blocks)]


def _webp_noise(rng, w, h, alpha):
    return _noise(rng, (h, w, 4 if alpha else 3), 255).astype(np.uint8)


def webp_grid():
    """{'predictor_single': one mode 0 .. 15 per file (alpha on the odd ones) at the widths and heights around the 64-pixel window and
    the 64-row groups; 'predictor_mixed': modes 0 .. 15 per block at block bits 2, 5, 6, 7 and 9; 'cross': cross-colour coefficients
    -128, -1, 0, 1, 127 on green and red of 0x00, 0x7f, 0x80, 0xff; 'palette': 2, 4 and 16 colours at packed widths from 1 up, with and
    without a predictor behind the palette; 'slots': more groups than table slots, taking turns in each slot, with every cache size
    that changes the slot count}"""
    if "webp" not in _CACHE:
        rng = np.random.default_rng(2103)
        single, mixed, cross, palette, slots = [], [], [], [], []
        for m in range(16):
            sizes = list(WEBP_KEPT) + [s for k, s in enumerate(WEBP_THINNED) if (k + m) % 4 == 0]
            for w, h in sizes:
                single.append((f"mode{m}-{w}x{h}", wu.encode(_webp_noise(rng, w, h, m % 2 == 1), [("predictor", 2, m)])))
        for bits in (2, 5, 6, 7, 9):
            for w, h in ((130, 131), (65, 200)):
                mixed.append((f"mixed-bits{bits}-{w}x{h}", wu.encode(_webp_noise(rng, w, h, bits % 2 == 1), [("predictor", bits, "mixed16")], seed=bits)))
        for k, v in enumerate((255, 0)):
            mixed.append((f"mixed-bits2-all{v}-65x66", wu.encode(np.full((66, 65, 4), v, np.uint8), [("predictor", 2, "mixed16")], seed=20 + k)))
        for bits in (2, 5):
            bh, bw = wu.sub(21, bits), wu.sub(33, bits)
            for shift in range(5):
                img = _webp_noise(rng, 33, 21, shift % 2 == 1)
                img[:, :, :2] = np.array([0x00, 0x7f, 0x80, 0xff], np.uint8)[rng.integers(0, 4, (21, 33, 2))]
                b = np.arange(bh * bw).reshape(bh, bw, 1) + shift
                coeffs = np.array(CROSS_VALUES)[(b * np.array([1, 2, 3]) + np.array([0, 1, 2])) % 5]
                cross.append((f"cross-bits{bits}-{shift}", wu.encode(img, [("cross", bits, coeffs)])))
        for v in (255, 0):
            cross.append((f"cross-bits2-all{v}", wu.encode(np.full((21, 33, 3), v, np.uint8), [("cross", 2, np.full((6, 9, 3), -128))])))
        for colours, bits in ((2, 3), (4, 2), (16, 1)):
            pal = np.unique(wu.to_argb(rng.integers(0, 256, (1, 64, 4)).astype(np.uint8)).ravel())[:colours]
            pal[0], pal[-1] = 0, 0xffffffff
            for w in list(range(1, 10)) + [15, 16, 17, 63, 64, 65]:
                a = pal[rng.integers(0, colours, (3, w))]
                img = np.stack([(a >> 16) & 255, (a >> 8) & 255, a & 255, a >> 24], axis=-1).astype(np.uint8)
                palette.append((f"palette{colours}-{w}x3", wu.encode(img, [("palette", colours, pal)])))
                if wu.sub(w, bits) <= 2:
                    palette.append((f"palette{colours}-predictor-{w}x3", wu.encode(img, [("palette", colours, pal), ("predictor", 2, "mixed16")], seed=w)))
        counts = webp_slot_counts()
        for n_groups in (4, 7, 9):
            for cb, n_slots in counts.items():
                img = wu.flat(rng, 40, 36, 30)
                tokens = wu.tokenize([int(v) for v in wu.to_argb(img).ravel()], 40, cb, "lz")
                pos, crossing = 0, 0
                for t in tokens:
                    crossing += t[0] == "ref" and (pos % 40) // 4 != ((pos % 40) + t[1] - 1) // 4
                    pos += wu.token_pixels(t)
                assert crossing > 10  # copies that cross block edges
                ent = slot_map(n_groups, n_slots, 10 * 9)
                slots.append((f"slots-groups{n_groups}-cache{cb}", wu.encode(img, cache_bits=cb, meta_bits=2, n_groups=n_groups, tokens=tokens, ent_map=ent)))
        _CACHE["webp"] = dict(predictor_single=single, predictor_mixed=mixed, cross=cross, palette=palette, slots=slots)
    return _CACHE["webp"]


# ------------------------------------------------------------------ GIF
# The expand kernel gives one wave a screen row and a block four of them; the launch has at most 256 blocks, so one trip of a wave's row
# loop covers 1024 rows.  The LZW kernel builds a frame of at most 16 384 indices in LDS and a longer one in global memory.
GIF_ROWS_PER_TRIP, GIF_LDS_FRAME = 1024, 16384
GIF_TALL = (1023, 1024, 1025, 1028, 2047, 2049)
GIF_COPY_LENGTHS = (63, 64, 65, 127, 128, 129)
GIF_OVERRUNS = (1, 63, 64, 65)
GIF_SMALL = "small-5x5"  # the file the tall screens are mixed with (test_recon_grid_gpu.py)


class _Built:
    """a format whose builders (gif_streams, bmp_streams) hand out the pixels the rule gives together with the file: references() takes
    them from _PIXELS and decodes nothing"""
    to_rgba16 = staticmethod(b3.rgba16_bytes)


_PIXELS = {}


def _gif_content(rng, shape, colours, opaque):
    """noise over `colours` indices and what it is shown with: (indices, m, palette, transparent index).  Not opaque: a palette half as
    long as the index range (indices past the palette) and a transparent index in the palette's middle, so that noise falls on both
    sides of it; opaque: the whole palette and no transparency, what Pillow decodes by the same rule."""
    m = max(2, (colours - 1).bit_length())
    idx = rng.integers(0, colours, shape).astype(np.uint8)
    if opaque:
        return idx, m, gs.colour_palette(1 << m, colours + 1), None
    n = max(2, (1 << m) // 2)
    return idx, m, gs.colour_palette(n, colours), n // 2


def _gif_image(rng, fw, fh, colours=32, opaque=False, **kw):
    idx, m, pal, trans = _gif_content(rng, (fh, fw), colours, opaque)
    return gs.image_gif(idx, pal, m=m, trans=trans, **kw)


class _Codes:
    """a raw code list that keeps count of what the decoder's table will hold: emit() returns the entry the code adds (the string
    before it and its first byte), or None"""

    def __init__(self, m):
        self.m, self.codes, self.out = m, [], 0
        self.clear()

    def clear(self):
        self.codes.append(1 << self.m)
        self.next, self.prev = (1 << self.m) + 2, False

    def emit(self, code, length):
        added = None
        if self.prev and self.next < gs.ENTRIES:
            added, self.next = self.next, self.next + 1
        self.prev = True
        self.codes.append(code)
        self.out += length
        return added


def _staircase(c, s, kwkwk=(), last=None):
    """After S[0], S[1] the pair (code of S[:j], literal S[j]) adds the entry S[:j + 1]: every pair begins with a plain copy of j bytes of
    noise.  Before the pair of j = L - 1 for L in kwkwk: (code of S[:L - 1], the next free entry), the copy of L bytes that overlaps its
    own output by one byte.  last = ("copy", L) or ("kwkwk", L): stop with that code (the caller clips it)."""
    c.emit(int(s[0]), 1)
    code = None
    for j in range(1, len(s)):
        if code is not None:
            if j + 1 in kwkwk or last == ("kwkwk", j + 1):
                c.emit(code, j)
                c.emit(c.next, j + 1)
                if last == ("kwkwk", j + 1):
                    return
            c.emit(code, j)
            if last == ("copy", j):
                return
        code = c.emit(int(s[j]), 1)
    assert last is None


def _gif_raw(name, c, m, w, h, pal, trans):
    stream = gs.pack_codes(c.codes, m)
    idx = gs.lzw_decode(stream, m, w * h)
    assert idx is not None, name
    return name, gs.write_gif((w, h), (0, 0), (w, h), m, stream, gct=pal, trans=trans), gs.render((w, h), (0, 0), idx.reshape(h, w), pal, trans)


def _gif_copies(rng):
    """raw code streams whose copies carry noise, each in a frame built in LDS (one staircase) and in one built in global memory (two,
    a Clear between them; three where the last one is cut short by a clipped string); literals in front fill the frame to a whole
    number of rows"""
    out = []
    for m, steps in ((4, 140), (8, 140)):
        pal, trans = gs.colour_palette(max(2, (1 << m) // 2), 50 + m), (1 << m) // 4
        for form, stairs in (("lds", 1), ("global", 2)):
            w = 97 if form == "lds" else 131
            # clipped last strings: the frame ends `room` bytes into them, room and length - room each 1, 63, 64 and 65 where they fit
            tails = [(kind, L, room) for kind, L in (("copy", 130), ("kwkwk", 65), ("kwkwk", 129)) if m == 4
                     for room in sorted({r for o in GIF_OVERRUNS for r in (o, L - o) if 0 < r < L})]
            for tail in [None] + tails:
                s = [rng.integers(0, 1 << m, steps) for _ in range(stairs + (tail is not None and form == "global"))]
                lits = rng.integers(0, 1 << m, w)

                def build(pad):
                    c = _Codes(m)
                    for v in lits[:pad]:
                        c.emit(int(v), 1)
                    for k in range(len(s)):
                        if k:
                            c.clear()
                        _staircase(c, s[k], GIF_COPY_LENGTHS, tail[:2] if tail and k == len(s) - 1 else None)
                    return c, c.out if tail is None else c.out - tail[1] + tail[2]  # (a clipped last string gives `room` bytes)

                c, total = build(-build(0)[1] % w)
                assert total % w == 0 and (total <= GIF_LDS_FRAME) == (form == "lds"), (m, form, tail, total)
                name = f"stairs-m{m}-{form}" + (f"-{tail[0]}{tail[1]}-room{tail[2]}" if tail else "")
                out.append(_gif_raw(name, c, m, w, total // w, pal, trans))
    return out


def gif_grid():
    """{'expand_rows': screens 5 .. 9 px wide and 1023 .. 2049 rows tall, plain and interlaced, the frame on the screen, one row down and
    1020 rows down (clipped at the bottom), and interlaced frames of 1024 .. 1031 rows (every residue mod 8); 'expand_cols': screens of
    127 .. 130 px with the frame's left edge at 0, 1, 63, 64, 65 and its right edge at 63, 64, 65, 128, 129 and past the screen;
    'lzw_switch': frames of 16 383, 16 384 and 16 385 indices, of 16 369 .. 16 383 (every residue of the last 16-byte store) and of
    1 .. 33; 'lzw_copies': raw streams whose plain and KwKwK copies of 63 .. 129 bytes carry noise, on both sides of the switch, and
    last strings clipped by the frame's end}"""
    if "gif" not in _CACHE:
        rng = np.random.default_rng(2104)
        rows, cols, switch = [], [], []
        add = lambda group, name, pair: group.append((name, pair[0], pair[1]))
        add(rows, GIF_SMALL, _gif_image(rng, 5, 5))
        for k, h in enumerate(GIF_TALL):
            w = 5 + k % 5
            for il in (False, True):
                kind = "interlaced" if il else "plain"
                add(rows, f"rows-{kind}-{w}x{h}" + ("-opaque" if il == (k % 2 == 0) else ""), _gif_image(rng, w, h, opaque=il == (k % 2 == 0), interlace=il))
                for fy in (1, 1020):  # (the frame as tall as the screen: it reaches fy rows past the bottom)
                    add(rows, f"rows-{kind}-{w}x{h}-fy{fy}", _gif_image(rng, w, h, screen=(w, h), pos=(0, fy), interlace=il))
        for fh in range(1024, 1032):
            add(rows, f"rows-interlaced-frame5x{fh}-fy0", _gif_image(rng, 5, fh, interlace=True))
            add(rows, f"rows-interlaced-frame5x{fh}-fy3", _gif_image(rng, 5, fh, screen=(5, fh + 5), pos=(0, 3), interlace=True))
        for w in (127, 128, 129, 130):
            for fx in (0, 1, 63, 64, 65):
                for k, right in enumerate((63, 64, 65, 128, 129, w + 3)):
                    if right > fx:
                        add(cols, f"cols-{w}x6-fx{fx}-right{right}", _gif_image(rng, right - fx, 6, screen=(w, 6), pos=(fx, 0), interlace=k % 2 == 1))
        exact = [(127, 129), (128, 128), (16384, 1), (1, 16384), (145, 113)]
        below = [(n, 1) if n % 2 else (1, n) for n in range(16369, 16383)]
        small = [(n, 1) if n % 2 else (1, n) for n in range(1, 34)]
        for k, (w, h) in enumerate(exact + below + small):
            for j, (colours, clear) in enumerate(((4, "never"), (256, "full"), (4, "full"), (256, "never"))):
                if (w, h) in exact or (k + j) % 4 == 0:  # the exact sizes take all four contents, the others one each in turn
                    opaque = (k + j) % 2 == 0
                    add(switch, f"switch-{w}x{h}-c{colours}-{clear}" + ("-opaque" if opaque else ""), _gif_image(rng, w, h, colours, opaque, clear=clear))
        grid = dict(expand_rows=rows, expand_cols=cols, lzw_switch=switch, lzw_copies=_gif_copies(rng))
        for files in grid.values():
            for name, _, px in files:
                _PIXELS[("gif", name)] = px
        _CACHE["gif"] = {g: [(n, d) for n, d, _ in files] for g, files in grid.items()}
    return _CACHE["gif"]


# ------------------------------------------------------------------ BMP
# The expand kernel's work item is a band of max(1, 2048 / G) rows of an image, G = ceil(w / 4) groups of four pixels; its 256 threads
# walk the band's rows * G groups flattened, stepping by (256 / G, 256 % G) and carrying a group overflow into the row.
BMP_GROUPS_PER_ITEM, BMP_THREADS = 2048, 256
BMP_KEPT = ((1, 2049), (9, 683), (1025, 15), (8193, 3))  # every variant and row order
BMP_THINNED = ((4, 2048), (5, 1025), (10, 1365), (17, 410), (25, 293), (1021, 9), (1024, 8), (8192, 3))  # size k: the variants with (k + variant) % 4 == 0


def bmp_walk(w, h):
    """the kernel's formulas restated: G, band, (dr, dg), the rows of every work item, the trips of thread 0 through a full item and
    the carries (g >= G) of all threads in it"""
    G = (w + 3) // 4
    band = max(1, BMP_GROUPS_PER_ITEM // G)
    dr, dg = BMP_THREADS // G, BMP_THREADS % G
    items = [min(band, h - row0) for row0 in range(0, h, band)]
    total = items[0] * G
    carries = 0
    for t in range(min(BMP_THREADS, total)):
        g = t % G
        for _ in range(t, total, BMP_THREADS):
            g += dg
            if g >= G:
                g, carries = g - G, carries + 1
    return dict(G=G, band=band, clamped=BMP_GROUPS_PER_ITEM // G == 0, dr=dr, dg=dg, items=items, trips=-(-total // BMP_THREADS), carries=carries)


def bmp_name(variant, top_down, w, h):
    return f"{variant}-{'topdown' if top_down else 'bottomup'}-{w}x{h}"


def bmp_grid():
    """{'bands': the 16 variants in both row orders (RLE: bottom-up) at the sizes where the band walk of the expand kernel changes:
    one group per row and eight trips, a last item of one row, steps that carry on every third trip, more groups than threads, more
    groups than an item holds}"""
    if "bmp" not in _CACHE:
        bands = []
        for v, variant in enumerate(bs.VARIANTS):
            sizes = list(BMP_KEPT) + [s for k, s in enumerate(BMP_THINNED) if (k + v) % 4 == 0]
            for w, h in sizes:
                for td in bs.ROW_ORDERS:
                    if td and variant.startswith("rle"):
                        continue
                    data, px = bs.make(variant, w, h, td, seed=2105)
                    bands.append((bmp_name(variant, td, w, h), data))
                    _PIXELS[("bmp", bands[-1][0])] = px
        _CACHE["bmp"] = dict(bands=bands)
    return _CACHE["bmp"]


# ------------------------------------------------------------------ references
GRIDS = dict(png=(png_grid, pu), tiff=(tiff_grid, tu), webp=(webp_grid, wu), gif=(gif_grid, _Built), bmp=(bmp_grid, _Built))


def references(fmt, group, hashes=True, layout=None):
    """[(name, file, reference pixels, BLAKE3 of their to_rgba16 or None)] of one group, or of the files of one layout in it (the
    first part of their names); each file is decoded (GIF and BMP: rendered by its builder) and hashed once per process"""
    grid, util = GRIDS[fmt]
    out = []
    for name, data in grid()[group]:
        if layout is not None and name.split("-")[0] != layout:
            continue
        item = _REFS.get((fmt, name))
        if item is None:
            ref = _PIXELS.get((fmt, name))
            if ref is None:
                st, ref = util.decode(data)
                assert st == 0, name
            ref.setflags(write=False)
            item = _REFS[(fmt, name)] = [name, data, ref, None]
        out.append(item)
    if hashes:
        todo = [item for item in out if item[3] is None]
        for item, digest in zip(todo, b3.blake3_many([util.to_rgba16(item[2]) for item in todo])):
            item[3] = digest
    return [tuple(item) for item in out]
