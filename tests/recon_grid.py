"""Grids of files for the stages behind the entropy decoders: the PNG unfilter kernel, the TIFF expand kernel and the WebP inverse
transforms and table slots.  Every grid puts the sizes where wave-shaped code goes wrong (rows and pixels 63 / 64 / 65 and 127 / 128 /
129, units of 1 to 8 bytes, every sample layout, every filter or predictor mode) under noise, so that running sums wrap, Paeth takes
all three branches, the clamping modes saturate at both ends and select meets ties (a share of every image holds only 0 and the
maximum).  Seeded, built once per process, (name, bytes) lists per group; references() decodes each file once with the plain Python
decoders and hashes what the pixel hash hashes."""
import os
import re

import numpy as np

import blake3_util as b3
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


# ------------------------------------------------------------------ references
GRIDS = dict(png=(png_grid, pu), tiff=(tiff_grid, tu), webp=(webp_grid, wu))


def references(fmt, group, hashes=True, layout=None):
    """[(name, file, reference pixels, BLAKE3 of their to_rgba16 or None)] of one group, or of the files of one layout in it (the
    first part of their names); each file is decoded and hashed once per process"""
    grid, util = GRIDS[fmt]
    out = []
    for name, data in grid()[group]:
        if layout is not None and name.split("-")[0] != layout:
            continue
        item = _REFS.get((fmt, name))
        if item is None:
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
