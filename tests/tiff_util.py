"""TIFF test helpers built on numpy and the standard library (no Pillow needed): a writer with every knob of the TIFF section of
include/rupphash.h (byte order, strips of any RowsPerStrip, tiles, the four compressions with its own LZW and PackBits encoders,
predictor, every sample layout, LZW streams with and without EOI and with Clear codes in mid-strip, tag overrides for damaged files); an
independent reference decoder returning (status, pixels) by the rule (a classic string-table LZW, zlib for Deflate); corpora."""
import struct
import zlib

import numpy as np

OK, INVALID, UNSUPPORTED = 0, -1, -5
SHORT, LONG = 3, 4
(T_WIDTH, T_LENGTH, T_BPS, T_COMPRESSION, T_PHOTOMETRIC, T_FILLORDER, T_STRIPOFFSETS, T_SPP, T_ROWSPERSTRIP, T_STRIPBYTECOUNTS, T_PLANAR, T_PREDICTOR,
 T_TILEWIDTH, T_TILELENGTH, T_TILEOFFSETS, T_TILEBYTECOUNTS, T_EXTRASAMPLES, T_SAMPLEFORMAT) = (256, 257, 258, 259, 262, 266, 273, 277, 278, 279, 284, 317,
                                                                                                   322, 323, 324, 325, 338, 339)
READ_TAGS = {T_WIDTH, T_LENGTH, T_BPS, T_COMPRESSION, T_PHOTOMETRIC, T_FILLORDER, T_STRIPOFFSETS, T_SPP, T_ROWSPERSTRIP, T_STRIPBYTECOUNTS, T_PLANAR,
             T_PREDICTOR, T_TILEWIDTH, T_TILELENGTH, T_TILEOFFSETS, T_TILEBYTECOUNTS, T_SAMPLEFORMAT}
ARRAY_TAGS = {T_BPS, T_STRIPOFFSETS, T_STRIPBYTECOUNTS, T_TILEOFFSETS, T_TILEBYTECOUNTS, T_SAMPLEFORMAT}
LZW_MAX_STRING = 3839


# ---------------------------------------------------------------- compressors

class _MsbWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, k):
        self.acc = (self.acc << k) | (v & ((1 << k) - 1))
        self.n += k
        while self.n >= 8:
            self.n -= 8
            self.out.append((self.acc >> self.n) & 255)
        self.acc &= (1 << self.n) - 1

    def done(self):
        if self.n:
            self.out.append((self.acc << (8 - self.n)) & 255)
        return bytes(self.out)


def lzw_encode(data, eoi=True, clear_every=None, first_clear=True, never_clear=False):
    """TIFF LZW: MSB-first codes of 9-12 bits, early change, Clear at 4094 entries.  clear_every: a Clear after that many codes
    (mid-strip); never_clear: let the table grow past its end (a stream the rule refuses)."""
    w = _MsbWriter()
    table, nxt, width = {}, 258, 9
    if first_clear:
        w.put(256, 9)
    cur, since = b"", 0
    for b in data:
        wc = cur + bytes([b])
        if len(wc) == 1 or wc in table:
            cur = wc
            continue
        w.put(cur[0] if len(cur) == 1 else table[cur], width)
        since += 1
        if (clear_every and since >= clear_every) or (nxt + 1 >= 4094 and not never_clear):
            if nxt + 1 >= (1 << width) and width < 12:  # (the reader has added its entry for this code)
                width += 1
            w.put(256, width)
            table, nxt, width, since = {}, 258, 9, 0
        else:
            table[wc] = nxt
            nxt += 1
            if nxt >= (1 << width) and width < 12:
                width += 1
        cur = bytes([b])
    if cur:
        w.put(cur[0] if len(cur) == 1 else table[cur], width)
        nxt += 1
        if nxt >= (1 << width) and width < 12:
            width += 1
    if eoi:
        w.put(257, width)
    return w.done()


def packbits_encode(data, row=None):
    """rows of `row` bytes are packed one by one, as the TIFF text asks"""
    out = bytearray()
    row = row or max(1, len(data))
    for r0 in range(0, len(data), row):
        d = data[r0:r0 + row]
        i = 0
        while i < len(d):
            j = i
            while j + 1 < len(d) and d[j + 1] == d[i] and j - i < 127:
                j += 1
            if j - i >= 2:
                out += bytes([257 - (j - i + 1), d[i]])
                i = j + 1
                continue
            j = i
            while j < len(d) and j - i < 128 and not (j + 2 < len(d) and d[j] == d[j + 1] == d[j + 2]):
                j += 1
            out += bytes([j - i - 1]) + bytes(d[i:j])
            i = j
    return bytes(out)


def compress(raw, compression, row=None, level=6, lzw=None):
    if compression == 1:
        return bytes(raw)
    if compression == 5:
        return lzw_encode(bytes(raw), **(lzw or {}))
    if compression in (8, 32946):
        return zlib.compress(bytes(raw), level)
    if compression == 32773:
        return packbits_encode(bytes(raw), row)
    raise ValueError(compression)


# ---------------------------------------------------------------- writer

def _pack_rows(s, bps, bo):
    """(rows, n) stored samples -> (rows, rowbytes) uint8"""
    s = np.asarray(s, np.int64)
    if bps == 16:
        hi, lo = (s >> 8) & 255, s & 255
        pair = [hi, lo] if bo == ">" else [lo, hi]
        return np.stack(pair, axis=-1).reshape(s.shape[0], -1).astype(np.uint8)
    if bps == 8:
        return s.astype(np.uint8)
    per = 8 // bps
    rows, n = s.shape
    s = np.concatenate([s, np.zeros((rows, (-n) % per), np.int64)], axis=1).reshape(rows, -1, per)
    return (s << np.array([8 - bps * (k + 1) for k in range(per)])).sum(axis=2).astype(np.uint8)


def segment_rows(samples, bps, bo="<", predictor=1, rows_per_strip=None, tile=None):
    """[(raw bytes, row bytes)] of the image's strips or tiles (tiles padded with zeros), predictor applied"""
    s = np.asarray(samples, np.int64)
    if s.ndim == 2:
        s = s[:, :, None]
    h, w, spp = s.shape
    blocks = []
    if tile:
        tw, th = tile
        for y0 in range(0, h, th):
            for x0 in range(0, w, tw):
                t = np.zeros((th, tw, spp), np.int64)
                sub = s[y0:y0 + th, x0:x0 + tw]
                t[:sub.shape[0], :sub.shape[1]] = sub
                blocks.append(t)
    else:
        rps = min(rows_per_strip or h, h)
        blocks = [s[y0:y0 + rps] for y0 in range(0, h, rps)]
    out = []
    for t in blocks:
        if predictor == 2:
            t = np.concatenate([t[:, :1], np.diff(t, axis=1)], axis=1) & ((1 << bps) - 1)
        rows = _pack_rows(t.reshape(t.shape[0], -1), bps, bo)
        out.append((rows.tobytes(), rows.shape[1]))
    return out


def write(tags, segments, bo="<", tiled=False, version=42, bom=None, with_counts=True, second_ifd=False):
    """tags: {tag: (type, [values])} without offsets / byte counts; segments: compressed bytes of each strip or tile"""
    E = bo
    body = bytearray()
    offs = []
    for sg in segments:
        offs.append(8 + len(body))
        body += sg
        if len(body) & 1:
            body += b"\0"
    tags = dict(tags)
    tags.setdefault(T_TILEOFFSETS if tiled else T_STRIPOFFSETS, (LONG, offs))
    if with_counts:
        tags.setdefault(T_TILEBYTECOUNTS if tiled else T_STRIPBYTECOUNTS, (LONG, [len(sg) for sg in segments]))
    tags = {t: v for t, v in tags.items() if v is not None}
    entries = bytearray()
    for tag in sorted(tags):
        typ, vals = tags[tag][0], list(tags[tag][1])
        count = tags[tag][2] if len(tags[tag]) > 2 else len(vals)
        fmt = {1: "B", SHORT: "H", LONG: "I"}[typ]
        payload = struct.pack(E + fmt * len(vals), *vals)
        if len(payload) <= 4:
            field = payload.ljust(4, b"\0")
        else:
            field = struct.pack(E + "I", 8 + len(body))
            body += payload
            if len(body) & 1:
                body += b"\0"
        entries += struct.pack(E + "HHI", tag, typ, count) + field
    ifd = 8 + len(body)
    out = (bom or (b"II" if bo == "<" else b"MM")) + struct.pack(E + "HI", version, ifd) + bytes(body)
    nxt = ifd + 2 + len(entries) + 4 if second_ifd else 0
    out += struct.pack(E + "H", len(tags)) + bytes(entries) + struct.pack(E + "I", nxt)
    if second_ifd:
        out += struct.pack(E + "H", 1) + struct.pack(E + "HHII", T_WIDTH, LONG, 1, 7) + struct.pack(E + "I", 0)
    return out


def base_tags(w, h, spp, bps, photometric, compression, predictor=1, rows_per_strip=None, tile=None):
    tags = {T_WIDTH: (LONG, [w]), T_LENGTH: (LONG, [h]), T_BPS: (SHORT, [bps] * spp), T_COMPRESSION: (SHORT, [compression]),
            T_PHOTOMETRIC: (SHORT, [photometric]), T_SPP: (SHORT, [spp]), T_PLANAR: (SHORT, [1])}
    if tile:
        tags[T_TILEWIDTH] = (SHORT, [tile[0]])
        tags[T_TILELENGTH] = (SHORT, [tile[1]])
    elif rows_per_strip:
        tags[T_ROWSPERSTRIP] = (LONG, [rows_per_strip])
    if predictor != 1:
        tags[T_PREDICTOR] = (SHORT, [predictor])
    if spp in (2, 4):
        tags[T_EXTRASAMPLES] = (SHORT, [2])
    return tags


def encode(samples, photometric=None, bps=8, bo="<", compression=1, predictor=1, rows_per_strip=None, tile=None, level=6, lzw=None, override=None,
           segment_edit=None, **wkw):
    """samples: (h, w) or (h, w, spp) stored sample values in the file's depth.  override: {tag: (type, values[, count]) or None (the tag is
    left out)}.  segment_edit: f(list of compressed segments) -> list"""
    s = np.asarray(samples)
    if s.ndim == 2:
        s = s[:, :, None]
    h, w, spp = s.shape
    if photometric is None:
        photometric = 2 if spp >= 3 else 1
    segs = [compress(raw, compression, rb, level, lzw) for raw, rb in segment_rows(s, bps, bo, predictor, rows_per_strip, tile)]
    if segment_edit:
        segs = segment_edit(segs)
    tags = base_tags(w, h, spp, bps, photometric, compression, predictor, rows_per_strip, tile)
    tags.update(override or {})
    return write(tags, segs, bo, tiled=tile is not None, **wkw)


# ---------------------------------------------------------------- reference decoder

def lzw_decode(data, cap):
    """cap bytes, or None by the rule: a string table of byte strings (the classic statement of the decoder)"""
    nbits, pos = len(data) * 8, 0
    big = int.from_bytes(data, "big") if data else 0
    out = bytearray()
    table, nxt, width, prev, after_clear = {}, 258, 9, None, False
    while len(out) < cap:
        if pos + width > nbits:
            return None
        code = (big >> (nbits - pos - width)) & ((1 << width) - 1)
        pos += width
        if code == 256:
            if after_clear:
                return None
            table, nxt, width, prev, after_clear = {}, 258, 9, None, True
            continue
        if code == 257:
            return None
        if prev is None:
            if code >= 256:
                return None
            s = bytes([code])
        elif code < 256:
            s = bytes([code])
        elif code < nxt:
            s = table[code]
        elif code == nxt:
            s = prev + prev[:1]
        else:
            return None
        after_clear = False
        room = cap - len(out)
        out += s[:room]
        if len(s) >= room:
            break
        if prev is not None:
            if nxt >= 4096:
                return None
            table[nxt] = prev + s[:1]
            nxt += 1
            if nxt + 1 >= (1 << width) and width < 12:
                width += 1
        prev = s
    return bytes(out)


def packbits_decode(data, cap):
    out, pos = bytearray(), 0
    while len(out) < cap:
        if pos >= len(data):
            return None
        c = data[pos]
        pos += 1
        if c == 128:
            continue
        if c < 128:
            if len(data) - pos < c + 1:
                return None
            out += data[pos:pos + c + 1]
            pos += c + 1
        else:
            if pos >= len(data):
                return None
            out += bytes([data[pos]]) * (257 - c)
            pos += 1
    return bytes(out[:cap])


def inflate(data, cap):
    try:
        d = zlib.decompressobj()
        raw = d.decompress(data)
        if not d.eof or len(raw) < cap:
            return None
    except zlib.error:
        return None
    return raw[:cap]


def max_expansion(comp, n):
    return {1: n, 5: LZW_MAX_STRING * (n * 8 // 9), 8: 1032 * n, 32773: 64 * n}[comp]


def parse(data):
    """(status, info) by the rule of include/rupphash.h, in the order it states"""
    n = len(data)
    if n < 8:
        return INVALID, None
    if data[:2] == b"II":
        E = "<"
    elif data[:2] == b"MM":
        E = ">"
    else:
        return INVALID, None
    version, ifd = struct.unpack(E + "HI", data[2:8])
    if version == 43:
        return UNSUPPORTED, None
    if version != 42 or ifd > n or n - ifd < 2:
        return INVALID, None
    cnt = struct.unpack(E + "H", data[ifd:ifd + 2])[0]
    if (n - ifd - 2) // 12 < cnt:
        return INVALID, None
    f = {}
    for e in range(cnt):
        at = ifd + 2 + 12 * e
        tag, typ, count = struct.unpack(E + "HHI", data[at:at + 8])
        if tag not in READ_TAGS:
            continue
        if typ not in (SHORT, LONG) or count == 0 or (tag not in ARRAY_TAGS and count != 1):
            return INVALID, None
        size = count * (2 if typ == SHORT else 4)
        off = at + 8
        if size > 4:
            off = struct.unpack(E + "I", data[at + 8:at + 12])[0]
            if off > n or n - off < size:
                return INVALID, None
        f[tag] = list(struct.unpack(E + ("H" if typ == SHORT else "I") * count, data[off:off + size]))
    if T_WIDTH not in f or T_LENGTH not in f:
        return INVALID, None
    w, h = f[T_WIDTH][0], f[T_LENGTH][0]
    if not w or not h:
        return INVALID, None
    g = lambda t, d: f[t][0] if t in f else d
    spp, comp, planar, fill, pred = g(T_SPP, 1), g(T_COMPRESSION, 1), g(T_PLANAR, 1), g(T_FILLORDER, 1), g(T_PREDICTOR, 1)
    bps = f.get(T_BPS, [1])
    if spp == 0 or len(bps) != spp:
        return INVALID, None
    photo = g(T_PHOTOMETRIC, 1 if spp <= 2 else 2)
    if comp not in (1, 5, 8, 32946, 32773) or fill != 1 or (planar != 1 and spp > 1) or photo > 2 or any(b != bps[0] for b in bps):
        return UNSUPPORTED, None
    if any(s != 1 for s in f.get(T_SAMPLEFORMAT, [])):
        return UNSUPPORTED, None
    if spp not in ((3, 4) if photo == 2 else (1, 2)):
        return UNSUPPORTED, None
    b = bps[0]
    if b not in ((1, 2, 4, 8, 16) if spp == 1 else (8, 16)):
        return UNSUPPORTED, None
    if pred != 1 and (pred != 2 or comp in (1, 32773) or b < 8):
        return UNSUPPORTED, None
    tiled = T_TILEWIDTH in f or T_TILELENGTH in f or T_TILEOFFSETS in f
    if tiled:
        if not (T_TILEWIDTH in f and T_TILELENGTH in f and T_TILEOFFSETS in f):
            return INVALID, None
        sw, sh = f[T_TILEWIDTH][0], f[T_TILELENGTH][0]
        if not sw or not sh:
            return INVALID, None
    else:
        if T_STRIPOFFSETS not in f:
            return INVALID, None
        sw, sh = w, g(T_ROWSPERSTRIP, h)
        if not sh:
            return INVALID, None
        sh = min(sh, h)
    sx, sy = -(-w // sw), -(-h // sh)
    rb = (sw * spp * b + 7) // 8
    if w * h > 1 << 28 or rb > 1 << 30 or sh * rb > 1 << 30 or (sx * sy * sh * rb if tiled else h * rb) > 1 << 30:
        return UNSUPPORTED, None
    offs, cnts = f.get(T_TILEOFFSETS if tiled else T_STRIPOFFSETS), f.get(T_TILEBYTECOUNTS if tiled else T_STRIPBYTECOUNTS)
    if len(offs) != sx * sy:
        return INVALID, None
    if (len(cnts) != sx * sy) if cnts is not None else comp != 1:
        return INVALID, None
    comp = 8 if comp == 32946 else comp
    segs = []
    for k in range(sx * sy):
        rows = sh if tiled else (h - k * sh if k + 1 == sx * sy else sh)
        dec = rows * rb
        c = cnts[k] if cnts is not None else dec
        if offs[k] > n or c > n - offs[k]:
            return INVALID, None
        segs.append((offs[k], c, dec, rows))
    if any(dec > max_expansion(comp, c) for _, c, dec, _ in segs):
        return UNSUPPORTED, None
    return OK, dict(w=w, h=h, spp=spp, bps=b, comp=comp, photo=photo, pred=pred, tiled=tiled, sw=sw, sh=sh, sx=sx, sy=sy, rb=rb, segs=segs, E=E)


def info(data):
    """(status, (w, h, channels, bit depth)) as rph_tiff_info"""
    st, i = parse(data)
    return (st, None) if st else (OK, (i["w"], i["h"], i["spp"], 16 if i["bps"] == 16 else 8))


def decode(data):
    """(status, native array or None): what rph_tiff_decode_host must give"""
    st, i = parse(data)
    if st != OK:
        return st, None
    w, h, spp, b = i["w"], i["h"], i["spp"], i["bps"]
    img = np.zeros((i["sy"] * i["sh"], i["sx"] * i["sw"], spp), np.int64)
    for k, (off, c, dec, rows) in enumerate(i["segs"]):
        src = data[off:off + c]
        raw = {1: lambda: src[:dec], 5: lambda: lzw_decode(src, dec), 8: lambda: inflate(src, dec), 32773: lambda: packbits_decode(src, dec)}[i["comp"]]()
        if raw is None:
            return INVALID, None
        a = np.frombuffer(raw, np.uint8).reshape(rows, i["rb"])
        if b == 16:
            a = a.astype(np.int64)
            s = (a[:, 0::2] << 8 | a[:, 1::2]) if i["E"] == ">" else (a[:, 1::2] << 8 | a[:, 0::2])
        elif b == 8:
            s = a.astype(np.int64)
        else:
            bits = np.unpackbits(a, axis=1)[:, :i["sw"] * b].reshape(rows, i["sw"], b)
            s = (bits * (1 << np.arange(b - 1, -1, -1))).sum(axis=2)
        s = s[:, :i["sw"] * spp].reshape(rows, i["sw"], spp)
        if i["pred"] == 2:
            s = np.cumsum(s, axis=1) & ((1 << b) - 1)
        y0, x0 = (k // i["sx"]) * i["sh"], (k % i["sx"]) * i["sw"]
        img[y0:y0 + rows, x0:x0 + i["sw"]] = s
    img = img[:h, :w]
    maxv = (1 << b) - 1
    if i["photo"] == 0:
        img = maxv - img
    if b < 8:
        img = img * (255 // maxv)
    img = img.astype(np.uint16 if b == 16 else np.uint8)
    return OK, img[:, :, 0] if spp == 1 else img


def to_rgba16(img):
    """to_rgba16() of a native array as little-endian bytes (what the pixel hash hashes)"""
    a = np.asarray(img)
    v = a.astype(np.uint32) * (257 if a.dtype == np.uint8 else 1)
    if v.ndim == 2:
        v = v[:, :, None]
    c = v.shape[2]
    if c == 1:
        v = np.concatenate([v, v, v, np.full_like(v, 65535)], axis=-1)
    elif c == 2:
        v = np.concatenate([v[:, :, :1]] * 3 + [v[:, :, 1:]], axis=-1)
    elif c == 3:
        v = np.concatenate([v, np.full_like(v[:, :, :1], 65535)], axis=-1)
    return v.astype("<u2").tobytes()


def hasher_pixels(img):
    """The 8-bit pixels PDQ sees (to_luma601 input): Luma8 as it is, LumaA8 as (l, l, l, a), 16-bit through round(v / 257)"""
    a = np.asarray(img)
    if a.dtype == np.uint16:
        v = ((a.astype(np.uint32) + 128) // 257).astype(np.uint8)
        if v.ndim == 2:
            v = v[:, :, None]
        return np.repeat(v[:, :, :1], 3, axis=2) if v.shape[2] <= 2 else np.ascontiguousarray(v[:, :, :3])
    if a.ndim == 2:
        return a
    if a.shape[2] == 2:
        return np.concatenate([a[:, :, :1]] * 3 + [a[:, :, 1:]], axis=-1)
    return a


# ---------------------------------------------------------------- corpora

LAYOUTS = [(1, 1, 1), (1, 1, 2), (1, 1, 4), (1, 1, 8), (1, 1, 16), (0, 1, 1), (0, 1, 4), (0, 1, 8), (0, 1, 16), (1, 2, 8), (1, 2, 16), (0, 2, 8),
           (2, 3, 8), (2, 3, 16), (2, 4, 8), (2, 4, 16)]  # (photometric, samples, bits)
COMPRESSIONS = (1, 5, 8, 32946, 32773)


def random_samples(rng, h, w, spp, bps, smooth=True):
    top = (1 << bps) - 1
    if smooth:
        yy, xx = np.mgrid[0:h, 0:w]
        base = (xx * 7 + yy * 3)[:, :, None] + np.arange(spp)[None, None, :] * 11
        noise = rng.integers(0, max(2, (top + 1) // 16), (h, w, spp))
        return ((base * max(1, (top + 1) // 64) + noise) % (top + 1)).astype(np.int64)
    return rng.integers(0, top + 1, (h, w, spp)).astype(np.int64)


def make_file(rng, w, h, photo=2, spp=3, bps=8, **kw):
    return encode(random_samples(rng, h, w, spp, bps), photo, bps, **kw)


def valid_corpus(seed=7):
    """(name, bytes): every sample layout x compression, strips and tiles, both byte orders, predictor where the rule takes it"""
    rng = np.random.default_rng(seed)
    out = []
    k = 0
    for photo, spp, bps in LAYOUTS:
        for comp in COMPRESSIONS:
            for tiled in (False, True):
                w, h = int(rng.integers(1, 50)), int(rng.integers(1, 40))
                bo = "<>"[k & 1]
                pred = 2 if (comp in (5, 8, 32946) and bps >= 8 and (k >> 1) & 1) else 1
                kw = dict(tile=[(16, 16), (32, 16), (7, 5), (48, 64)][k % 4]) if tiled else dict(rows_per_strip=[None, 1, 3, 8, 100][k % 5])
                out.append((f"p{photo}_s{spp}_b{bps}_c{comp}_{'tile' if tiled else 'strip'}_{'le' if bo == '<' else 'be'}_pr{pred}_{w}x{h}",
                            make_file(rng, w, h, photo, spp, bps, bo=bo, compression=comp, predictor=pred, **kw)))
                k += 1
    for bo in "<>":
        for spp, bps in [(3, 8), (3, 16), (4, 16), (1, 16), (2, 8)]:
            for comp in (5, 8):
                out.append((f"pred2_s{spp}_b{bps}_c{comp}_{bo == '<' and 'le' or 'be'}", make_file(rng, 37, 21, 2 if spp >= 3 else 1, spp, bps, bo=bo, compression=comp,
                                                                                                  predictor=2, tile=(16, 16) if comp == 5 else None, rows_per_strip=4)))
    for w, h in [(1, 1), (4, 4), (5, 5), (64, 1), (1, 64), (65, 3), (129, 2)]:
        out.append((f"lzw_{w}x{h}", make_file(rng, w, h, compression=5, predictor=2)))
    noise = rng.integers(0, 256, (90, 90)).astype(np.int64)
    out.append(("lzw_table_fills", encode(noise, compression=5)))  # one strip of 8100 random bytes: the writer sends Clear at 4094
    out.append(("lzw_no_eoi", encode(noise[:20, :30], compression=5, lzw=dict(eoi=False))))
    out.append(("lzw_clear_mid_strip", encode(noise[:40, :40], compression=5, lzw=dict(clear_every=37))))
    out.append(("lzw_no_first_clear", encode(noise[:9, :9], compression=5, lzw=dict(first_clear=False))))
    out.append(("lzw_runs", encode(np.zeros((50, 300, 3), np.int64) + 9, compression=5, rows_per_strip=10)))  # KwKwK after KwKwK
    out.append(("lzw_runs_pred", encode(np.tile(np.arange(300)[None, :, None] * 2 % 256, (30, 1, 3)), compression=5, predictor=2)))
    out.append(("packbits_runs", encode(np.zeros((20, 400), np.int64) + 3, compression=32773)))
    out.append(("deflate_stored", make_file(rng, 45, 17, compression=8, level=0)))
    out.append(("deflate_l9", make_file(rng, 45, 17, compression=8, level=9, predictor=2)))
    out.append(("no_rows_per_strip", make_file(rng, 20, 30, compression=5)))
    out.append(("rows_per_strip_above_height", make_file(rng, 20, 9, compression=1, override={T_ROWSPERSTRIP: (LONG, [0xFFFFFFFF])})))
    out.append(("no_byte_counts_uncompressed", make_file(rng, 20, 12, rows_per_strip=5, with_counts=False)))
    out.append(("no_photometric", make_file(rng, 11, 9, override={T_PHOTOMETRIC: None})))
    out.append(("second_ifd", make_file(rng, 11, 9, compression=5, second_ifd=True)))
    out.append(("unknown_tags", make_file(rng, 11, 9, override={274: (SHORT, [6]), 305: (SHORT, [1, 2, 3, 4, 5]), 65000: (LONG, [1])})))
    out.append(("short_width_tag", make_file(rng, 11, 9, override={T_WIDTH: (SHORT, [11]), T_LENGTH: (SHORT, [9])})))
    out.append(("big_tile", make_file(rng, 40, 30, compression=5, predictor=2, tile=(128, 128))))  # 48 KiB: built in global memory
    out.append(("big_strip", encode(random_samples(rng, 80, 100, 3, 8, smooth=False), compression=5)))
    return out


def _lzw_codes(codes):
    """codes written at the widths a reader would be at: [(code, width)]"""
    w = _MsbWriter()
    for c, k in codes:
        w.put(c, k)
    return w.done()


def rule_corpus():
    """(name, bytes, expected status): one file per line of the rule and per cell of the UNSUPPORTED column"""
    rng = np.random.default_rng(11)
    s = random_samples(rng, 8, 8, 1, 8)[:, :, 0]
    rgb = random_samples(rng, 8, 8, 3, 8)
    raw = s.astype(np.uint8).tobytes()
    good = encode(s)
    out = []
    one = lambda name, st, **kw: out.append((name, encode(kw.pop("img", s), **kw), st))
    seg = lambda b: (lambda segs: [b])
    out.append(("good", good, OK))
    out.append(("bad_byte_order", b"IM" + good[2:], INVALID))
    one("bad_version", INVALID, version=41)
    one("bigtiff", UNSUPPORTED, version=43)
    out.append(("ifd_offset_outside", good[:4] + struct.pack("<I", len(good) + 1), INVALID))
    ifd = struct.unpack("<I", good[4:8])[0]
    out.append(("entry_count_outside", good[:ifd] + struct.pack("<H", 200) + good[ifd + 2:], INVALID))
    out.append(("ifd_cut", good[:-40], INVALID))
    one("value_array_outside", INVALID, img=rgb, override={T_BPS: (SHORT, [0xFFF0, 0], 3)})
    one("strip_outside", INVALID, override={T_STRIPBYTECOUNTS: (LONG, [5000])})
    one("strip_offset_outside", INVALID, override={T_STRIPOFFSETS: (LONG, [0x7FFFFFFF])})
    one("missing_width", INVALID, override={T_WIDTH: None})
    one("missing_length", INVALID, override={T_LENGTH: None})
    one("missing_offsets", INVALID, override={T_STRIPOFFSETS: None})
    one("missing_byte_counts_lzw", INVALID, compression=5, with_counts=False)
    one("byte_type_width", INVALID, override={T_WIDTH: (1, [8])})
    one("width_count_2", INVALID, override={T_WIDTH: (SHORT, [8, 8])})
    one("bps_count_mismatch", INVALID, override={T_BPS: (SHORT, [8, 8])})
    one("zero_width", INVALID, override={T_WIDTH: (LONG, [0])})
    one("zero_height", INVALID, override={T_LENGTH: (LONG, [0])})
    one("zero_rows_per_strip", INVALID, override={T_ROWSPERSTRIP: (LONG, [0])})
    one("zero_tile_width", INVALID, tile=(16, 16), override={T_TILEWIDTH: (SHORT, [0])})
    one("tile_length_missing", INVALID, tile=(16, 16), override={T_TILELENGTH: None})
    one("zero_samples", INVALID, override={T_SPP: (SHORT, [0])})
    one("strip_count_mismatch", INVALID, rows_per_strip=2, override={T_ROWSPERSTRIP: (LONG, [3])})
    one("count_array_mismatch", INVALID, rows_per_strip=2, override={T_STRIPBYTECOUNTS: (LONG, [16, 16, 16])})
    # LZW
    lz = lambda name, st, codes: one(name, st, compression=5, segment_edit=seg(_lzw_codes(codes) + bytes(80)))
    lz("lzw_clear_clear", INVALID, [(256, 9), (256, 9), (65, 9)])
    lz("lzw_first_code_258", INVALID, [(256, 9), (258, 9)])
    lz("lzw_first_code_eoi", INVALID, [(256, 9), (257, 9)])
    lz("lzw_no_clear_first_code_300", INVALID, [(300, 9)])
    lz("lzw_code_above_next", INVALID, [(256, 9), (65, 9), (66, 9), (260, 9)])
    lz("lzw_early_eoi", INVALID, [(256, 9), (65, 9), (66, 9), (257, 9)])
    lz("lzw_kwkwk_ok", OK, [(256, 9), (65, 9), (258, 9), (259, 9), (260, 9), (261, 9), (262, 9), (263, 9), (264, 9), (265, 9), (266, 9), (267, 9)])
    full = lzw_encode(raw)
    one("lzw_truncated", INVALID, compression=5, segment_edit=seg(full[:len(full) // 2]))
    one("lzw_trailing_garbage", OK, compression=5, segment_edit=seg(lzw_encode(raw, eoi=False) + b"\xff\x00\xff"))
    noise = rng.integers(0, 256, (90, 90)).astype(np.int64)
    one("lzw_table_overflow", INVALID, img=noise, compression=5, lzw=dict(never_clear=True))
    # PackBits
    pk = lambda name, st, b: one(name, st, compression=32773, segment_edit=seg(b))
    pk("packbits_cut_literal", INVALID, bytes([63]) + raw[:40])
    pk("packbits_cut_run", INVALID, bytes([31]) + raw[:32] + bytes([0x81]))
    pk("packbits_runs_out", INVALID, bytes([31]) + raw[:32])
    pk("packbits_extra_runs", OK, bytes([63]) + raw + bytes([0x81, 7, 0x81]))
    pk("packbits_overlong_run", OK, bytes([60]) + raw[:61] + bytes([257 - 100, 9]))
    pk("packbits_noop", OK, bytes([128, 63]) + raw)
    # Deflate
    z = zlib.compress(raw)
    zf = lambda name, st, b: one(name, st, compression=8, segment_edit=seg(b))
    zf("deflate_adler", INVALID, z[:-1] + bytes([z[-1] ^ 1]))
    zf("deflate_short", INVALID, zlib.compress(raw[:-1]))
    zf("deflate_truncated", INVALID, z[:-6])
    zf("deflate_header", INVALID, b"\x79" + z[1:])
    zf("deflate_tail_in_stream", OK, zlib.compress(raw + b"extra bytes"))
    zf("deflate_after_adler", OK, z + b"junk")
    # left to the caller's decoders
    one("planar_2", UNSUPPORTED, img=rgb, override={T_PLANAR: (SHORT, [2])})
    one("fill_order_2", UNSUPPORTED, override={T_FILLORDER: (SHORT, [2])})
    for c in (2, 3, 4, 6, 7, 34712, 50000):
        one(f"compression_{c}", UNSUPPORTED, override={T_COMPRESSION: (SHORT, [c])})
    for p in (3, 5, 6, 8, 32803):
        one(f"photometric_{p}", UNSUPPORTED, img=rgb if p != 3 else s, override={T_PHOTOMETRIC: (SHORT, [p])})
    one("unequal_bits", UNSUPPORTED, img=rgb, override={T_BPS: (SHORT, [8, 8, 16])})
    one("five_samples", UNSUPPORTED, img=random_samples(rng, 8, 8, 5, 8), photometric=2)
    one("rgb_photometric_one_sample", UNSUPPORTED, photometric=2)
    one("gray_three_samples", UNSUPPORTED, img=rgb, photometric=1)
    one("sample_format_float", UNSUPPORTED, override={T_SAMPLEFORMAT: (SHORT, [3])})
    one("sample_format_signed", UNSUPPORTED, override={T_SAMPLEFORMAT: (SHORT, [2])})
    one("gray_3_bit", UNSUPPORTED, override={T_BPS: (SHORT, [3])})
    one("gray_32_bit", UNSUPPORTED, override={T_BPS: (SHORT, [32])})
    one("rgb_4_bit", UNSUPPORTED, img=rgb, override={T_BPS: (SHORT, [4, 4, 4])})
    one("predictor_3", UNSUPPORTED, compression=5, override={T_PREDICTOR: (SHORT, [3])})
    one("predictor_2_4_bit", UNSUPPORTED, img=s % 16, bps=4, compression=5, override={T_PREDICTOR: (SHORT, [2])})
    one("predictor_2_uncompressed", UNSUPPORTED, override={T_PREDICTOR: (SHORT, [2])})
    one("predictor_2_packbits", UNSUPPORTED, compression=32773, override={T_PREDICTOR: (SHORT, [2])})
    # implausible or too large
    one("bomb", UNSUPPORTED, compression=8, override={T_WIDTH: (LONG, [30000]), T_LENGTH: (LONG, [30000])})
    one("too_many_bytes", UNSUPPORTED, img=np.zeros((8, 8, 4), np.int64), bps=16, compression=8, override={T_WIDTH: (LONG, [16000]), T_LENGTH: (LONG, [16000])})
    one("deflate_implausible", UNSUPPORTED, compression=8, override={T_WIDTH: (LONG, [4000]), T_LENGTH: (LONG, [4000])})
    one("lzw_implausible", UNSUPPORTED, compression=5, override={T_WIDTH: (LONG, [4000]), T_LENGTH: (LONG, [4000])})
    one("packbits_implausible", UNSUPPORTED, compression=32773, override={T_WIDTH: (LONG, [100]), T_LENGTH: (LONG, [100])})
    one("uncompressed_short_strip", UNSUPPORTED, override={T_LENGTH: (LONG, [9])})
    return out


def random_damage(data, rng):
    b = bytearray(data)
    k = int(rng.integers(0, 5))
    ifd = struct.unpack(("<" if b[:2] == b"II" else ">") + "I", b[4:8])[0]
    if k == 0:  # bytes overwritten anywhere
        for _ in range(int(rng.integers(1, 4))):
            b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
    elif k == 1:  # truncation
        b = b[:int(rng.integers(1, len(b)))]
    elif k == 2:  # a bit flipped inside the strips and tiles
        if ifd > 9:
            b[int(rng.integers(8, min(ifd, len(b))))] ^= 1 << int(rng.integers(0, 8))
    elif k == 3:  # an offset, count or value of the IFD edited
        if ifd + 2 < len(b):
            b[int(rng.integers(ifd, len(b)))] = int(rng.integers(0, 256))
    else:  # bytes taken out of the data (every later offset is off)
        i = int(rng.integers(8, len(b)))
        b = b[:i] + b[i + int(rng.integers(1, 9)):]
    return bytes(b)


def damaged_corpus(seed=2026, n_random=200):
    """(name, bytes): the rule corpus plus seeded random damage of valid files"""
    rng = np.random.default_rng(seed)
    base = valid_corpus(seed)
    out = [(n, d) for n, d, _ in rule_corpus()]
    for k in range(n_random):
        name, d = base[int(rng.integers(0, len(base)))]
        out.append((f"rand{k}_{name}", random_damage(d, rng)))
    return out
