"""PNG test helpers built on zlib and numpy (no Pillow needed): an encoder for every colour type, bit depth, filter, zlib setting and
IDAT split; a reference decoder (zlib.decompress, a numpy unfilter, the EXPAND rules of include/rupphash.h); to_rgba16; a seeded
damaged corpus with one file per item of the damaged-file rule plus random damage and truncation."""
import struct
import zlib

import numpy as np

SIG = b"\x89PNG\r\n\x1a\n"
OK, INVALID, UNSUPPORTED = 0, -1, -5
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
DEPTHS = {0: (1, 2, 4, 8, 16), 2: (8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 6: (8, 16)}
ADAM7 = [(0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)]


def chunk(ctype, body):
    return struct.pack(">I", len(body)) + ctype + body + struct.pack(">I", zlib.crc32(ctype + body) & 0xFFFFFFFF)


def passes(w, h, interlace):
    """[(x0, y0, dx, dy, pw, ph)] of the passes that hold pixels"""
    out = []
    for x0, y0, dx, dy in (ADAM7 if interlace else [(0, 0, 1, 1)]):
        pw = (w - x0 + dx - 1) // dx if w > x0 else 0
        ph = (h - y0 + dy - 1) // dy if h > y0 else 0
        if pw and ph:
            out.append((x0, y0, dx, dy, pw, ph))
    return out


def pack_rows(samples, depth):
    """samples (rows, cols * nch) ints -> (rows, rowbytes) uint8 in PNG order"""
    s = np.asarray(samples, np.int64)
    if depth == 16:
        return np.stack([(s >> 8) & 255, s & 255], axis=-1).reshape(s.shape[0], -1).astype(np.uint8)
    if depth == 8:
        return s.astype(np.uint8)
    per = 8 // depth
    rows, n = s.shape
    pad = (-n) % per
    s = np.concatenate([s, np.zeros((rows, pad), np.int64)], axis=1).reshape(rows, -1, per)
    shifts = np.array([8 - depth * (k + 1) for k in range(per)])
    return (s << shifts).sum(axis=2).astype(np.uint8)


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_row(f, row, prev, bpp):
    x = row.astype(np.int64)
    b = prev.astype(np.int64)
    a = np.concatenate([np.zeros(min(bpp, len(x)), np.int64), x[:max(0, len(x) - bpp)]])
    c = np.concatenate([np.zeros(min(bpp, len(b)), np.int64), b[:max(0, len(b) - bpp)]])
    pred = 0 * x if f == 0 else a if f == 1 else b if f == 2 else (a + b) >> 1 if f == 3 else _paeth(a, b, c)
    return ((x - pred) & 255).astype(np.uint8)


def encode(samples, ctype, depth, palette=None, trns=None, interlace=False, filters="adaptive", level=6, strategy=zlib.Z_DEFAULT_STRATEGY,
           wbits=15, idat_split=None, extra_chunks=(), after_iend=b"", raw_tail=b""):
    """samples: (h, w, nch) or (h, w) ints in the file's depth (palette images: indices).  filters: an int 0-4 for every row,
    "adaptive" (min-sum-abs), or a list cycled over the rows.  idat_split: int chunk size or list of sizes.  raw_tail: bytes appended
    to the image inside the zlib stream."""
    s = np.asarray(samples)
    if s.ndim == 2:
        s = s[:, :, None]
    h, w, nch = s.shape
    assert nch == CHANNELS[ctype]
    bpp = max(1, nch * depth // 8)
    raw = bytearray()
    k = 0
    for x0, y0, dx, dy, pw, ph in passes(w, h, interlace):
        sub = s[y0::dy, x0::dx][:ph, :pw].reshape(ph, pw * nch)
        rows = pack_rows(sub, depth)
        prev = np.zeros(rows.shape[1], np.uint8)
        for r in rows:
            if filters == "adaptive":
                cands = [filter_row(f, r, prev, bpp) for f in range(5)]
                f = int(np.argmin([np.abs(c.astype(np.int8).astype(np.int64)).sum() for c in cands]))
                fr = cands[f]
            else:
                f = filters if isinstance(filters, int) else filters[k % len(filters)]
                fr = filter_row(f, r, prev, bpp)
            raw += bytes([f]) + fr.tobytes()
            prev = r
            k += 1
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy)
    z = co.compress(bytes(raw) + raw_tail) + co.flush()
    ihdr = struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, 1 if interlace else 0)
    out = SIG + chunk(b"IHDR", ihdr)
    if palette is not None:
        out += chunk(b"PLTE", np.asarray(palette, np.uint8).reshape(-1).tobytes())
    if trns is not None:
        out += chunk(b"tRNS", trns)
    for c in extra_chunks:
        out += c
    if idat_split is None:
        parts = [z]
    else:
        sizes = idat_split if isinstance(idat_split, (list, tuple)) else [idat_split]
        parts, i, j = [], 0, 0
        while i < len(z):
            n = max(1, sizes[j % len(sizes)])
            parts.append(z[i:i + n])
            i += n
            j += 1
    for p in parts:
        out += chunk(b"IDAT", p)
    return out + chunk(b"IEND", b"") + after_iend


def trns_gray(key):
    return struct.pack(">H", key)


def trns_rgb(r, g, b):
    return struct.pack(">HHH", r, g, b)


# ---------------------------------------------------------------- reference decoder

def parse(data):
    """(status, info) by the rule of include/rupphash.h"""
    if len(data) < 8 or data[:8] != SIG:
        return INVALID, None
    info = dict(plte=None, trns=None, idat=b"")
    pos, have_plte, ihdr = 8, False, None
    while len(data) - pos >= 12:
        n = struct.unpack(">I", data[pos:pos + 4])[0]
        t = data[pos + 4:pos + 8]
        if n > 0x7FFFFFFF or n > len(data) - pos - 12:
            break
        body = data[pos + 8:pos + 8 + n]
        if t == b"IEND":
            break
        if zlib.crc32(t + body) & 0xFFFFFFFF != struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0]:
            return INVALID, None
        if ihdr is None:
            if t != b"IHDR" or n != 13:
                return INVALID, None
            w, h, d, ct, cm, fm, im = struct.unpack(">IIBBBBB", body)
            if not w or not h or w > 0x7FFFFFFF or h > 0x7FFFFFFF or ct not in DEPTHS or d not in DEPTHS[ct] or cm or fm or im > 1:
                return INVALID, None
            ihdr = (w, h, d, ct, im)
        elif t == b"IHDR":
            return INVALID, None
        elif t == b"PLTE":
            if have_plte or n == 0 or n % 3 or n > 768:
                return INVALID, None
            have_plte = True
            if ihdr[3] in (2, 3, 6):
                info["plte"] = np.frombuffer(body, np.uint8).reshape(-1, 3)
        elif t == b"tRNS":
            ct = ihdr[3]
            if ct == 0 and n == 2:
                info["trns"] = struct.unpack(">H", body)
            elif ct == 2 and n == 6:
                info["trns"] = struct.unpack(">HHH", body)
            elif ct == 3 and 1 <= n <= 256:
                info["trns"] = np.frombuffer(body, np.uint8)
        elif t == b"IDAT":
            info["idat"] += body
        elif not t[0] & 0x20:
            return INVALID, None
        pos += n + 12
    if ihdr is None or (ihdr[3] == 3 and not have_plte):
        return INVALID, None
    w, h, d, ct, im = ihdr
    info.update(w=w, h=h, depth=d, ctype=ct, interlace=im)
    nch = CHANNELS[ct]
    info["passes"] = [(p, (pw * nch * d + 7) // 8) for p in passes(w, h, im) for pw in [p[4]]]
    raw = sum(p[5] * (1 + rb) for p, rb in info["passes"])
    info["raw_bytes"] = raw
    if raw > 1032 * len(info["idat"]) or raw > (1 << 30) or w * h > (1 << 28):
        return UNSUPPORTED, info
    return OK, info


def unfilter(raw, rows, rowbytes, bpp):
    """raw: bytes of rows * (1 + rowbytes) -> (rows, rowbytes) uint8, or None for a filter type above 4"""
    a = np.frombuffer(raw, np.uint8).reshape(rows, 1 + rowbytes)
    out = np.zeros((rows, rowbytes), np.int64)
    prev = np.zeros(rowbytes, np.int64)
    for y in range(rows):
        f = int(a[y, 0])
        x = a[y, 1:].astype(np.int64)
        if f > 4:
            return None
        if f == 0:
            r = x
        elif f == 2:
            r = (x + prev) & 255
        elif f == 1:
            r = x.copy()
            for i in range(bpp, rowbytes):
                r[i] = (r[i] + r[i - bpp]) & 255
        else:
            r = x.copy()
            for i in range(rowbytes):
                left = r[i - bpp] if i >= bpp else 0
                up = prev[i]
                ul = prev[i - bpp] if i >= bpp else 0
                if f == 3:
                    r[i] = (r[i] + ((left + up) >> 1)) & 255
                else:
                    p = left + up - ul
                    pa, pb, pc = abs(p - left), abs(p - up), abs(p - ul)
                    r[i] = (r[i] + (left if pa <= pb and pa <= pc else up if pb <= pc else ul)) & 255
        out[y] = r
        prev = r
    return out.astype(np.uint8)


def unpack_rows(rows, depth, n):
    """(rows, rowbytes) -> (rows, n) sample ints"""
    if depth == 16:
        r = rows.astype(np.uint32)
        return (r[:, 0::2] << 8 | r[:, 1::2])[:, :n]
    if depth == 8:
        return rows[:, :n].astype(np.uint32)
    bits = np.unpackbits(rows, axis=1)[:, :n * depth].reshape(rows.shape[0], n, depth)
    return (bits * (1 << np.arange(depth - 1, -1, -1))).sum(axis=2).astype(np.uint32)


def decode(data):
    """(status, native array or None): what rph_png_decode_host must give"""
    st, info = parse(data)
    if st != OK:
        return st, None
    try:
        d = zlib.decompressobj()
        raw = d.decompress(info["idat"])
        if not d.eof:
            return INVALID, None
    except zlib.error:
        return INVALID, None
    if len(raw) < info["raw_bytes"]:
        return INVALID, None
    w, h, depth, ct = info["w"], info["h"], info["depth"], info["ctype"]
    nch = CHANNELS[ct]
    bpp = max(1, nch * depth // 8)
    samples = np.zeros((h, w, nch), np.uint32)
    off = 0
    for (x0, y0, dx, dy, pw, ph), rb in info["passes"]:
        rows = unfilter(raw[off:off + ph * (1 + rb)], ph, rb, bpp)
        if rows is None:
            return INVALID, None
        off += ph * (1 + rb)
        samples[y0::dy, x0::dx][:ph, :pw] = unpack_rows(rows, depth, pw * nch).reshape(ph, pw, nch)
    return OK, expand(samples, info)


def expand(s, info):
    depth, ct, trns = info["depth"], info["ctype"], info["trns"]
    maxv = 65535 if depth == 16 else 255
    dt = np.uint16 if depth == 16 else np.uint8
    if ct == 0:
        g = s[:, :, 0]
        v = g * (255 // ((1 << depth) - 1)) if depth < 8 else g
        if trns is None:
            return v.astype(dt)
        return np.stack([v, np.where(g == trns[0], 0, maxv)], axis=-1).astype(dt)
    if ct == 2:
        if trns is None:
            return s.astype(dt)
        a = np.where((s[:, :, 0] == trns[0]) & (s[:, :, 1] == trns[1]) & (s[:, :, 2] == trns[2]), 0, maxv)
        return np.concatenate([s, a[:, :, None]], axis=-1).astype(dt)
    if ct == 3:
        pal = info["plte"]
        idx = s[:, :, 0]
        n = len(pal)
        rgb = np.zeros(idx.shape + (3,), np.uint8)
        ok = idx < n
        rgb[ok] = pal[idx[ok]]
        if trns is None:
            return rgb
        alpha_tab = np.full(256, 255, np.uint8)
        t = trns[:n]
        alpha_tab[:len(t)] = t
        a = np.where(ok, alpha_tab[np.minimum(idx, 255)], 255).astype(np.uint8)
        return np.concatenate([rgb, a[:, :, None]], axis=-1)
    return s.astype(dt)


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

def random_samples(rng, h, w, ctype, depth, smooth=True):
    nch = CHANNELS[ctype]
    top = (1 << depth) - 1
    if ctype == 3:
        top = min(top, 255)
    if smooth:
        yy, xx = np.mgrid[0:h, 0:w]
        base = (xx * 7 + yy * 3)[:, :, None] + np.arange(nch)[None, None, :] * 11
        noise = rng.integers(0, max(2, (top + 1) // 16), (h, w, nch))
        v = (base * max(1, (top + 1) // 64) + noise) % (top + 1)
    else:
        v = rng.integers(0, top + 1, (h, w, nch))
    return v.astype(np.int64)


def layouts():
    """(ctype, depth, with_trns) for every colour type and depth"""
    out = []
    for ct, ds in DEPTHS.items():
        for d in ds:
            out.append((ct, d, False))
            if ct in (0, 2, 3):
                out.append((ct, d, True))
    return out


def make_file(rng, w, h, ct, d, with_trns, interlace=False, **kw):
    s = random_samples(rng, h, w, ct, d)
    palette = trns = None
    if ct == 3:
        n = int(rng.integers(1, 1 << d)) if d < 8 else int(rng.integers(2, 257))
        palette = rng.integers(0, 256, (n, 3))
        s = s % (n + 1)  # some indices past the palette
        if with_trns:
            trns = rng.integers(0, 256, int(rng.integers(1, n + 1))).astype(np.uint8).tobytes()
    elif with_trns:
        key = [int(s[0, 0, c]) for c in range(CHANNELS[ct])]
        trns = trns_gray(key[0]) if ct == 0 else trns_rgb(*key)
    return encode(s, ct, d, palette=palette, trns=trns, interlace=interlace, **kw)


def valid_corpus(seed=7):
    """(name, bytes): every layout, interlaced and not, filters, zlib settings, IDAT splits"""
    rng = np.random.default_rng(seed)
    out = []
    for ct, d, t in layouts():
        for il in (False, True):
            w, h = int(rng.integers(1, 40)), int(rng.integers(1, 30))
            out.append((f"ct{ct}_d{d}_t{int(t)}_i{int(il)}_{w}x{h}", make_file(rng, w, h, ct, d, t, interlace=il)))
    for w, h in [(1, 1), (3, 7), (9, 1), (1, 9), (8, 8), (5, 5), (4, 4)]:
        out.append((f"adam7_{w}x{h}", make_file(rng, w, h, 2, 8, False, interlace=True)))
    for f in range(5):
        out.append((f"filter{f}", make_file(rng, 33, 21, 6, 8, False, filters=f)))
        out.append((f"filter{f}_16", make_file(rng, 17, 9, 2, 16, False, filters=f)))
        out.append((f"filter{f}_1bit", make_file(rng, 29, 70, 0, 1, False, filters=f)))
    out.append(("filter_cycle", make_file(rng, 31, 23, 2, 8, False, filters=[0, 1, 2, 3, 4, 4, 3])))
    out.append(("tall_paeth", make_file(rng, 7, 150, 4, 8, False, filters=4)))
    for lvl, strat, name in [(0, zlib.Z_DEFAULT_STRATEGY, "stored"), (1, zlib.Z_DEFAULT_STRATEGY, "l1"), (9, zlib.Z_DEFAULT_STRATEGY, "l9"),
                             (6, zlib.Z_FIXED, "fixed"), (6, zlib.Z_RLE, "rle"), (6, zlib.Z_HUFFMAN_ONLY, "huffman")]:
        out.append((f"zlib_{name}", make_file(rng, 45, 17, 2, 8, False, level=lvl, strategy=strat)))
    for wb in range(9, 16):
        out.append((f"wbits{wb}", make_file(rng, 40, 40, 0, 8, False, wbits=wb)))
    out.append(("idat_1byte", make_file(rng, 12, 10, 6, 8, False, idat_split=1)))
    out.append(("idat_mixed", make_file(rng, 30, 20, 2, 8, False, idat_split=[3, 1, 50, 7])))
    # 32 KiB distances and 258-byte lengths: a random block repeated 32 KiB later, and long runs
    blk = rng.integers(0, 256, (64, 128, 4))
    big = np.concatenate([blk, blk], axis=0)  # rows of 513 bytes: the repeat lies 32 832 bytes back
    out.append(("far_copies", encode(big, 6, 8, filters=0, level=9)))
    out.append(("long_runs", encode(np.zeros((40, 300, 3), np.int64) + 9, 2, 8, filters=0, level=9)))
    out.append(("rle_runs", encode(np.zeros((20, 200), np.int64) + 3, 0, 8, filters=1, strategy=zlib.Z_RLE)))
    out.append(("tail_in_stream", make_file(rng, 10, 10, 2, 8, False, raw_tail=bytes(5000))))
    out.append(("after_iend", make_file(rng, 10, 10, 2, 8, False, after_iend=b"garbage after IEND")))
    out.append(("ancillary", make_file(rng, 10, 10, 2, 8, False, extra_chunks=[chunk(b"tEXt", b"k\x00v"), chunk(b"gAMA", b"\x00\x00\xb1\x8f")])))
    no_iend = make_file(rng, 10, 10, 2, 8, False)
    out.append(("no_iend", no_iend[:-12]))
    return out


def _recrc(data, pos):
    """fix the CRC of the chunk at pos"""
    n = struct.unpack(">I", data[pos:pos + 4])[0]
    body = bytes(data[pos + 4:pos + 8 + n])
    data[pos + 8 + n:pos + 12 + n] = struct.pack(">I", zlib.crc32(body) & 0xFFFFFFFF)


def _idat_pos(data):
    pos = 8
    while True:
        n = struct.unpack(">I", data[pos:pos + 4])[0]
        if data[pos + 4:pos + 8] == b"IDAT":
            return pos, n
        pos += n + 12


def _with_zlib(samples_file_kw, z):
    """a file whose single IDAT holds z"""
    s, ct, d = samples_file_kw
    ihdr = struct.pack(">IIBBBBB", s.shape[1], s.shape[0], d, ct, 0, 0, 0)
    return SIG + chunk(b"IHDR", ihdr) + chunk(b"IDAT", z) + chunk(b"IEND", b"")


def _zlib_raw(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
    return co.compress(raw) + co.flush()


def _adler(b):
    return struct.pack(">I", zlib.adler32(b) & 0xFFFFFFFF)


def rule_corpus():
    """(name, bytes, expected status): one file per item of the damaged-file rule"""
    rng = np.random.default_rng(11)
    s = random_samples(rng, 8, 8, 0, 8)[:, :, 0]
    good = bytearray(encode(s, 0, 8, filters=0))
    raw = b"".join(b"\x00" + bytes(r) for r in s.astype(np.uint8))
    geo = (s, 0, 8)
    out = []
    out.append(("bad_signature", b"\x89PNG\r\n\x1b\n" + bytes(good[8:]), INVALID))
    b = bytearray(good)
    b[8 + 4:8 + 8] = b"IHDX"
    out.append(("ihdr_not_first", bytes(b), INVALID))
    for name, field, val in [("ihdr_zero_width", 0, b"\x00\x00\x00\x00"), ("ihdr_bad_depth", 8, b"\x03"), ("ihdr_bad_ctype", 9, b"\x05"),
                             ("ihdr_compression", 10, b"\x01"), ("ihdr_filter", 11, b"\x01"), ("ihdr_interlace", 12, b"\x02")]:
        b = bytearray(good)
        b[16 + field:16 + field + len(val)] = val
        _recrc(b, 8)
        out.append((name, bytes(b), INVALID))
    b = bytearray(good)
    p, n = _idat_pos(b)
    b[p + 8 + n] ^= 1
    out.append(("crc_mismatch", bytes(b), INVALID))
    out.append(("unknown_critical", bytes(good[:33]) + chunk(b"ABCD", b"x") + bytes(good[33:]), INVALID))
    out.append(("unknown_ancillary", bytes(good[:33]) + chunk(b"abCD", b"x") + bytes(good[33:]), OK))
    out.append(("missing_plte", encode(s % 4, 3, 8, filters=0)[:33] + encode(s % 4, 3, 8, filters=0, palette=[[1, 2, 3]] * 4)[33 + 24:], INVALID))
    out.append(("second_ihdr", bytes(good[:33]) + bytes(good[8:33]) + bytes(good[33:]), INVALID))
    # zlib
    z = bytearray(_zlib_raw(raw))
    for name, mut in [("zlib_cm", lambda q: q.__setitem__(0, 0x79)), ("zlib_cinfo", lambda q: q.__setitem__(0, 0x88)),
                      ("zlib_fcheck", lambda q: q.__setitem__(1, q[1] ^ 1))]:
        q = bytearray(z)
        mut(q)
        out.append((name, _with_zlib(geo, bytes(q)), INVALID))
    q = bytearray(z)
    q[1] |= 0x20
    q[1] = (q[1] & 0xE0) | ((31 - ((q[0] << 8) | (q[1] & 0xE0)) % 31) % 31)
    out.append(("zlib_fdict", _with_zlib(geo, bytes(q)), INVALID))
    out.append(("block_type_3", _with_zlib(geo, b"\x78\x01" + bytes([0b111])), INVALID))
    stored = b"\x78\x01" + bytes([1]) + struct.pack("<HH", len(raw), (~len(raw) + 1) & 0xFFFF) + raw + _adler(raw)
    out.append(("stored_nlen", _with_zlib(geo, stored), INVALID))
    ok_stored = b"\x78\x01" + bytes([1]) + struct.pack("<HH", len(raw), ~len(raw) & 0xFFFF) + raw + _adler(raw)
    out.append(("stored_ok", _with_zlib(geo, ok_stored), OK))
    # dynamic block headers written bit by bit
    out.append(("oversubscribed", _with_zlib(geo, b"\x78\x01" + _bits([(1, 1), (2, 2), (0, 5), (0, 5), (0, 4)] + [(7, 3)] * 4)), INVALID))
    out.append(("incomplete_cl", _with_zlib(geo, b"\x78\x01" + _bits([(1, 1), (2, 2), (0, 5), (0, 5), (0, 4)] + [(1, 3)] * 3 + [(0, 3)])), INVALID))
    out.append(("lit_286", _with_zlib(geo, b"\x78\x01" + _fixed_symbols([286])), INVALID))
    out.append(("dist_30", _with_zlib(geo, b"\x78\x01" + _fixed_symbols([65, ("len", 0, 30)])), INVALID))
    out.append(("dist_too_far", _with_zlib(geo, b"\x78\x01" + _fixed_symbols([65, ("len", 0, 1)])), INVALID))  # distance 2 after 1 byte
    q = bytearray(z)
    q[-1] ^= 1
    out.append(("adler", _with_zlib(geo, bytes(q)), INVALID))
    b = bytearray(encode(s, 0, 8, filters=0))
    out.append(("filter_5", _with_zlib(geo, _zlib_raw(b"\x05" + raw[1:])), INVALID))
    out.append(("short_stream", _with_zlib(geo, _zlib_raw(raw[:-1])), INVALID))
    out.append(("truncated_stream", _with_zlib(geo, bytes(z[:-6])), INVALID))
    out.append(("no_idat", bytes(good[:33]) + chunk(b"IEND", b""), UNSUPPORTED))
    # accepted
    out.append(("tail_in_stream", _with_zlib(geo, _zlib_raw(raw + b"extra bytes")), OK))
    out.append(("after_adler", _with_zlib(geo, bytes(z) + b"junk"), OK))
    out.append(("after_iend", bytes(good) + b"trailing", OK))
    out.append(("missing_iend", bytes(good[:-12]), OK))
    out.append(("cut_last_chunk", bytes(good[:-12]) + chunk(b"tEXt", b"abcdef")[:9], OK))
    # the plausibility bound
    bomb = bytearray(SIG + chunk(b"IHDR", struct.pack(">IIBBBBB", 30000, 30000, 8, 6, 0, 0, 0)) + chunk(b"IDAT", _zlib_raw(b"\x00" * 1000)) + chunk(b"IEND", b""))
    out.append(("bomb", bytes(bomb), UNSUPPORTED))
    return out


def _bits(fields):
    """LSB-first bit writer: fields (value, nbits)"""
    acc, n, out = 0, 0, bytearray()
    for v, k in fields:
        acc |= v << n
        n += k
    while n > 0:
        out.append(acc & 255)
        acc >>= 8
        n -= 8
    return bytes(out)


def _rev(v, n):
    return int(format(v, f"0{n}b")[::-1], 2)


def _fixed_code(sym):
    if sym < 144:
        return sym + 0x30, 8
    if sym < 256:
        return sym - 144 + 0x190, 9
    if sym < 280:
        return sym - 256, 7
    return sym - 280 + 0xC0, 8


def _fixed_symbols(items):
    """a final fixed block: literal ints, or ("len", length symbol offset, distance symbol) with no extra bits"""
    f = [(1, 1), (1, 2)]
    for it in items:
        if isinstance(it, tuple):
            code, n = _fixed_code(257 + it[1])
            f.append((_rev(code, n), n))
            f.append((_rev(it[2], 5), 5))
        else:
            code, n = _fixed_code(it)
            f.append((_rev(code, n), n))
    code, n = _fixed_code(256)
    f.append((_rev(code, n), n))
    return _bits(f) + b"\x00\x00\x00\x00"


def random_damage(data, rng):
    b = bytearray(data)
    k = int(rng.integers(0, 4))
    if k == 0:
        for _ in range(int(rng.integers(1, 4))):
            b[int(rng.integers(8, len(b)))] = int(rng.integers(0, 256))
    elif k == 1:
        b = b[:int(rng.integers(8, len(b)))]
    elif k == 2:
        p, n = _idat_pos(b)
        if n:
            b[p + 8 + int(rng.integers(0, n))] ^= 1 << int(rng.integers(0, 8))
            _recrc(b, p)  # damage the stream itself, past the CRC
    else:
        i = int(rng.integers(8, len(b)))
        b = b[:i] + bytes(rng.integers(0, 256, int(rng.integers(1, 9))).astype(np.uint8)) + b[i:]
    return bytes(b)


def damaged_corpus(seed=2026, n_random=200):
    """(name, bytes): the rule corpus plus seeded random damage and truncation of valid files"""
    rng = np.random.default_rng(seed)
    base = valid_corpus(seed)
    out = [(n, d) for n, d, _ in rule_corpus()]
    for k in range(n_random):
        name, d = base[int(rng.integers(0, len(base)))]
        out.append((f"rand{k}_{name}", random_damage(d, rng)))
    return out
