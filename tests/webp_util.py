"""Lossless WebP (VP8L) for the tests, plain Python and numpy, written from the format text: a reference decoder that applies the
damaged-file rule of include/rupphash.h (WebP section) by itself, a small writer that can force each feature of the format on its own,
and the corpora of named files the CPU and GPU tests share."""
import heapq
import struct

import numpy as np

INVALID, UNSUPPORTED = -1, -5
CODE_LENGTH_ORDER = [17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15]
# the neighbours (dx, dy) of distance codes 1 .. 120
PLANE = [(0, 1), (1, 0), (1, 1), (-1, 1), (0, 2), (2, 0), (1, 2), (-1, 2), (2, 1), (-2, 1), (2, 2), (-2, 2), (0, 3), (3, 0), (1, 3), (-1, 3), (3, 1),
         (-3, 1), (2, 3), (-2, 3), (3, 2), (-3, 2), (0, 4), (4, 0), (1, 4), (-1, 4), (4, 1), (-4, 1), (3, 3), (-3, 3), (2, 4), (-2, 4), (4, 2), (-4, 2),
         (0, 5), (3, 4), (-3, 4), (4, 3), (-4, 3), (5, 0), (1, 5), (-1, 5), (5, 1), (-5, 1), (2, 5), (-2, 5), (5, 2), (-5, 2), (4, 4), (-4, 4), (3, 5),
         (-3, 5), (5, 3), (-5, 3), (0, 6), (6, 0), (1, 6), (-1, 6), (6, 1), (-6, 1), (2, 6), (-2, 6), (6, 2), (-6, 2), (4, 5), (-4, 5), (5, 4), (-5, 4),
         (3, 6), (-3, 6), (6, 3), (-6, 3), (0, 7), (7, 0), (1, 7), (-1, 7), (5, 5), (-5, 5), (7, 1), (-7, 1), (4, 6), (-4, 6), (6, 4), (-6, 4), (2, 7),
         (-2, 7), (7, 2), (-7, 2), (3, 7), (-3, 7), (7, 3), (-7, 3), (5, 6), (-5, 6), (6, 5), (-6, 5), (8, 0), (4, 7), (-4, 7), (7, 4), (-7, 4), (8, 1),
         (8, 2), (6, 6), (-6, 6), (8, 3), (5, 7), (-5, 7), (7, 5), (-7, 5), (8, 4), (6, 7), (-6, 7), (7, 6), (-7, 6), (8, 5), (7, 7), (-7, 7), (8, 6),
         (8, 7)]
assert len(PLANE) == 120 and len(set(PLANE)) == 120


class Refused(Exception):
    def __init__(self, status, why):
        super().__init__(why)
        self.status = status


def sub(v, bits):
    return (v + (1 << bits) - 1) >> bits


def plane_distance(xsize, code):
    if code > 120:
        return code - 120
    dx, dy = PLANE[code - 1]
    return max(1, dx + dy * xsize)


def cache_key(argb, bits):
    return ((argb * 0x1e35a7bd) & 0xffffffff) >> (32 - bits)


# ------------------------------------------------------------------ reference decoder
class BitReader:
    def __init__(self, data, pos=0):
        self.d, self.pos = bytes(data), pos

    def take(self, k):
        """k bits, least significant first; zeros past the end, and `over` says so (the rule: refused once consumed)"""
        if k == 0:
            return 0
        p = self.pos >> 3
        v = int.from_bytes(self.d[p:p + 5], "little") >> (self.pos & 7)
        self.pos += k
        return v & ((1 << k) - 1)

    def peek(self, k):
        p = self.pos >> 3
        return (int.from_bytes(self.d[p:p + 4], "little") >> (self.pos & 7)) & ((1 << k) - 1)

    def check(self):
        if self.pos > 8 * len(self.d):
            raise Refused(INVALID, "out of bits")


class Code:
    """lengths -> canonical prefix code; a single symbol reads zero bits; anything else must be complete"""

    def __init__(self, lens):
        used = [(l, s) for s, l in enumerate(lens) if l]
        if not used:
            raise Refused(INVALID, "code without symbols")
        self.single = used[0][1] if len(used) == 1 else None
        if self.single is not None:
            return
        if sum(1 << (15 - l) for l, _ in used) != 1 << 15:
            raise Refused(INVALID, "over-subscribed or incomplete code")
        # every pattern of `width` bits as they come out of the stream (least significant first) -> (symbol, length)
        self.width = max(l for l, _ in used)
        self.table, code, prev = [None] * (1 << self.width), 0, 0
        for l, s in sorted(used):
            code <<= l - prev
            prev = l
            first = int(format(code, f"0{l}b")[::-1], 2)
            for k in range(first, 1 << self.width, 1 << l):
                self.table[k] = (s, l)
            code += 1

    def read(self, br):
        if self.single is not None:
            return self.single
        s, l = self.table[br.peek(self.width)]  # (a complete code assigns every pattern)
        br.pos += l
        return s


def _read_code(br, n):
    lens = [0] * max(n, 256)
    if br.take(1):
        two, first8 = br.take(1), br.take(1)
        lens[br.take(8 if first8 else 1)] = 1
        if two:
            lens[br.take(8)] = 1
    else:
        cl = [0] * 19
        for i in range(4 + br.take(4)):
            cl[CODE_LENGTH_ORDER[i]] = br.take(3)
        clc = Code(cl)
        max_symbol = n
        if br.take(1):
            nbits = 2 + 2 * br.take(3)
            max_symbol = 2 + br.take(nbits)
            if max_symbol > n:
                raise Refused(INVALID, "max_symbol above the alphabet")
        s, prev = 0, 8
        while s < n and max_symbol:
            max_symbol -= 1
            br.check()
            c = clc.read(br)
            if c < 16:
                lens[s] = c
                s += 1
                prev = c or prev
                continue
            rep = 3 + br.take(2) if c == 16 else 3 + br.take(3) if c == 17 else 11 + br.take(7)
            if s + rep > n:
                raise Refused(INVALID, "repeat past the alphabet")
            lens[s:s + rep] = [prev if c == 16 else 0] * rep
            s += rep
    br.check()
    return Code(lens[:n])


def _read_group(br, cache_bits):
    return [_read_code(br, n) for n in (280 + ((1 << cache_bits) if cache_bits else 0), 256, 256, 256, 40)]


def _read_cache_bits(br):
    if not br.take(1):
        return 0
    b = br.take(4)
    if not 1 <= b <= 11:
        raise Refused(INVALID, "colour cache size")
    return b


def _prefix(sym, br):
    if sym < 4:
        return sym + 1
    extra = (sym - 2) >> 1
    return ((2 + (sym & 1)) << extra) + br.take(extra) + 1


def _read_pixels(br, xsize, ysize, cache_bits, groups, ent=None, meta_bits=0):
    total, out = xsize * ysize, []
    cache = [0] * (1 << cache_bits) if cache_bits else None
    bw = sub(xsize, meta_bits)
    green_n = 280 + (len(cache) if cache else 0)

    def put(v):
        out.append(v)
        if cache is not None:
            cache[cache_key(v, cache_bits)] = v

    while len(out) < total:
        br.check()
        y, x = divmod(len(out), xsize)
        g = groups[ent[(y >> meta_bits) * bw + (x >> meta_bits)]] if ent is not None else groups[0]
        s = g[0].read(br)
        if s < 256:
            r, b, a = g[1].read(br), g[2].read(br), g[3].read(br)
            put(a << 24 | r << 16 | s << 8 | b)
        elif s < 280:
            n = _prefix(s - 256, br)
            dist = plane_distance(xsize, _prefix(g[4].read(br), br))
            br.check()
            if dist > len(out):
                raise Refused(INVALID, "distance before the first pixel")
            if n > total - len(out):
                raise Refused(INVALID, "copy past the last pixel")
            for _ in range(n):
                put(out[-dist])
        elif s < green_n:
            put(cache[s - 280])
        else:
            raise Refused(INVALID, "symbol past the alphabet")
    br.check()
    return out


def _read_sub_image(br, xsize, ysize):
    cache_bits = _read_cache_bits(br)
    return _read_pixels(br, xsize, ysize, cache_bits, [_read_group(br, cache_bits)])


def _ch(v):
    return (v >> 24, (v >> 16) & 255, (v >> 8) & 255, v & 255)


def _pack(c):
    return c[0] << 24 | c[1] << 16 | c[2] << 8 | c[3]


def _clip(v):
    return 0 if v < 0 else 255 if v > 255 else v


def _avg(a, b):
    return tuple((p + q) >> 1 for p, q in zip(a, b))


def predict(mode, L, T, TL, TR):
    """the format's 14 predictors on (a, r, g, b) tuples; 14 and 15 as 0 (libwebp)"""
    if mode == 1:
        return L
    if mode == 2:
        return T
    if mode == 3:
        return TR
    if mode == 4:
        return TL
    if mode == 5:
        return _avg(_avg(L, TR), T)
    if mode == 6:
        return _avg(L, TL)
    if mode == 7:
        return _avg(L, T)
    if mode == 8:
        return _avg(TL, T)
    if mode == 9:
        return _avg(T, TR)
    if mode == 10:
        return _avg(_avg(L, TL), _avg(T, TR))
    if mode == 11:
        # the estimate L + T - TL: its Manhattan distance to L is sum |T - TL|, to T sum |L - TL|; L when strictly nearer
        return L if sum(abs(t - tl) for t, tl in zip(T, TL)) < sum(abs(l - tl) for l, tl in zip(L, TL)) else T
    if mode == 12:
        return tuple(_clip(l + t - tl) for l, t, tl in zip(L, T, TL))
    if mode == 13:
        a = _avg(L, T)
        return tuple(_clip(p + int((p - q) / 2)) for p, q in zip(a, TL))
    return (255, 0, 0, 0)


def _add(a, b):
    return tuple((p + q) & 255 for p, q in zip(a, b))


def _s8(v):
    return v - 256 if v & 128 else v


def _inverse(px, h, tr):
    kind, bits, xsize, aux = tr
    bw = sub(xsize, bits)
    if kind == 0:
        c = [_ch(v) for v in px]
        for y in range(h):
            for x in range(xsize):
                q = y * xsize + x
                if y == 0:
                    p = (255, 0, 0, 0) if x == 0 else c[q - 1]
                elif x == 0:
                    p = c[q - xsize]
                else:
                    mode = (aux[(y >> bits) * bw + (x >> bits)] >> 8) & 15
                    p = predict(mode, c[q - 1], c[q - xsize], c[q - xsize - 1], c[q - xsize + 1])  # (last column: the next pixel in memory)
                c[q] = _add(c[q], p)
        return [_pack(v) for v in c]
    if kind == 1:
        out = []
        for q, v in enumerate(px):
            y, x = divmod(q, xsize)
            m = aux[(y >> bits) * bw + (x >> bits)]
            a, r, g, b = _ch(v)
            r = (r + ((_s8(m & 255) * _s8(g)) >> 5)) & 255
            b = (b + ((_s8((m >> 8) & 255) * _s8(g)) >> 5)) & 255
            b = (b + ((_s8((m >> 16) & 255) * _s8(r)) >> 5)) & 255
            out.append(_pack((a, r, g, b)))
        return out
    if kind == 2:
        return [_pack((a, (r + g) & 255, g, (b + g) & 255)) for a, r, g, b in map(_ch, px)]
    bpp, out = 8 >> bits, []
    for y in range(h):
        for x in range(xsize):
            packed = (px[y * bw + (x >> bits)] >> 8) & 255
            i = (packed >> ((x & ((1 << bits) - 1)) * bpp)) & ((1 << bpp) - 1)
            out.append(aux[i] if i < len(aux) else 0)
    return out


def parse(data):
    """container and VP8L header: (chunk payload, w, h, alpha); raises Refused by the rule"""
    data = bytes(data)
    if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"WEBP":
        raise Refused(INVALID, "tags")
    end = struct.unpack_from("<I", data, 4)[0] + 8
    if end > len(data) or end < 12:
        raise Refused(INVALID, "RIFF size")
    o, canvas = 12, None
    while True:
        if end - o < 8:
            raise Refused(INVALID, "no image chunk")
        tag, size = data[o:o + 4], struct.unpack_from("<I", data, o + 4)[0]
        if size > end - o - 8:
            raise Refused(INVALID, "chunk past the end")
        if tag in (b"VP8 ", b"ALPH", b"ANIM", b"ANMF"):
            raise Refused(UNSUPPORTED, "lossy or animated")
        if tag == b"VP8X" and o == 12:
            if size < 10:
                raise Refused(INVALID, "VP8X size")
            if data[o + 8] & 2:
                raise Refused(UNSUPPORTED, "animated")
            canvas = (int.from_bytes(data[o + 12:o + 15], "little") + 1, int.from_bytes(data[o + 15:o + 18], "little") + 1)
        if tag == b"VP8L":
            chunk = data[o + 8:o + 8 + size]
            break
        o += 8 + ((size + 1) & ~1)
        if o > end:
            raise Refused(INVALID, "chunk past the end")
    if len(chunk) < 5 or chunk[0] != 0x2f:
        raise Refused(INVALID, "signature")
    v = struct.unpack_from("<I", chunk, 1)[0]
    if v >> 29:
        raise Refused(INVALID, "version")
    w, h = (v & 0x3fff) + 1, ((v >> 14) & 0x3fff) + 1
    if canvas is not None and canvas != (w, h):
        raise Refused(INVALID, "canvas size")
    return chunk, w, h, (v >> 28) & 1


def info(data):
    try:
        _, w, h, alpha = parse(data)
    except Refused as e:
        return e.status, None
    return 0, (w, h, 4 if alpha else 3, 8)


def decode(data):
    """(status, pixels): (h, w, 3) or (h, w, 4) uint8 by the header's alpha bit, or (status, None) by the rule"""
    try:
        chunk, w, h, alpha = parse(data)
        br = BitReader(chunk, 40)
        transforms, seen, xsize = [], set(), w
        while br.take(1):
            kind = br.take(2)
            if kind in seen:
                raise Refused(INVALID, "transform twice")
            seen.add(kind)
            if kind in (0, 1):
                bits = br.take(3) + 2
                transforms.append((kind, bits, xsize, _read_sub_image(br, sub(xsize, bits), sub(h, bits))))
            elif kind == 2:
                transforms.append((kind, 0, xsize, None))
            else:
                n = br.take(8) + 1
                bits = 0 if n > 16 else 1 if n > 4 else 2 if n > 2 else 3
                pal = [_ch(v) for v in _read_sub_image(br, n, 1)]
                for k in range(1, n):
                    pal[k] = _add(pal[k], pal[k - 1])
                transforms.append((kind, bits, xsize, [_pack(c) for c in pal]))
                xsize = sub(xsize, bits)
            br.check()
        cache_bits = _read_cache_bits(br)
        ent, meta_bits, n_groups = None, 0, 1
        if br.take(1):
            meta_bits = br.take(3) + 2
            ent = [(v >> 8) & 0xffff for v in _read_sub_image(br, sub(xsize, meta_bits), sub(h, meta_bits))]
            n_groups = max(ent) + 1
            # the rule's bound on lookup tables, counted over the groups some block uses, before any code is read
            if len(set(ent)) * 2 * (1360 + 280 + ((1 << cache_bits) if cache_bits else 0) + 808) > 64 << 20:
                raise Refused(UNSUPPORTED, "more than 64 MiB of tables")
        br.check()
        groups = [_read_group(br, cache_bits) for _ in range(n_groups)]
        px = _read_pixels(br, xsize, h, cache_bits, groups, ent, meta_bits)
        for tr in reversed(transforms):
            px = _inverse(px, h, tr)
    except Refused as e:
        return e.status, None
    a = np.array(px, np.uint32).reshape(h, w)
    out = np.stack([(a >> 16) & 255, (a >> 8) & 255, a & 255, a >> 24], axis=-1).astype(np.uint8)
    return 0, out if alpha else np.ascontiguousarray(out[:, :, :3])


def to_rgba16(img):
    """to_rgba16() of an Rgb8 / Rgba8 image as little-endian bytes"""
    h, w, c = img.shape
    out = np.full((h, w, 4), 65535, np.uint16)
    out[:, :, :c] = img.astype(np.uint16) * 257
    return out.astype("<u2").tobytes()


# ------------------------------------------------------------------ writer
class BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, value, k):
        assert 0 <= value < (1 << k) or k == 0, (value, k)
        self.acc |= value << self.n
        self.n += k
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def put_many(self, values, counts):
        """put(values[i], counts[i]) for every i, as one array operation"""
        values, counts = np.asarray(values, np.uint32).ravel(), np.asarray(counts, np.int64).ravel()
        ends = np.cumsum(counts)
        which = np.repeat(np.arange(len(counts)), counts)
        bit = np.arange(int(ends[-1]) if len(ends) else 0) - (ends - counts)[which]
        bits = np.concatenate([np.array([(self.acc >> k) & 1 for k in range(self.n)], np.uint8), ((values[which] >> bit) & 1).astype(np.uint8)])
        whole = len(bits) // 8 * 8
        self.out += np.packbits(bits[:whole], bitorder="little").tobytes()
        self.acc, self.n = sum(int(b) << k for k, b in enumerate(bits[whole:])), len(bits) - whole

    def bytes(self):
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


def huffman_lengths(hist, limit=15):
    """code lengths for the counts in hist (0 = unused); complete whenever two or more symbols are used"""
    used = [s for s, c in enumerate(hist) if c]
    lens = [0] * len(hist)
    if len(used) == 1:
        lens[used[0]] = 1
        return lens
    counts = {s: hist[s] for s in used}
    while True:
        heap = [(c, s, (s,)) for s, c in counts.items()]
        heapq.heapify(heap)
        depth = dict.fromkeys(used, 0)
        while len(heap) > 1:
            c1, s1, m1 = heapq.heappop(heap)
            c2, s2, m2 = heapq.heappop(heap)
            for s in m1 + m2:
                depth[s] += 1
            heapq.heappush(heap, (c1 + c2, min(s1, s2), m1 + m2))
        if max(depth.values()) <= limit:
            break
        counts = {s: (c >> 1) + 1 for s, c in counts.items()}
    for s, d in depth.items():
        lens[s] = d
    return lens


def canonical(lens):
    """symbol -> (code, length), codes most significant bit first"""
    out, code, prev = {}, 0, 0
    for l, s in sorted((l, s) for s, l in enumerate(lens) if l):
        code <<= l - prev
        prev = l
        out[s] = (code, l)
        code += 1
    return out


class CodeWriter:
    def __init__(self, lens):
        used = [s for s, l in enumerate(lens) if l]
        self.single = len(used) == 1
        self.codes = canonical(lens)
        # the codes as the stream holds them: most significant bit first, so reversed for a writer of least significant bits first
        self.rev, self.len = np.zeros(len(lens), np.uint32), np.zeros(len(lens), np.int64)
        for s, (code, l) in self.codes.items():
            self.rev[s], self.len[s] = int(format(code, f"0{l}b")[::-1], 2), 0 if self.single else l

    def put(self, bw, s):
        assert s in self.codes
        bw.put(int(self.rev[s]), int(self.len[s]))


def write_code(bw, lens, simple=True, max_symbol=False, repeats=False, hack=None):
    """one prefix code; hack: 'over' / 'incomplete' / 'repeat_past' / 'max_symbol_big' damage it by the rule's items"""
    n = len(lens)
    used = [s for s, l in enumerate(lens) if l]
    if hack is None and simple and len(used) <= 2 and all(s < 256 for s in used) and all(lens[s] == 1 for s in used):
        bw.put(1, 1)
        bw.put(len(used) - 1, 1)
        first8 = used[0] > 1
        bw.put(int(first8), 1)
        bw.put(used[0], 8 if first8 else 1)
        if len(used) == 2:
            bw.put(used[1], 8)
        return
    lens = list(lens)
    if hack == "over":
        lens[[s for s in range(n) if not lens[s]][0]] = 1
    if hack == "incomplete":
        lens[max(used, key=lambda s: lens[s])] = 0
    bw.put(0, 1)
    top = max(s for s, l in enumerate(lens) if l) + 1 if max_symbol else n
    tokens, s = [], 0  # (symbol of the code-length code, extra bits, count of extra bits)
    while s < top:
        run = 1
        while repeats and s + run < top and lens[s + run] == lens[s]:
            run += 1
        if repeats and lens[s] == 0 and run >= 3:
            run = min(run, 138)
            tokens.append((17, run - 3, 3) if run <= 10 else (18, run - 11, 7))
        elif repeats and run >= 4 and lens[s]:
            run = min(run - 1, 6)
            tokens += [(lens[s], 0, 0), (16, run - 3, 2)]
            run += 1
        else:
            run = 1
            tokens.append((lens[s], 0, 0))
        s += run
    if hack == "repeat_past":
        tokens[-1] = (18, 127, 7)
    if hack == "repeat_first":  # the code begins with symbol 16: the format repeats 8
        assert lens[:6] == [8] * 6
        tokens[:6] = [(16, 3, 2)]
    hist = [0] * 19
    for t, _, _ in tokens:
        hist[t] += 1
    cl = huffman_lengths(hist, 7)
    ncl = max(4, max(i for i, s in enumerate(CODE_LENGTH_ORDER) if cl[s]) + 1)
    bw.put(ncl - 4, 4)
    for i in range(ncl):
        bw.put(cl[CODE_LENGTH_ORDER[i]], 3)
    if max_symbol or hack == "max_symbol_big":
        ms = n + 1 if hack == "max_symbol_big" else max(2, len(tokens))
        assert ms == len(tokens) or hack or len(tokens) < 2
        k = next(k for k in range(8) if ms - 2 < 1 << (2 + 2 * k))
        bw.put(1, 1)
        bw.put(k, 3)
        bw.put(ms - 2, 2 + 2 * k)
    else:
        bw.put(0, 1)
    cw = CodeWriter(cl)
    for t, extra, nbits in tokens:
        cw.put(bw, t)
        bw.put(extra, nbits)


def _prefix_encode(v):
    """value >= 1 -> (prefix symbol, extra bits, their count)"""
    v -= 1
    if v < 4:
        return v, 0, 0
    hb = v.bit_length() - 1
    second = (v >> (hb - 1)) & 1
    extra = hb - 1
    return 2 * hb + second, v & ((1 << extra) - 1), extra


def distance_code(xsize, dist, plane=True):
    if plane:
        for c in range(1, 121):
            if plane_distance(xsize, c) == dist:
                return c
    return dist + 120


def tokenize(px, xsize, cache_bits=0, refs="none", plane=True, min_len=3):
    """pixels -> tokens ('lit', argb) / ('cache', key) / ('ref', length, distance code); refs 'lz' finds repeats greedily"""
    tokens, cache, last, q, n = [], [0] * (1 << cache_bits) if cache_bits else None, {}, 0, len(px)

    def enter(v):
        if cache is not None:
            cache[cache_key(v, cache_bits)] = v

    while q < n:
        best = 0
        if refs == "lz" and q + 1 < n:
            src = last.get((px[q], px[q + 1]))
            if src is not None:
                m = 0
                while q + m < n and m < 4096 and px[src + m] == px[q + m]:
                    m += 1
                best, dist = (m, q - src) if q - src + 120 <= 1 << 20 else (0, 0)  # (the largest distance code)
        if best >= min_len:
            tokens.append(("ref", best, distance_code(xsize, dist, plane)))
            for k in range(best):
                enter(px[q + k])
                if q + k + 1 < n:
                    last[(px[q + k], px[q + k + 1])] = q + k
            q += best
            continue
        v = px[q]
        if cache is not None and cache[cache_key(v, cache_bits)] == v:
            tokens.append(("cache", cache_key(v, cache_bits)))
        else:
            tokens.append(("lit", v))
        enter(v)
        if q + 1 < n:
            last[(v, px[q + 1])] = q
        q += 1
    return tokens


def token_pixels(t):
    return t[1] if t[0] == "ref" else 1


def write_pixels(bw, tokens, xsize, cache_bits=0, ent=None, meta_bits=0, n_groups=1, code_kw=None, hack=None, lens=None, info=None):
    """the codes of every group, then the tokens; an array of ARGB values for tokens stands for that many literals of one group.
    lens: f(group, alphabet 0 .. 4, histogram, the lengths the writer would choose) -> the lengths to use; info: a dict that receives
    bit_start and bit_end, the writer's bit position in front of the first token and behind the last"""
    code_kw = code_kw or {}
    if isinstance(tokens, np.ndarray):
        assert ent is None and n_groups == 1 and not cache_bits and hack is None
        c = [(tokens >> 8) & 255, (tokens >> 16) & 255, tokens & 255, tokens >> 24]
        ws = []
        for k, n in enumerate((280, 256, 256, 256, 40)):
            hist = np.bincount(c[k], minlength=n).tolist() if k < 4 else [1] + [0] * 39
            lens = huffman_lengths(hist)
            write_code(bw, lens, **code_kw)
            ws.append(CodeWriter(lens))
        bw.put_many(np.stack([ws[k].rev[c[k]] for k in range(4)], axis=-1), np.stack([ws[k].len[c[k]] for k in range(4)], axis=-1))
        return
    green_n = 280 + ((1 << cache_bits) if cache_bits else 0)
    hists = [[[0] * n for n in (green_n, 256, 256, 256, 40)] for _ in range(n_groups)]
    bwid, pos, where = sub(xsize, meta_bits), 0, []
    for t in tokens:
        y, x = divmod(pos, xsize)
        g = ent[(y >> meta_bits) * bwid + (x >> meta_bits)] if ent is not None else 0
        where.append(g)
        h = hists[g]
        if t[0] == "lit":
            a, r, gr, b = _ch(t[1])
            h[0][gr] += 1
            h[1][r] += 1
            h[2][b] += 1
            h[3][a] += 1
        elif t[0] == "cache":
            h[0][280 + t[1]] += 1
        else:
            h[0][256 + _prefix_encode(t[1])[0]] += 1
            h[4][_prefix_encode(t[2])[0]] += 1
        pos += token_pixels(t)
    writers = []
    for g in range(n_groups):
        ws = []
        for k, hist in enumerate(hists[g]):
            if not any(hist):
                hist[0] = 1
            ln = huffman_lengths(hist)
            ln = lens(g, k, hist, ln) if lens else ln
            hk = hack if (hack and g == 0 and k == (3 if hack in ("max_symbol_big", "repeat_first") else 0)) else None
            if hk == "repeat_first":
                ln = [8] * 256
            write_code(bw, ln, hack=hk, **code_kw)
            ws.append(CodeWriter(ln))
        writers.append(ws)
    if info is not None:
        info["bit_start"] = 8 * len(bw.out) + bw.n
    for t, g in zip(tokens, where):
        ws = writers[g]
        if t[0] == "lit":
            a, r, gr, b = _ch(t[1])
            ws[0].put(bw, gr)
            ws[1].put(bw, r)
            ws[2].put(bw, b)
            ws[3].put(bw, a)
        elif t[0] == "cache":
            ws[0].put(bw, 280 + t[1])
        else:
            s, e, nb = _prefix_encode(t[1])
            ws[0].put(bw, 256 + s)
            bw.put(e, nb)
            s, e, nb = _prefix_encode(t[2])
            ws[4].put(bw, s)
            bw.put(e, nb)
    if info is not None:
        info["bit_end"] = 8 * len(bw.out) + bw.n


def write_sub_image(bw, px, xsize):
    bw.put(0, 1)  # no colour cache
    write_pixels(bw, np.asarray(px, np.uint32).ravel(), xsize)


def _channels(a):
    return np.stack([a >> 24, (a >> 16) & 255, (a >> 8) & 255, a & 255], axis=-1).astype(np.int64)


def _unchannels(c):
    c = c.astype(np.uint32) & 255
    return (c[..., 0] << 24) | (c[..., 1] << 16) | (c[..., 2] << 8) | c[..., 3]


def forward_predictor(a, bits, modes):
    """a: (h, w) uint32; modes: (bh, bw) ints 0 .. 15 (14 and 15 predict as 0) -> residuals"""
    h, w = a.shape
    c = _channels(a)
    flat = c.reshape(-1, 4)
    idx = np.arange(h * w).reshape(h, w)
    L, T, TL, TR = (flat[np.clip(idx - d, 0, None)] for d in (1, w, w + 1, w - 1))
    avg = lambda p, q: (p + q) >> 1
    half_a = avg(L, T)
    d = half_a - TL
    sel = (np.abs(T - TL).sum(-1) < np.abs(L - TL).sum(-1))[..., None]
    black = np.zeros_like(L)
    black[..., 0] = 255
    preds = [black, L, T, TR, TL, avg(avg(L, TR), T), avg(L, TL), avg(L, T), avg(TL, T), avg(T, TR), avg(avg(L, TL), avg(T, TR)), np.where(sel, L, T),
             np.clip(L + T - TL, 0, 255), np.clip(half_a + np.sign(d) * (np.abs(d) // 2), 0, 255), black, black]
    mode_px = np.kron(modes, np.ones((1 << bits, 1 << bits), np.int64))[:h, :w]
    mode_px = mode_px.copy()
    mode_px[:, 0] = 2
    mode_px[0, :] = 1
    mode_px[0, 0] = 0
    pred = np.zeros_like(c)
    for m in range(16):
        pred = np.where((mode_px == m)[..., None], preds[m], pred)
    return _unchannels(c - pred)


def forward_cross(a, bits, coeffs):
    """coeffs: (bh, bw, 3) signed green_to_red, green_to_blue, red_to_blue"""
    h, w = a.shape
    c = _channels(a)
    k = np.kron(coeffs, np.ones((1 << bits, 1 << bits, 1), np.int64))[:h, :w]
    s8 = lambda v: np.where(v & 128, (v & 255) - 256, v & 255)
    r, g, b = c[..., 1], c[..., 2], c[..., 3]
    nb = b - ((k[..., 1] * s8(g)) >> 5) - ((k[..., 2] * s8(r)) >> 5)
    nr = r - ((k[..., 0] * s8(g)) >> 5)
    out = c.copy()
    out[..., 1], out[..., 3] = nr, nb
    return _unchannels(out)


def riff(chunks):
    body = b"WEBP" + b"".join(tag + struct.pack("<I", len(d)) + d + b"\0" * (len(d) & 1) for tag, d in chunks)
    return b"RIFF" + struct.pack("<I", len(body)) + body


def container(chunk, w, h, form="simple", vp8x_alpha=False, extra=True):
    if form == "simple":
        return riff([(b"VP8L", chunk)])
    flags = (0x10 if vp8x_alpha else 0) | (0x08 if extra else 0)
    x = bytes([flags, 0, 0, 0]) + (w - 1).to_bytes(3, "little") + (h - 1).to_bytes(3, "little")
    chunks = [(b"VP8X", x)] + ([(b"unkn", b"abc")] if extra else []) + [(b"VP8L", chunk)] + ([(b"EXIF", b"Exif\0\0II*\0\x08\0\0\0\0\0")] if extra else [])
    return riff(chunks)


def to_argb(img):
    img = np.asarray(img, np.uint32)
    a = img[..., 3] if img.shape[-1] == 4 else np.full(img.shape[:2], 255, np.uint32)
    return (a << 24) | (img[..., 0] << 16) | (img[..., 1] << 8) | img[..., 2]


def encode(img, transforms=(), cache_bits=0, meta_bits=None, n_groups=1, refs="none", plane=True, form="simple", alpha=None, vp8x_alpha=None, code_kw=None,
           tokens=None, hack=None, cache_bits_raw=None, trailing=b"", seed=0, ent_map=None, lens=None, info=None):
    """img: (h, w, 3 or 4) uint8.  transforms, in the order written: ('predictor', bits 2 .. 9, mode 0 .. 15 | 'mixed' (modes 0 .. 13) |
    'mixed16' (0 .. 15) | an array of modes per block), ('cross', bits 2 .. 9[, an array (bh, bw, 3) of signed coefficients]), ('green',),
    ('palette'[, declared colours[, the palette as ARGB values]]).  tokens: the main stream's tokens as given (the pixels then are what they decode to).  ent_map: the group of every
    block of the entropy image, in place of the writer's own pattern.  lens, info: as write_pixels takes them."""
    rng = np.random.default_rng(seed)
    a = to_argb(img)
    h, w = a.shape
    alpha = (np.asarray(img).shape[-1] == 4) if alpha is None else alpha
    bw = BitWriter()
    bw.put(0x2f, 8)
    bw.put(w - 1, 14)
    bw.put(h - 1, 14)
    bw.put(int(alpha), 1)
    bw.put(0 if hack != "version" else 1, 3)
    for tr in transforms:
        bw.put(1, 1)
        hh, ww = a.shape
        if tr[0] == "predictor":
            bits = tr[1]
            shape = (sub(hh, bits), sub(ww, bits))
            modes = tr[2]
            if isinstance(modes, str):
                modes = rng.integers(0, 14 if modes == "mixed" else 16, shape)
            modes = np.broadcast_to(np.asarray(modes, np.int64), shape)
            bw.put(0, 2)
            bw.put(bits - 2, 3)
            write_sub_image(bw, (0xff000000 | (modes.astype(np.uint32) << 8)).ravel(), shape[1])
            a = forward_predictor(a, bits, modes)
        elif tr[0] == "cross":
            bits = tr[1]
            shape = (sub(hh, bits), sub(ww, bits))
            k = np.broadcast_to(np.asarray(tr[2], np.int64), shape + (3,)) if len(tr) > 2 else rng.integers(-40, 40, shape + (3,))
            bw.put(1, 2)
            bw.put(bits - 2, 3)
            write_sub_image(bw, (0xff000000 | ((k[..., 2] & 255) << 16) | ((k[..., 1] & 255) << 8) | (k[..., 0] & 255)).astype(np.uint32).ravel(), shape[1])
            a = forward_cross(a, bits, k)
        elif tr[0] == "green":
            bw.put(2, 2)
            c = _channels(a)
            c[..., 1] -= c[..., 2]
            c[..., 3] -= c[..., 2]
            a = _unchannels(c)
        else:
            if len(tr) > 2:  # (the palette as given: its size does not depend on the colours in use)
                pal = np.asarray(tr[2], np.uint32)
                index = (a[..., None] == pal).argmax(-1)
                assert np.array_equal(pal[index], a)
            else:
                pal, index = np.unique(a, return_inverse=True)
                index = index.reshape(a.shape)
            n = len(pal) if len(tr) < 2 else tr[1]  # (a declared count below the colours in use: indexes past the palette)
            assert len(pal) <= 256
            bits = 0 if n > 16 else 1 if n > 4 else 2 if n > 2 else 3
            bw.put(3, 2)
            bw.put(n - 1, 8)
            pc = _channels(pal[:n].astype(np.uint32))
            pc[1:] -= pc[:-1].copy()
            write_sub_image(bw, _unchannels(pc), n)
            ppb, bpp = 1 << bits, 8 >> bits
            padded = np.zeros((hh, sub(ww, bits) * ppb), np.uint32)
            padded[:, :ww] = index
            packed = sum(padded[:, k::ppb] << (k * bpp) for k in range(ppb))
            a = (0xff000000 | (packed << 8)).astype(np.uint32)
    bw.put(0, 1)
    xsize = a.shape[1]
    if cache_bits_raw is not None:
        bw.put(1, 1)
        bw.put(cache_bits_raw, 4)
    elif cache_bits:
        bw.put(1, 1)
        bw.put(cache_bits, 4)
    else:
        bw.put(0, 1)
    px = [int(v) for v in a.ravel()]
    ent = None
    if meta_bits is not None:
        shape = (sub(h, meta_bits), sub(xsize, meta_bits))
        if ent_map is None:
            ent = [int(v) for v in (np.arange(shape[0] * shape[1]) * 7 % n_groups)]
            ent[-1] = n_groups - 1
        else:
            ent = [int(v) for v in np.asarray(ent_map).ravel()]
            assert len(ent) == shape[0] * shape[1] and max(ent) == n_groups - 1
        bw.put(1, 1)
        bw.put(meta_bits - 2, 3)
        write_sub_image(bw, [0xff000000 | (g << 8) for g in ent], shape[1])
        if hack == "cut_after_entropy_image":
            return container(bw.bytes(), w, h, form, bool(alpha))
    else:
        bw.put(0, 1)
    if tokens is None:
        plain = refs == "none" and not cache_bits and ent is None and hack is None
        tokens = a.ravel().astype(np.uint32) if plain else tokenize(px, xsize, cache_bits, refs, plane)
    write_pixels(bw, tokens, xsize, cache_bits, ent, meta_bits or 0, n_groups, code_kw, hack if hack in ("over", "incomplete", "repeat_past", "max_symbol_big", "repeat_first") else None,
                 lens, info)
    chunk = bw.bytes() + trailing
    if hack == "signature":
        chunk = b"\x2e" + chunk[1:]
    return container(chunk, w, h, form, bool(alpha) if vp8x_alpha is None else vp8x_alpha)


# ------------------------------------------------------------------ content and corpora
def photo(rng, w, h, alpha=False):
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(xx * 3 + yy * 2 + 40 * c) % 256 for c in range(4 if alpha else 3)], axis=-1)
    return ((base + rng.integers(0, 24, base.shape)) % 256).astype(np.uint8)


def flat(rng, w, h, colours, alpha=False):
    pal = rng.integers(0, 256, (colours, 4 if alpha else 3))
    yy, xx = np.mgrid[0:h, 0:w]
    idx = ((xx // 3 + yy // 2) % colours)
    idx[rng.integers(0, h, 1 + h // 4), rng.integers(0, w, 1 + h // 4)] = rng.integers(0, colours, 1 + h // 4)
    idx.flat[:colours] = np.arange(colours) if colours <= w * h else 0
    return pal[idx].astype(np.uint8)


def short_distance_file(rng, code):
    """a 24 x 20 image whose stream uses distance code `code` (1 .. 120) for a copy in its last rows"""
    w, h = 24, 20
    head = [("lit", int(v)) for v in to_argb(photo(rng, w, 9)).ravel()]
    head += [("lit", int(v)) for v in to_argb(photo(rng, 10, 1)).ravel()]
    body = [("ref", 5, code)]
    rest = w * h - len(head) - 5
    return encode(np.zeros((h, w, 3), np.uint8), tokens=head + body + [("lit", 0xff102030 + k) for k in range(rest)])


_VALID = {}


def valid_corpus(stride=1):
    """(name, file) of every feature the writer can force; stride n keeps every n-th"""
    if not _VALID:
        rng = np.random.default_rng(11)
        out = []
        add = lambda name, data: out.append((name, data))
        for m in range(14):
            add(f"predictor_mode_{m}", encode(photo(rng, 23, 19, alpha=m % 2 == 1), [("predictor", 2 + m % 3, m)], seed=m))
        add("predictor_mixed", encode(photo(rng, 70, 67), [("predictor", 2, "mixed")], seed=1))
        add("predictor_mixed_wide", encode(photo(rng, 150, 9, alpha=True), [("predictor", 3, "mixed")], seed=2))
        add("predictor_tall", encode(photo(rng, 3, 140), [("predictor", 2, "mixed")], seed=3))
        add("cross_colour", encode(photo(rng, 33, 21), [("cross", 3)], seed=4))
        add("subtract_green", encode(photo(rng, 33, 21, alpha=True), [("green",)]))
        for colours in (2, 4, 16, 17, 256):
            add(f"palette_{colours}", encode(flat(rng, 37, 29, colours, alpha=colours == 4), [("palette",)], refs="lz" if colours > 4 else "none"))
        add("palette_index_past_end", encode(flat(rng, 21, 9, 12), [("palette", 9)]))
        add("three_transforms_cache_lz", encode(photo(rng, 45, 38, alpha=True), [("green",), ("predictor", 3, "mixed"), ("cross", 2)], cache_bits=4, refs="lz", seed=5))
        add("palette_then_predictor", encode(flat(rng, 45, 38, 5), [("palette",), ("predictor", 2, "mixed")], seed=6))
        add("four_transforms_with_palette", encode(flat(rng, 41, 30, 40), [("palette",), ("green",), ("predictor", 2, "mixed"), ("cross", 2)], seed=7))
        for cb in (1, 6, 11):
            add(f"cache_{cb}", encode(flat(rng, 40, 33, 30), cache_bits=cb, refs="lz" if cb == 6 else "none"))
        add("cache_none_lz", encode(flat(rng, 40, 33, 30), refs="lz"))
        for g, mb, wh in ((1, 3, (30, 20)), (2, 2, (30, 20)), (300, 2, (96, 80))):
            add(f"groups_{g}", encode(photo(rng, *wh) if g < 300 else flat(rng, *wh, 6), meta_bits=mb, n_groups=g, refs="lz", cache_bits=3 if g == 2 else 0))
        one = np.zeros((8, 9, 3), np.uint8) + np.array([9, 200, 31], np.uint8)
        add("simple_codes_one_symbol", encode(one))
        two = one.copy()
        two[::2, ::3] = (9, 100, 31)
        add("simple_codes_two_symbols", encode(two))
        add("normal_codes_only", encode(two, code_kw=dict(simple=False)))
        add("max_symbol", encode(photo(rng, 20, 16) // 4, code_kw=dict(max_symbol=True)))
        add("code_length_repeats", encode(photo(rng, 20, 16) // 2, code_kw=dict(repeats=True)))
        for code in range(1, 121):
            add(f"distance_code_{code}", short_distance_file(rng, code))
        add("long_distances", encode(np.tile(photo(rng, 50, 7), (6, 1, 1)), refs="lz", plane=False))
        run = np.zeros((12, 40, 3), np.uint8) + 77
        run[:, 20:] = np.tile(photo(rng, 5, 1), (12, 4, 1))
        add("overlap_distance_1_and_below_64", encode(run, refs="lz"))
        add("copy_ends_on_last_pixel", encode(np.tile(photo(rng, 31, 1), (9, 1, 1)), refs="lz"))
        for w, h in ((1, 1), (4, 4), (5, 5), (16384, 1), (1, 16384)):
            add(f"size_{w}x{h}", encode(flat(rng, w, h, 3) if w * h > 100 else photo(rng, w, h), [("predictor", 4, "mixed")] if w * h > 100 else [], refs="lz", seed=8))
        img = photo(rng, 26, 17, alpha=True)
        add("vp8x_container", encode(img, [("predictor", 2, 11)], form="vp8x"))
        add("vp8x_flag_without_header_bit", encode(img, form="vp8x", alpha=False, vp8x_alpha=True))
        add("header_bit_without_vp8x_flag", encode(img, form="vp8x", alpha=True, vp8x_alpha=False))
        add("alpha_pixels_without_header_bit", encode(img, alpha=False))
        add("trailing_bytes_in_chunk", encode(img, trailing=b"\x55" * 7))
        d = encode(img)
        add("bytes_after_riff", d + b"junkjunk")
        _VALID["all"] = out
    return _VALID["all"][::stride]


def _resize_chunk(data, keep):
    """the simple-form file with its VP8L payload cut to `keep` bytes"""
    chunk = data[20:20 + struct.unpack_from("<I", data, 16)[0]][:keep]
    return riff([(b"VP8L", chunk)])


def rule_corpus():
    """(name, file, status): one file per line of the rule"""
    rng = np.random.default_rng(13)
    img = photo(rng, 19, 14)
    good = encode(img, [("predictor", 2, "mixed")], refs="lz")
    w = 19
    lits = lambda n: [("lit", 0xff000000 + 977 * k) for k in range(n)]
    x = container(good[20:], 19, 14, "vp8x")
    out = [
        ("good", good, 0),
        ("bad_riff_tag", b"RIFX" + good[4:], INVALID),
        ("bad_webp_tag", good[:8] + b"WEBQ" + good[12:], INVALID),
        ("riff_size_past_file", good[:4] + struct.pack("<I", len(good)) + good[8:], INVALID),
        ("riff_size_short_of_image", good[:4] + struct.pack("<I", len(good) - 12) + good[8:], INVALID),
        ("riff_size_below_file", good + b"tail", 0),
        ("chunk_past_file", riff([(b"VP8X", bytes([0, 0, 0, 0, 18, 0, 0, 13, 0, 0]))])[:4] + struct.pack("<I", 4 + 18 + 12) + b"WEBP" + b"VP8X" + struct.pack("<I", 10)
         + bytes([0, 0, 0, 0, 18, 0, 0, 13, 0, 0]) + b"EXIF" + struct.pack("<I", 1000) + b"1234", INVALID),
        ("missing_image_chunk", riff([(b"VP8X", bytes([0, 0, 0, 0, 18, 0, 0, 13, 0, 0])), (b"EXIF", b"1234")]), INVALID),
        ("empty_riff", riff([]), INVALID),
        ("canvas_mismatch", container(good[20:], 20, 14, "vp8x"), INVALID),
        ("chunks_after_image", x, 0),
        ("signature", encode(img, hack="signature"), INVALID),
        ("version", encode(img, hack="version"), INVALID),
        ("transform_twice", encode(img, [("green",), ("green",)]), INVALID),
        ("cache_size_0", encode(img, cache_bits_raw=0), INVALID),
        ("cache_size_12", encode(img, cache_bits_raw=12), INVALID),
        ("over_subscribed_code", encode(img, hack="over"), INVALID),
        ("incomplete_code", encode(img, hack="incomplete"), INVALID),
        ("repeat_past_alphabet", encode(img, hack="repeat_past", code_kw=dict(repeats=True)), INVALID),
        ("repeat_with_nothing_before_it", encode(img, hack="repeat_first", code_kw=dict(simple=False)), 0),
        ("tables_above_64_mib", encode(np.zeros((360, 360, 3), np.uint8), cache_bits=11, meta_bits=2, n_groups=7464, hack="cut_after_entropy_image"), UNSUPPORTED),
        ("tables_just_below_64_mib", encode(np.zeros((360, 360, 3), np.uint8), cache_bits=11, meta_bits=2, n_groups=7463, hack="cut_after_entropy_image"), INVALID),
        ("max_symbol_above_alphabet", encode(img, hack="max_symbol_big", code_kw=dict(simple=False)), INVALID),
        ("distance_before_first_pixel", encode(img, tokens=lits(3) + [("ref", 4, 120 + 4)] + lits(19 * 14 - 7)), INVALID),
        ("distance_to_first_pixel", encode(img, tokens=lits(3) + [("ref", 4, 120 + 3)] + lits(19 * 14 - 7)), 0),
        ("copy_past_last_pixel", encode(img, tokens=lits(19 * 14 - 5) + [("ref", 6, 120 + 2)]), INVALID),
        ("copy_to_last_pixel", encode(img, tokens=lits(19 * 14 - 5) + [("ref", 5, 120 + 2)]), 0),
        ("out_of_bits", _resize_chunk(good, (len(good) - 20) * 2 // 3), INVALID),
        ("out_of_bits_in_front", _resize_chunk(good, 9), INVALID),
        ("header_only", _resize_chunk(good, 5), INVALID),
        ("short_header", _resize_chunk(good, 4), INVALID),
        ("animated_flag", riff([(b"VP8X", bytes([2, 0, 0, 0, 18, 0, 0, 13, 0, 0])), (b"VP8L", good[20:])]), UNSUPPORTED),
        ("anmf_chunk", riff([(b"VP8X", bytes([0, 0, 0, 0, 18, 0, 0, 13, 0, 0])), (b"ANMF", bytes(16)), (b"VP8L", good[20:])]), UNSUPPORTED),
        ("lossy_chunk", riff([(b"VP8 ", bytes(30))]), UNSUPPORTED),
        ("alph_chunk", riff([(b"VP8X", bytes([16, 0, 0, 0, 18, 0, 0, 13, 0, 0])), (b"ALPH", bytes(8)), (b"VP8 ", bytes(30))]), UNSUPPORTED),
    ]
    assert w == 19
    return out


def damaged_corpus(seed=1, n_random=200):
    """the rule's files (without their statuses) and random damage to valid ones: bytes overwritten, bits flipped, cuts, insertions"""
    rng = np.random.default_rng(seed)
    out = [(n, d) for n, d, _ in rule_corpus()]
    pool = [d for n, d in valid_corpus() if len(d) < 3000 and not n.startswith("distance_code")]
    for k in range(n_random):
        g = bytearray(pool[int(rng.integers(0, len(pool)))])
        kind = int(rng.integers(0, 4))
        if kind == 0:
            for _ in range(int(rng.integers(1, 5))):
                g[int(rng.integers(0, len(g)))] = int(rng.integers(0, 256))
        elif kind == 1:
            for _ in range(int(rng.integers(1, 4))):
                g[int(rng.integers(20, len(g)))] ^= 1 << int(rng.integers(0, 8))
        elif kind == 2:
            g = bytearray(riff([(b"VP8L", bytes(g[20:int(rng.integers(21, len(g)))]))]))
        else:
            g.insert(int(rng.integers(20, len(g))), int(rng.integers(0, 256)))
            g[4:8] = struct.pack("<I", len(g) - 8)
        out.append((f"random_{k}_{kind}", bytes(g)))
    return out
