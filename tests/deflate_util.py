"""A deflate *writer* for tests, built on numpy and the standard library: an LSB-first bit writer, canonical and length-limited Huffman
codes, stored / fixed / dynamic block writers that take explicit tokens, code lengths and code-length sequences, `expand` (the plain
byte-by-byte statement of what a token list decodes to), a zlib wrapper, a PNG and a TIFF carrier, and three corpora: named_streams()
(one or more streams per corner of inflate.h and of the device sink of png_kernels.hip that zlib's own encoder never writes),
random_streams() (seeded, valid by construction) and refused_streams() (invalid twins of named cases, one bit of structure apart).
zlib's decoder is the reference for acceptance: every stream announces a 32 KiB window (CINFO 7), where its distance check and the
project's agree.  Not a test module."""
import functools
import struct
import zlib

import numpy as np

import png_util as pu
import tiff_util as tu

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [k for k in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
WINDOW = 32768
EDGE_LENS = (3, 63, 64, 65, 66, 128, 129, 257, 258)
EDGE_DISTS = tuple(range(1, 67)) + (127, 128, 129)


# ---------------------------------------------------------------- bits and codes

class BitWriter:
    """deflate's bit order: fields least significant bit first, Huffman codes most significant bit first"""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, k):
        assert 0 <= v < (1 << k) or k == 0
        self.acc |= v << self.n
        self.n += k
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c):
        code, k = c
        self.put(int(format(code, f"0{k}b")[::-1], 2), k)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def raw(self, data):
        assert self.n == 0
        self.out += data


def canonical(lens):
    """{symbol: (code, length)} of the canonical Huffman code of RFC 1951 3.2.2 (an incomplete set of lengths gets its first codes)"""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def kraft(lens, limit=15):
    """code space used, in units of 2^-limit (a complete code: 2^limit)"""
    return sum(1 << (limit - l) for l in lens if l)


def _split_to(depths, m, limit, rng):
    """split leaves shallower than `limit` until there are m of them"""
    depths = list(depths)
    if len(depths) > m:
        raise ValueError("more free code space than symbols")
    while len(depths) < m:
        open_ = [i for i, d in enumerate(depths) if d < limit]
        if not open_:
            raise ValueError("more symbols than code space")
        i = open_[int(rng.integers(0, len(open_)))] if rng is not None else min(open_, key=lambda j: depths[j])
        depths[i] += 1
        depths.append(depths[i])
    return sorted(depths)


def fill_code(n, fixed, others, limit=15, rng=None):
    """Lengths for n symbols: `fixed` {symbol: length} as given, and the symbols of `others` (in order: the first get the shortest)
    share all the code space that is left, so that the code is complete"""
    lens = [0] * n
    for s, l in fixed.items():
        lens[s] = l
    free = (1 << limit) - kraft(lens, limit)
    assert free >= 0
    nodes = [d for d in range(0, limit + 1) if (free >> (limit - d)) & 1]
    for s, d in zip(others, _split_to(nodes, len(others), limit, rng)):
        lens[s] = d
    assert kraft(lens, limit) == 1 << limit
    return lens


def limited_code(freqs, max_len=None, limit=15, rng=None):
    """A length-limited prefix code for the symbols with a non-zero frequency: complete, no length above `limit`, frequent symbols
    short.  max_len forces the longest length (brought into the range the number of symbols allows: m symbols reach depths
    ceil(log2 m) ... m - 1).  One symbol gets the single code of length 1 (incomplete); none gives all zeros."""
    used = sorted((s for s, f in enumerate(freqs) if f), key=lambda s: -freqs[s])
    lens = [0] * len(freqs)
    m = len(used)
    if m == 0:
        return lens
    if m == 1:
        lens[used[0]] = 1
        return lens
    lo = max(1, (m - 1).bit_length())
    d = min(max(max_len if max_len is not None else lo + 1, lo), min(limit, m - 1))
    chain = list(range(1, d)) + [d, d]  # the deepest shape: one leaf per depth and two at the bottom
    for s, l in zip(used, _split_to(chain, m, d, rng)):
        lens[s] = l
    assert kraft(lens, limit) == 1 << limit and max(lens) == d
    return lens


# ---------------------------------------------------------------- tokens

def length_symbol(length, sym=None):
    """(symbol - 257, extra value, extra bits); sym = 284 spells 258 as 227 + 31"""
    if sym is None:
        s = max(k for k in range(29) if LEN_BASE[k] <= length)
    else:
        s = sym - 257
    extra = length - LEN_BASE[s]
    assert 0 <= extra < (1 << LEN_EXTRA[s]) or (extra == 0 and LEN_EXTRA[s] == 0), (length, sym)
    return s, extra, LEN_EXTRA[s]


def distance_symbol(dist):
    assert 1 <= dist <= WINDOW
    s = max(k for k in range(30) if DIST_BASE[k] <= dist)
    return s, dist - DIST_BASE[s], DIST_EXTRA[s]


def _emit_tokens(w, tokens, lit, dist):
    """A token is a literal byte, (length, distance[, length symbol]), or an escape for streams that must be refused:
    ("sym", literal/length symbol), ("dsym", distance symbol) or ("bits", value, count)"""
    for t in tokens:
        if isinstance(t, tuple) and isinstance(t[0], str):
            if t[0] == "sym":
                w.code(lit[t[1]])
            elif t[0] == "dsym":
                w.code(dist[t[1]])
            else:
                w.put(t[1], t[2])
        elif isinstance(t, tuple):
            s, ev, eb = length_symbol(t[0], t[2] if len(t) > 2 else None)
            w.code(lit[257 + s])
            w.put(ev, eb)
            d, dv, db = distance_symbol(t[1])
            w.code(dist[d])
            w.put(dv, db)
        else:
            w.code(lit[t])


def expand(tokens, history=b""):
    """What the tokens decode to after `history`: the byte-by-byte forward copy of RFC 1951 (escapes produce nothing)"""
    out = bytearray(history)
    for t in tokens:
        if isinstance(t, tuple):
            if isinstance(t[0], str):
                continue
            length, dist = t[0], t[1]
            assert 1 <= dist <= len(out) and dist <= WINDOW
            for _ in range(length):
                out.append(out[-dist])
        else:
            out.append(t)
    return bytes(out[len(history):])


def token_freqs(tokens):
    lf, df = [0] * 286, [0] * 30
    lf[256] = 1
    for t in tokens:
        if isinstance(t, tuple):
            if isinstance(t[0], str):
                continue
            lf[257 + length_symbol(t[0], t[2] if len(t) > 2 else None)[0]] += 1
            df[distance_symbol(t[1])[0]] += 1
        else:
            lf[t] += 1
    return lf, df


# ---------------------------------------------------------------- blocks: each is a function of the bit writer

def stored(data, final=False):
    data = bytes(data)
    assert len(data) <= 65535

    def emit(w):
        w.put(int(final), 1)
        w.put(0, 2)
        w.align()
        w.raw(struct.pack("<HH", len(data), ~len(data) & 0xFFFF) + data)
    return emit


def fixed(tokens, final=False, eob=True):
    lit, dist = canonical(FIXED_LIT), canonical(FIXED_DIST)

    def emit(w):
        w.put(int(final), 1)
        w.put(1, 2)
        _emit_tokens(w, tokens, lit, dist)
        if eob:
            w.code(lit[256])
    return emit


def cl_rle(lens, rng=None):
    """The code-length sequence of `lens`: ints 0-15, (16, n) = the previous length n = 3-6 times more, (17, n) = 3-10 zeros,
    (18, n) = 11-138 zeros.  Greedy without rng; with one, runs are cut at random places and some are spelled out."""
    seq, i = [], 0
    while i < len(lens):
        v, run = lens[i], 1
        while i + run < len(lens) and lens[i + run] == v:
            run += 1
        if rng is not None and rng.random() < 0.3:
            run = int(rng.integers(1, run + 1))
        if v == 0 and run >= 3:
            n = min(run, 138)
            if rng is not None and rng.random() < 0.5:
                n = int(rng.integers(3, n + 1))
            seq.append((18, n) if n >= 11 else (17, n))
            i += n
        elif v and run >= 4:
            seq.append(v)
            n = min(run - 1, 6)
            if rng is not None and rng.random() < 0.5:
                n = int(rng.integers(3, n + 1))
            seq.append((16, n))
            i += 1 + n
        else:
            seq.append(v)
            i += 1
    return seq


def cl_expand(seq):
    out = []
    for it in seq:
        if isinstance(it, tuple):
            out += [out[-1] if it[0] == 16 else 0] * it[1]
        else:
            out.append(it)
    return out


def dynamic(tokens, lit_lens, dist_lens, final=False, cl_sequence=None, hclen=None, cl_lens=None, eob=True, check=True):
    """lit_lens: 257-286 literal/length code lengths, dist_lens: 1-30 distance code lengths (HLIT and HDIST follow from the counts).
    cl_sequence: the code-length symbols to write (see cl_rle; default: the greedy one), cl_lens: the 19 lengths of the code-length
    code (default: a length-limited code of the sequence's symbols), hclen: how many of them the header carries (default: up to the
    last non-zero one).  check=False lets a stream that must be refused break the rules."""
    lit_lens, dist_lens = list(lit_lens), list(dist_lens)
    seq = cl_sequence if cl_sequence is not None else cl_rle(lit_lens + dist_lens)
    if cl_lens is None:
        f = [0] * 19
        for it in seq:
            f[it[0] if isinstance(it, tuple) else it] += 1
        if sum(1 for x in f if x) < 2:  # (the code-length code must be complete: two codes at the least)
            f[[s for s in (0, 1) if not f[s]][0]] += 1
        cl_lens = limited_code(f, limit=7)
    need = max(k for k in range(19) if cl_lens[CL_ORDER[k]]) + 1
    hclen = max(4, need) if hclen is None else hclen
    if check:
        assert 257 <= len(lit_lens) <= 286 and 1 <= len(dist_lens) <= 30 and 4 <= need <= hclen <= 19
        assert cl_expand(seq) == lit_lens + dist_lens and lit_lens[256]
    lit, dist, cl = canonical(lit_lens), canonical(dist_lens), canonical(cl_lens)

    def emit(w):
        w.put(int(final), 1)
        w.put(2, 2)
        w.put(len(lit_lens) - 257, 5)
        w.put(len(dist_lens) - 1, 5)
        w.put(hclen - 4, 4)
        for k in range(hclen):
            w.put(cl_lens[CL_ORDER[k]], 3)
        for it in seq:
            if isinstance(it, tuple):
                w.code(cl[it[0]])
                w.put(it[1] - (11 if it[0] == 18 else 3), {16: 2, 17: 3, 18: 7}[it[0]])
            else:
                w.code(cl[it])
        _emit_tokens(w, tokens, lit, dist)
        if eob:
            w.code(lit[256])
    return emit


def dynamic_auto(tokens, final=False, max_len=None, dist_max_len=None, nlen=None, ndist=None, rng=None, extra_lit=(), extra_dist=(), **kw):
    """A dynamic block whose codes are built from the tokens' own frequencies (extra_lit / extra_dist: symbols that get a code
    although no token uses them, which a deep code needs when the tokens use few symbols)"""
    lf, df = token_freqs(tokens)
    for s in extra_lit:
        lf[s] += 1
    for s in extra_dist:
        df[s] += 1
    nlen = nlen or max(257, max(s for s in range(286) if lf[s]) + 1)
    ndist = ndist or max([1] + [s + 1 for s in range(30) if df[s]])
    lit_lens = limited_code(lf[:nlen], max_len, rng=rng)
    dist_lens = limited_code(df[:ndist], dist_max_len, rng=rng)
    return dynamic(tokens, lit_lens, dist_lens, final, **kw)


def zlib_stream(blocks, raw, adler=None):
    """78 01 (CINFO 7, no dictionary), the blocks, the Adler-32 of raw"""
    w = BitWriter()
    for b in blocks:
        b(w)
    w.align()
    a = zlib.adler32(bytes(raw)) & 0xFFFFFFFF if adler is None else adler
    return b"\x78\x01" + bytes(w.out) + struct.pack(">I", a)


# ---------------------------------------------------------------- carriers

def png_carrier(z, cap):
    """A PNG of colour type 0, depth 8, height 1 whose raw bytes (filter byte 0 + the row) are the first `cap` bytes the stream
    decodes to; what follows them inside the stream is accepted by the PNG rule.  Expected pixels: raw[1:cap]."""
    assert cap >= 2
    ihdr = struct.pack(">IIBBBBB", cap - 1, 1, 8, 0, 0, 0, 0)
    return pu.SIG + pu.chunk(b"IHDR", ihdr) + pu.chunk(b"IDAT", z) + pu.chunk(b"IEND", b"")


def filler(n, seed):
    """(zlib stream, bytes): n bytes in stored blocks, the last three as a fixed block when there is room"""
    data = bytes(np.random.default_rng(seed).integers(0, 256, n).astype(np.uint8))
    head = data[:-3] if n > 3 else b""
    blocks = [stored(head[i:i + 65535]) for i in range(0, len(head), 65535)] + [fixed(list(data[len(head):]), True)]
    return zlib_stream(blocks, data), data


def tiff_carrier(z, cap, seed=0):
    """(file, expected bytes): an 8-bit gray TIFF one pixel wide, Compression 8, three strips of one zlib stream each: `cap` bytes of
    filler, the stream under test (its first `cap` bytes; it lands at offset `cap`, whatever that is a multiple of), and a short
    strip of 1-37 bytes.  Streams of one call therefore differ in where their bytes go and in how many they keep."""
    assert cap >= 1
    tail = 1 + (seed * 7 + cap) % min(cap, 37)
    z0, d0 = filler(cap, seed)
    z2, d2 = filler(tail, seed + 1)
    h = 2 * cap + tail
    return tu.write(tu.base_tags(1, h, 1, 8, 1, 8, 1, cap), [z0, z, z2]), (d0, d2)


def tiff_expected(raw, cap, fill):
    return fill[0] + bytes(raw[:cap]) + fill[1]


# ---------------------------------------------------------------- named streams

def _bytes(n, seed):
    """n bytes with no period (so that a copy from the wrong place shows), the first one 0: a PNG row's filter byte"""
    b = bytearray(np.random.default_rng(1000 + seed).integers(0, 256, n).astype(np.uint8))
    if n:
        b[0] = 0
    return bytes(b)


def _stored_run(data):
    return [stored(data[i:i + 65535]) for i in range(0, len(data), 65535)]


class _Corpus:
    def __init__(self):
        self.items = []

    def add(self, name, blocks, raw, cap=None):
        raw = bytes(raw)
        assert len(raw) >= 2 and raw[0] == 0 and len(raw) <= 200_000, name
        assert all(n != name for n, _, _, _ in self.items), name
        self.items.append((name, zlib_stream(blocks, raw), raw, cap if cap is not None else len(raw)))

    def tokens(self, name, prefix, tokens, kind, cap=None, suffix=b"", **kw):
        """stored prefix, the tokens as one block of `kind`, literal suffix in a final fixed block"""
        body = expand(tokens, prefix)
        blk = fixed(tokens) if kind == "fixed" else dynamic_auto(tokens, **kw)
        self.add(name, _stored_run(prefix) + [blk, fixed(list(suffix), True)], prefix + body + suffix, cap)


def _copy_cases(c):
    # the grid: every distance of the edge set with every length of it, one stream per distance
    for k, dist in enumerate(EDGE_DISTS):
        prefix = _bytes(max(dist, 2) + k % 5, k)
        tokens = []
        for j, length in enumerate(EDGE_LENS):
            tokens += [(length, dist)] + list(_bytes(3 + j, 7 * k + j)[1:])
        c.tokens(f"copy_dist{dist}", prefix, tokens, "fixed" if k & 1 else "dynamic", suffix=_bytes(5, k)[1:])
    # the ring: copies that start at each phase before the wrap, at it and after it; distance 32768 where source slot = target slot
    for k, back in enumerate((258, 257, 129, 65, 64, 63, 2, 1, 0)):
        for dist in (1, 3, 65, 300, 4097, 32768 - back if back else 32768):
            n0 = WINDOW - back
            if dist > n0:
                continue
            tokens = [(258, dist), 7, (66, dist), 9, (3, 1)]
            c.tokens(f"ring_start{n0}_dist{dist}", _bytes(n0, 50 + k), tokens, "dynamic" if k & 1 else "fixed", suffix=b"\x01\x02")
    for n0 in (WINDOW, WINDOW + 1, WINDOW + 63, 40000, 2 * WINDOW - 100, 2 * WINDOW):
        tokens = [(258, WINDOW), 5, (258, WINDOW), (257, WINDOW - 1), 6, (64, WINDOW)]
        c.tokens(f"dist32768_at{n0}", _bytes(n0, 70 + n0 % 13), tokens, "fixed", suffix=b"\x03")
    c.tokens("dist32768_after_40000_literals", b"", list(_bytes(40000, 77)) + [(258, WINDOW), (3, WINDOW)], "dynamic")
    # the 4 KiB flush: copies that begin just below a multiple of 4096 unflushed bytes
    for k, back in enumerate((258, 257, 65, 64, 3, 2, 1, 0)):
        for mult in (1, 2):
            n0 = 4096 * mult - back
            tokens = [(258, 1), (258, n0), 1, (3, 2), (258, 65), 2] + [(64, 64)] * 3
            c.tokens(f"flush_start{n0}", _bytes(n0, 90 + k), tokens, "fixed" if (k + mult) & 1 else "dynamic", suffix=_bytes(9, k)[1:])
    # cap: the image ends inside a copy and the stream goes on, reading on both sides of the image's last byte
    for k, (n0, into) in enumerate([(100, 1), (100, 16), (90, 63), (77, 64), (300, 65), (1000, 257), (4000, 100), (4090, 7), (WINDOW - 100, 101), (WINDOW - 100, 99)]):
        tokens = [(258, 7), 1, 2, 3, (258, 200 if n0 >= 200 else 5), (129, 1), 4, (258, 258), (65, 300 if n0 >= 300 else 64)] + list(_bytes(40, k)) + [(258, 40)]
        c.tokens(f"cap_{n0}_plus{into}", _bytes(n0, 110 + k), tokens, "dynamic" if k & 1 else "fixed", cap=n0 + into, suffix=b"\x09" * 3)
    tail = [(258, 1)] * 160 + list(_bytes(300, 5)) + [(258, 300)] * 40  # more than a ring and several flushes past the image
    c.tokens("cap_then_52000_more", _bytes(50, 3), tail, "dynamic", cap=45)


def _huffman_cases(c):
    # a literal/length code with every length 1 ... 15, every symbol of it used; then the same for the distance code
    order = [0x41] + list(range(1, 14)) + [256, 0]  # lengths 1, 2, ..., 15, 15
    lit_lens = [0] * 257
    for l, s in enumerate(order[:-1], 1):
        lit_lens[s] = l
    lit_lens[0] = 15
    tokens = [0] + [s for s in order[:-2]] * 3 + [0, 13, 12, 0x41, 0]
    c.add("lit_lengths_1_to_15", [dynamic(tokens, lit_lens, [0], True)], expand(tokens))
    p = _bytes(300, 29)
    t = [(3, DIST_BASE[s]) for s in range(16)] * 2
    c.add("dist_lengths_1_to_15", _stored_run(p) + [dynamic(t, fill_code(258, {}, [257, 256, 0]), list(range(1, 16)) + [15], True)], p + expand(t, p))
    # deep codes whose every symbol is used: lengths 10 ... 15 are all reached through the slow walk
    for depth in (10, 11, 12, 13, 14, 15):
        data = bytes([0]) + bytes(np.random.default_rng(depth).permutation(255).astype(np.uint8) + 1)
        tokens = list(data) + [(3 + k, 1 + k) for k in range(256)] + list(data[::-1])
        c.add(f"deep_code_{depth}", [dynamic_auto(tokens, True, max_len=depth, dist_max_len=depth, rng=np.random.default_rng(depth))], expand(tokens))
    # HLIT = 286 and HDIST = 30 with every length and distance symbol used (distance symbol 29 needs 24577 bytes of history)
    prefix = _bytes(WINDOW, 31)
    tokens = [(LEN_BASE[k] + (1 << LEN_EXTRA[k]) - 1 if k < 28 else 258, DIST_BASE[k] + (1 << DIST_EXTRA[k]) - 1) for k in range(29)] + \
             [(LEN_BASE[k], DIST_BASE[k]) for k in range(29)] + [(4, DIST_BASE[29]), (5, WINDOW)]
    c.tokens("all_length_and_distance_symbols", prefix, tokens, "dynamic", max_len=15, dist_max_len=15, extra_lit=range(200))
    c.tokens("all_length_and_distance_symbols_fixed", prefix, tokens, "fixed")
    # 258 spelled as symbol 284 with extra bits 31
    for kind in ("fixed", "dynamic"):
        c.tokens(f"length_258_as_284_plus_31_{kind}", _bytes(300, 41), [(258, 300, 284), 1, (258, 1, 284), (258, 258), (257, 2)], kind)
    # distance codes that huff_build treats specially
    lit_lens = fill_code(286, {}, [0, 1, 2, 3, 256, 257, 258, 285], rng=None)
    c.add("single_distance_code_symbol_0", [dynamic([0, 1, 2, 3, (3, 1), (4, 1), (258, 1)], lit_lens, [1], True)], expand([0, 1, 2, 3, (3, 1), (4, 1), (258, 1)]))
    t = [0, 1, 2, 3, 1, 2, (3, 5), (4, 6), (258, 5)]
    c.add("single_distance_code_symbol_4", [dynamic(t, lit_lens, [0, 0, 0, 0, 1], True)], expand(t))
    t = [0] + list(_bytes(25000, 43)) + [(258, 24577), (3, 25200)]
    c.add("single_distance_code_symbol_29", [dynamic_auto(t[:-2]), dynamic(t[-2:], lit_lens, [0] * 29 + [1], True)], expand(t))
    c.add("no_distance_code", [dynamic([0, 1, 2, 3, 3, 2], lit_lens, [0], True)], bytes([0, 1, 2, 3, 3, 2]))
    c.add("no_distance_code_hdist_30", [dynamic([0, 1, 2], lit_lens, [0] * 30, True)], bytes([0, 1, 2]))
    eob_only = [0] * 256 + [1]
    c.add("literal_code_of_end_of_block_alone", [fixed([0, 5]), dynamic([], eob_only, [0]), dynamic([], eob_only, [1]), fixed([6], True)], bytes([0, 5, 6]))
    c.add("two_code_literal_code", [fixed([0]), dynamic([7, 7, 7], fill_code(257, {}, [7, 256]), [0], True)], bytes([0, 7, 7, 7]))


def _header_cases(c):
    base = [0, 9, 9, 8, (5, 2), (3, 1)]
    raw = expand(base)
    # repeat codes whose run crosses from the literal/length lengths into the distance lengths
    lit = fill_code(286, {283: 2, 284: 2, 285: 2}, [0, 8, 9, 256, 259, 257])  # ends 2 2 2; distance lengths 2 2 2 2 follow
    head = cl_rle(lit[:283])
    c.add("repeat_16_crosses_into_distances", [dynamic(base, lit, [2, 2, 2, 2], True, cl_sequence=head + [2, (16, 6)])], raw)
    c.add("repeat_16_ends_at_the_boundary", [dynamic(base, lit, [2, 2, 2, 2], True, cl_sequence=head + [2, 2, 2] + [2, (16, 3)])], raw)
    lit = fill_code(280, {}, [0, 8, 9, 256, 259, 257, 1, 2])
    lit += [0] * 6
    head = cl_rle(lit[:260])
    assert lit[260:] == [0] * 26
    far = [0, 9, 9, 8, 1, 2, 8, 9, (5, 5), (3, 8), (5, 6)]  # (distance symbols 4 and 5)
    c.add("repeat_18_crosses_into_distances", [dynamic(far, lit, [0, 0, 0, 0, 1, 1], True, cl_sequence=head + [(18, 30), 1, 1])], expand(far))
    c.add("repeat_17_crosses_into_distances", [dynamic(far, lit, [0, 0, 0, 0, 1, 1], True, cl_sequence=head + [(18, 20), (17, 10), 1, 1])], expand(far))
    c.add("repeat_18_is_the_whole_tail", [dynamic([0, 8, 9, 8], lit, [0] * 30, True, cl_sequence=head + [(18, 56)])], bytes([0, 8, 9, 8]))
    c.add("repeat_17_ends_exactly_at_the_end", [dynamic([0, 8, 9, 8], lit, [0] * 4, True, cl_sequence=head + [(18, 23), (17, 7)])], bytes([0, 8, 9, 8]))
    c.add("repeat_16_ends_exactly_at_the_end", [dynamic(base, lit, [1, 1] + [0] * 9 + [0], True, cl_sequence=head + [(18, 26), 1, 1, 0, (16, 6), (16, 3)])], expand(base))
    # a code-length code that uses all 19 symbols, HCLEN = 19
    lit = fill_code(286, {k: k + 1 for k in range(1, 15)}, [0, 256, 257, 258, 17, 40, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29])
    seq = cl_rle(lit + [1, 1])
    used = {it[0] if isinstance(it, tuple) else it for it in seq}
    assert used == set(range(19)), sorted(used)
    t = [0, 20, 21, 29, 1, 14, 13, 2, (3, 1), (4, 2), 14]
    c.add("all_19_code_length_symbols", [dynamic(t, lit, [1, 1], True, cl_sequence=seq, cl_lens=limited_code([1] * 19, 7, limit=7), hclen=19)], expand(t))
    c.add("hclen_19_with_trailing_zero_lengths", [dynamic(base, *_simple(base), final=True, hclen=19)], raw)
    # the shortest header that can carry a non-zero length: 16 17 18 0 8
    t = [1, 200, 255, 1]
    c.add("hclen_5", [fixed([0]), dynamic(t, [0] + [8] * 256, [0], True, cl_sequence=[0, 8] + [(16, 6)] * 42 + [(16, 3), 0], hclen=5)], bytes([0] + t))


def _simple(tokens):
    lf, df = token_freqs(tokens)
    return limited_code(lf[:max(257, max(s for s in range(286) if lf[s]) + 1)]), limited_code(df[:max([1] + [s + 1 for s in range(30) if df[s]])])


def _block_cases(c):
    d = _bytes(70000, 61)
    c.add("empty_stored_blocks", [stored(b""), fixed([0, 1]), stored(b""), stored(b""), dynamic_auto([2, (3, 1)]), stored(b""), stored(b"", True)], bytes([0, 1, 2, 2, 2, 2]))
    c.add("final_empty_fixed_block", [stored(d[:9]), fixed([], True)], d[:9])
    c.add("only_empty_blocks_around_two_bytes", [fixed([]), stored(b""), fixed([0, 7]), dynamic([], [0] * 256 + [1], [0]), fixed([], True)], bytes([0, 7]))
    # a stored block that begins while the bit buffer still holds whole bytes, shorter and longer than what it holds
    for n in (0, 1, 2, 3, 4, 5, 7, 8, 9, 64, 300):
        blocks = [fixed([0, 1, 2]), stored(d[100:100 + n]), fixed([3]), stored(d[500:500 + n]), dynamic_auto([4, 5, (3, 2)]), stored(d[900:900 + n], True)]
        c.add(f"stored_{n}_after_huffman_blocks", blocks, bytes([0, 1, 2]) + d[100:100 + n] + b"\x03" + d[500:500 + n] + bytes([4, 5, 4, 5, 4]) + d[900:900 + n])
    for n in (4095, 4096, 4097, 65535):
        t = [(258, min(n, WINDOW)), 1]
        c.add(f"stored_{n}", [stored(d[:n]), fixed(t, True)], d[:n] + expand(t, d[:n]))
        c.add(f"stored_{n}_after_3_bytes", [fixed([0, 1, 2]), stored(d[:n], True)], bytes([0, 1, 2]) + d[:n])
    # hundreds of tiny blocks of alternating types
    blocks, out = [], bytearray()
    for k in range(400):
        if k % 3 == 0:
            b = d[k:k + 1 + k % 4]
            blocks.append(stored(b))
            out += b
        else:
            t = [d[k], (3 + k % 30, 1 + k % min(len(out), 40))] if out and k % 2 else [d[k]]
            blocks.append(fixed(t) if k % 3 == 1 else dynamic_auto(t, max_len=1 + k % 3))
            out += expand(t, bytes(out))
    blocks.append(stored(b"", True))
    c.add("400_tiny_blocks", blocks, out)


def _flush_cases(c):
    # final flushes of every residue mod 16 and mod 64, below and above one 4 KiB flush
    d = _bytes(5000, 67)
    for r in range(64):
        n = 100 + r
        if r & 1:
            c.add(f"final_flush_of_{n}", [stored(d[:n - 40]), fixed([(40, n - 40)], True)], d[:n - 40] + d[:40])
        else:
            c.add(f"final_flush_of_{n}", [fixed(list(d[:50])), stored(d[50:n], True)], d[:n])
    for n in (4095, 4096 + 1, 4096 + 15, 4096 + 16, 4096 + 17, 4096 + 63, 4096 + 64, 4096 + 65, 8191, 8192):
        t = [(258, 100)] * ((n - 100) // 258) + list(d[:(n - 100) % 258])
        c.add(f"final_flush_at_{n}", [stored(d[:100]), fixed(t, True)], d[:100] + expand(t, d[:100]))
    # long all-0xFF outputs: the Adler sums are largest before their reductions
    for n in (4096, 5552, 5553, 65536, 199_999):
        t = [0, 255] + [(258, 1)] * ((n - 2) // 258)
        t += [255] * (n - len(expand(t)))
        c.add(f"all_ff_{n}", [dynamic_auto(t, True)], expand(t))
    ff = b"\x00" + b"\xff" * 65534
    c.add("all_ff_stored_twice", [stored(ff), stored(ff[1:] + b"\xff", True)], ff + ff[1:] + b"\xff")


@functools.lru_cache(maxsize=None)
def _named():
    c = _Corpus()
    _copy_cases(c)
    _huffman_cases(c)
    _header_cases(c)
    _block_cases(c)
    _flush_cases(c)
    return tuple(c.items)


def named_streams():
    """[(name, zlib bytes, expected raw bytes)]; stream_cap(name) = the bytes a carrier's image keeps (less than all for cap_*)"""
    return [(n, z, raw) for n, z, raw, _ in _named()]


def stream_cap(name):
    return {n: cap for n, _, _, cap in _named()}[name]


# ---------------------------------------------------------------- random streams

def _random_tokens(rng, out, count):
    tokens, alphabet = [], int(rng.choice([2, 4, 16, 64, 256]))
    base = int(rng.integers(0, 256))
    n = len(out)
    for _ in range(count):
        if n and rng.random() < 0.55:
            far = min(n, WINDOW)
            dist = int(rng.choice(EDGE_DISTS + (WINDOW, WINDOW - 1, 4096, 4097))) if rng.random() < 0.5 else int(rng.integers(1, far + 1))
            if dist > far:
                dist = far
            length = int(rng.choice(EDGE_LENS)) if rng.random() < 0.5 else int(rng.integers(3, 259))
            tokens.append((length, dist, 284) if length == 258 and rng.random() < 0.3 else (length, dist))
            n += length
        else:
            tokens.append((base + int(rng.integers(0, alphabet))) & 255)
            n += 1
    return tokens


def _random_dynamic(rng, tokens, final):
    lf, df = token_freqs(tokens)
    nlen = int(rng.integers(max(257, max(s for s in range(286) if lf[s]) + 1), 287))
    ndist = int(rng.integers(max([1] + [s + 1 for s in range(30) if df[s]]), 31))
    depth, ddepth = int(rng.integers(1, 16)), int(rng.integers(1, 16))
    # a code of depth d needs d + 1 symbols: symbols no token uses get codes until there are enough (and some more at random)
    free = [s for s in rng.permutation(nlen) if not lf[s]]
    for s in free[:max(0, depth + 1 - sum(1 for f in lf if f)) + int(rng.integers(0, 5))]:
        lf[int(s)] = 1
    if any(df) or rng.random() < 0.5:
        free = [s for s in rng.permutation(ndist) if not df[s]]
        want = max(0, ddepth + 1 - sum(1 for f in df if f)) if any(df) or rng.random() < 0.7 else 1
        for s in free[:want]:
            df[int(s)] = 1
    lit_lens, dist_lens = limited_code(lf[:nlen], depth, rng=rng), limited_code(df[:ndist], ddepth, rng=rng)
    seq = cl_rle(lit_lens + dist_lens, rng)
    f = [0] * 19
    for it in seq:
        f[it[0] if isinstance(it, tuple) else it] += 1
    for s in rng.permutation(19)[:int(rng.integers(0, 4)) + (2 if sum(1 for x in f if x) < 2 else 0)]:
        f[int(s)] += 1
    cl_lens = limited_code(f, int(rng.integers(1, 8)), limit=7, rng=rng)
    need = max(k for k in range(19) if cl_lens[CL_ORDER[k]]) + 1
    return dynamic(tokens, lit_lens, dist_lens, final, cl_sequence=seq, cl_lens=cl_lens, hclen=int(rng.integers(max(4, need), 20)))


def random_streams(seed, n):
    """[(name, zlib bytes, expected raw bytes)]: 1-12 blocks of random types, tokens biased to matches with lengths and distances from
    the edge sets and uniform, never farther back than the output so far, random length-limited codes of a forced depth 1-15, random
    repeats in the code-length sequence, empty stored blocks at random.  The first byte is 0."""
    rng = np.random.default_rng(seed)
    res = []
    for k in range(n):
        out, blocks = bytearray(), []
        nblocks = int(rng.integers(1, 13))
        if rng.random() < 0.2:  # start near the ring's wrap
            out += _bytes(int(rng.integers(WINDOW - 300, WINDOW + 300)), int(rng.integers(0, 1 << 30)))
            blocks += [stored(bytes(out))]
        for b in range(nblocks):
            final = b == nblocks - 1
            if rng.random() < 0.2:
                blocks.append(stored(b""))
            kind = int(rng.integers(0, 3))
            if kind == 0:
                size = int(rng.choice([0, 1, 2, 5, 63, 64, 65, 300, 4095, 4096, 4097])) if rng.random() < 0.8 else int(rng.integers(0, 20000))
                data = bytes(rng.integers(0, 256, size).astype(np.uint8))
                if not out and data:
                    data = b"\x00" + data[1:]
                blocks.append(stored(data, final))
                out += data
                continue
            count = int(rng.choice([0, 1, 3, 20, 100, 400])) if len(out) < 150_000 else 1
            tokens = _random_tokens(rng, out, count)
            if not out:
                tokens = [0] + tokens
            blocks.append(fixed(tokens, final) if kind == 1 else _random_dynamic(rng, tokens, final))
            out += expand(tokens, bytes(out))
        if len(out) < 2:
            blocks.insert(0, fixed([0, 1]))
            out = bytearray([0, 1]) + out
            assert out[0] == 0
        assert len(out) <= 200_000
        res.append((f"random{seed}_{k}", zlib_stream(blocks, out), bytes(out)))
    return res


# ---------------------------------------------------------------- refused streams

def refused_streams():
    """[(name, zlib bytes, cap)]: invalid twins of named cases, one bit of structure apart; cap = the bytes of the valid twin (the
    carrier's geometry).  zlib.decompress raises on every one."""
    out = []

    def add(name, blocks, raw, adler=None):
        out.append((name, zlib_stream(blocks, raw, adler), max(2, len(raw))))

    # a distance one byte too far at each phase of the output
    for n0 in (1, 2, 64, 257, 4095, 4096, 4097, WINDOW - 258, WINDOW - 1):
        p = _bytes(n0, n0)
        good = expand([(258, n0)], p)
        for kind in ("fixed", "dynamic"):
            t = [(258, n0 + 1)]
            blk = fixed(t, True) if kind == "fixed" else dynamic_auto(t, True)
            add(f"distance_{n0 + 1}_after_{n0}_bytes_{kind}", _stored_run(p) + [blk], p + good)
    lit_lens = fill_code(286, {}, [0, 1, 2, 3, 256, 257, 258, 285])
    # the unassigned pattern of a single-code distance tree: the length symbol, then bit 1 where the only code is 0
    for name, dl in (("symbol_0", [1]), ("symbol_4", [0, 0, 0, 0, 1])):
        add(f"single_distance_code_{name}_unassigned_pattern", [dynamic([0, 1, 2, 3, 1, 2, ("sym", 257), ("bits", 1, 1), ("bits", 0, 1)], lit_lens, dl, True)],
            bytes([0, 1, 2, 3, 1, 2, 1, 2, 1]))
    add("lone_distance_code_of_length_2", [dynamic([0, 1, 2, 3], lit_lens, [2], True, check=False)], bytes([0, 1, 2, 3]))
    add("a_match_where_there_is_no_distance_code", [dynamic([0, 1, 2, 3, ("sym", 257), ("bits", 0, 1)], lit_lens, [0], True)], bytes([0, 1, 2, 3, 3, 3, 3]))
    # the code-length sequence
    lit = fill_code(280, {}, [0, 8, 9, 256, 259, 257, 1, 2]) + [0] * 6
    head = cl_rle(lit[:260])
    base = [0, 9, 9, 8, (5, 2), (3, 1)]
    raw = expand(base)
    lit1 = list(lit)
    cl = limited_code([1] * 19, limit=7)
    add("code_16_first", [dynamic(base, lit, [1, 1], True, cl_sequence=[(16, 3)] + cl_rle(lit[3:] + [1, 1]), cl_lens=cl, check=False)], raw)
    add("run_one_past_the_end_18", [dynamic(base[:4], lit, [0] * 4, True, cl_sequence=head + [(18, 31)], cl_lens=cl, check=False)], raw[:4])
    add("run_one_past_the_end_17", [dynamic(base[:4], lit, [0] * 4, True, cl_sequence=head + [(18, 23), (17, 8)], cl_lens=cl, check=False)], raw[:4])
    add("run_one_past_the_end_16", [dynamic(base, lit, [1, 1] + [0] * 10, True, cl_sequence=head + [(18, 26), 1, 1, 0, (16, 6), (16, 4)], cl_lens=cl, check=False)], raw)
    lit1[256] = 0
    lit1[3] = lit[256]  # (the same code space, the end-of-block code given to another symbol)
    assert lit[3] == 0
    add("no_end_of_block_code", [dynamic(base[:4], lit1, [0], True, eob=False, check=False)], raw[:4])
    add("hlit_287", [dynamic(base[:4], lit + [0], [0], True, cl_sequence=cl_rle(lit + [0, 0]), check=False)], raw[:4])
    add("symbol_286_fixed", [fixed([0, 1, ("sym", 286)], True)], bytes([0, 1]))
    add("symbol_287_fixed", [fixed([0, 1, ("sym", 287)], True)], bytes([0, 1]))
    add("distance_symbol_30_fixed", [fixed([0, 1, ("sym", 257), ("dsym", 30)], True)], bytes([0, 1, 1, 1, 1]))
    add("distance_symbol_30_dynamic", [dynamic([0, 1, ("sym", 257), ("dsym", 30)], lit_lens, [0] * 30 + [1], True, check=False)], bytes([0, 1, 1, 1, 1]))
    add("oversubscribed_distance_code", [dynamic([0, 1], lit_lens, [1, 1, 1], True, check=False)], bytes([0, 1]))
    add("incomplete_literal_code", [dynamic([0, 1], [l + (s == 285) for s, l in enumerate(lit_lens)], [0], True, check=False)], bytes([0, 1]))
    # an Adler-32 that is off by one after a long all-0xFF output
    for n in (5553, 199_999):
        t = [0, 255] + [(258, 1)] * ((n - 2) // 258)
        t += [255] * (n - len(expand(t)))
        raw = expand(t)
        a = zlib.adler32(raw) & 0xFFFFFFFF
        add(f"adler_low_half_off_by_one_after_all_ff_{n}", [dynamic_auto(t, True)], raw, adler=a ^ 1)
        add(f"adler_high_half_off_by_one_after_all_ff_{n}", [dynamic_auto(t, True)], raw, adler=(a + 0x10000) & 0xFFFFFFFF)
    return out


# ---------------------------------------------------------------- what the test modules share

RANDOM_SEED, RANDOM_COUNT = 2026, 150


@functools.lru_cache(maxsize=None)
def valid_streams():
    """[(name, zlib bytes, raw bytes, cap)]: the named streams and RANDOM_COUNT random ones"""
    return tuple([(n, z, raw, stream_cap(n)) for n, z, raw in named_streams()] + [(n, z, raw, len(raw)) for n, z, raw in random_streams(RANDOM_SEED, RANDOM_COUNT)])


@functools.lru_cache(maxsize=None)
def carrier_files(carrier):
    """[(name, file, expected pixel bytes or None for a refused stream)] of every valid and refused stream; carrier: "png" or "tiff" """
    out = []
    for k, (name, z, raw, cap) in enumerate(valid_streams()):
        if carrier == "png":
            out.append((name, png_carrier(z, cap), raw[1:cap]))
        else:
            data, fill = tiff_carrier(z, cap, k)
            out.append((name, data, tiff_expected(raw, cap, fill)))
    for k, (name, z, cap) in enumerate(refused_streams()):
        out.append((name, png_carrier(z, cap) if carrier == "png" else tiff_carrier(z, cap, k)[0], None))
    return tuple(out)
