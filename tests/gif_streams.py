"""GIF files for the tests of the GIF path (include/rupphash.h, GIF section): a numpy restatement of the pixel rule, a Python restatement of
the LZW rule, a small GIF writer whose LZW encoder does what the test tells it (Clear never / every N codes / when the table is full, EOI
or not, sub-block sizes, minimum code size), a raw-code mode for streams no encoder writes, and the three corpora the CPU and GPU tests
share: files Pillow writes, files the writer makes with their expected pixels, damaged files with their exact status.

    python tests/gif_streams.py DIR     dumps every file of the helper's corpora (valid and damaged) into DIR as *.gif
"""
import functools
import io
import struct

import numpy as np

INVALID, UNSUPPORTED = -1, -5
ENTRIES = 4096


# ---- the LZW rule, restated with a plain (prefix, byte) table ----
class _Widths:
    """the decoder's view of a code sequence: which width each code is read with"""

    def __init__(self, m):
        self.m, self.clear = m, 1 << m
        self.reset()
        self.have_prev = False

    def reset(self):
        self.next, self.width = self.clear + 2, self.m + 1

    def feed(self, code):
        """the width `code` is read with; then the state after it"""
        w = self.width
        if code == self.clear:
            self.reset()
            self.have_prev = False
        elif code != self.clear + 1:
            if self.have_prev and self.next < ENTRIES:
                self.next += 1
                if self.next == 1 << self.width and self.width < 12:
                    self.width += 1
            self.have_prev = True
        return w


def pack_codes(codes, m):
    """codes (ints, or (code, width) pairs that overrule the decoder's width) -> bytes, least significant bit first"""
    st, acc, nb, out = _Widths(m), 0, 0, bytearray()
    for c in codes:
        if isinstance(c, tuple):
            c, w = c
            st.feed(c)
        else:
            w = st.feed(c)
        acc |= c << nb
        nb += w
        while nb >= 8:
            out.append(acc & 255)
            acc >>= 8
            nb -= 8
    if nb:
        out.append(acc & 255)
    return bytes(out)


def lzw_encode(indices, m, clear="full", eoi=True):
    """indices -> code list.  clear: "never" (no Clear at all: the table fills up and stays, deferred clear), "full" (a Clear first and
    one whenever the table is full) or N (a Clear first and one after every N codes)."""
    cl, first = 1 << m, (1 << m) + 2
    codes = [] if clear == "never" else [cl]
    table, nxt, since = {}, first, 0
    w = None
    for b in indices:
        b = int(b)
        assert b < cl
        if w is None:
            w = (b,)
            continue
        wb = w + (b,)
        if len(wb) == 1 or wb in table:
            w = wb
            continue
        codes.append(w[0] if len(w) == 1 else table[w])
        since += 1
        if nxt < ENTRIES:
            table[wb] = nxt
            nxt += 1
        w = (b,)
        if (clear == "full" and nxt == ENTRIES) or (isinstance(clear, int) and since >= clear):
            codes.append(cl)
            table, nxt, since = {}, first, 0
    if w is not None:
        codes.append(w[0] if len(w) == 1 else table[w])
    if eoi:
        codes.append(cl + 1)
    return codes


def lzw_decode(stream, m, n):
    """the rule: n indices from the joined stream, or None for a stream that is refused"""
    cl, eoi, first = 1 << m, (1 << m) + 1, (1 << m) + 2
    bits = int.from_bytes(stream, "little")
    avail, used = 8 * len(stream), 0
    table = {}
    nxt, width, prev = first, m + 1, None
    out = []
    while len(out) < n:
        if used + width > avail:
            return None
        code = (bits >> used) & ((1 << width) - 1)
        used += width
        if code == cl:
            table, nxt, width, prev = {}, first, m + 1, None
            continue
        if code == eoi:
            return None
        if code < cl:
            s = [code]
        elif prev is None:
            return None
        elif code < nxt:
            s = table[code]
        elif code == nxt:
            s = prev + [prev[0]]
        else:
            return None
        out += s
        if prev is not None and nxt < ENTRIES:
            table[nxt] = prev + [s[0]]
            nxt += 1
            if nxt == 1 << width and width < 12:
                width += 1
        prev = s
    return np.array(out[:n], np.uint8)


def lzw_events(stream, m, n):
    """a trace of the rule over the same stream: one (kind, at, src, length, written, distinct, clipped) per code that gives bytes, in
    order, or None for a stream lzw_decode refuses.  kind: "literal", "copy" (a table entry) or "kwkwk" (the next free entry); at: the
    position in the frame's indices the string begins at; src: where the string it copies begins (an entry is the string before it and
    the byte behind that string; None for a literal); length: the string's bytes; written: those that fit the frame; distinct: the
    number of different bytes among the written ones; clipped: length > written.  Written for the tests' coverage claims, apart from
    lzw_decode: the table holds (position, length) as the device's does."""
    cl, eoi, first = 1 << m, (1 << m) + 1, (1 << m) + 2
    bits = int.from_bytes(stream, "little")
    avail, used = 8 * len(stream), 0
    pos, length = {}, {}
    nxt, width, prev = first, m + 1, None  # prev: (position, length) of the string before
    out, events = [], []
    while len(out) < n:
        if used + width > avail:
            return None
        code = (bits >> used) & ((1 << width) - 1)
        used += width
        if code == cl:
            pos, length, nxt, width, prev = {}, {}, first, m + 1, None
            continue
        if code == eoi:
            return None
        at, room = len(out), n - len(out)
        if code < cl:
            kind, src, ln = "literal", None, 1
            out.append(code)
        elif prev is None:
            return None
        elif code < nxt:
            kind, src, ln = "copy", pos[code], length[code]
        elif code == nxt:
            kind, src, ln = "kwkwk", prev[0], prev[1] + 1
        else:
            return None
        written = min(ln, room)
        if src is not None:
            for i in range(written):  # (forward, byte by byte: an overlapping copy repeats its period)
                out.append(out[src + i])
        events.append((kind, at, src, ln, written, len(set(out[at:at + written])), ln > written))
        if prev is not None and nxt < ENTRIES:
            pos[nxt], length[nxt] = prev[0], prev[1] + 1
            nxt += 1
            if nxt == 1 << width and width < 12:
                width += 1
        prev = (at, ln)
    return events


# ---- the pixel rule ----
def pass_order(h):
    return list(range(0, h, 8)) + list(range(4, h, 8)) + list(range(2, h, 4)) + list(range(1, h, 2))


def render(screen, pos, idx, pal, trans=None):
    """screen (w, h); frame at pos (x, y) with indices idx (fh, fw) in display order; pal (n, 3) -> (h, w, 4) Rgba8"""
    w, h = screen
    out = np.zeros((h, w, 4), np.uint8)
    pal = np.asarray(pal, np.uint8).reshape(-1, 3)
    fh, fw = idx.shape
    rgba = np.zeros((fh, fw, 4), np.uint8)
    ok = idx < len(pal)
    rgba[ok, :3] = pal[idx[ok]]
    rgba[ok, 3] = 255
    if trans is not None:
        rgba[ok & (idx == trans), 3] = 0
    x, y = pos
    cw, ch = max(0, min(fw, w - x)), max(0, min(fh, h - y))
    out[y:y + ch, x:x + cw] = rgba[:ch, :cw]
    return out


# ---- the writer ----
def sub_blocks(stream, size=255, terminator=True):
    """size: one block size, or a list of sizes used in turn"""
    sizes = [size] if isinstance(size, int) else list(size)
    out, pos, k = bytearray(), 0, 0
    while pos < len(stream):
        s = min(sizes[k % len(sizes)], len(stream) - pos)
        out.append(s)
        out += stream[pos:pos + s]
        pos += s
        k += 1
    if terminator:
        out.append(0)
    return bytes(out)


def table_bytes(pal):
    """(n, 3) with n a power of two from 2 to 256 -> (size field, bytes)"""
    pal = np.asarray(pal, np.uint8).reshape(-1, 3)
    n = len(pal)
    assert n in (2, 4, 8, 16, 32, 64, 128, 256)
    return n.bit_length() - 2, pal.tobytes()


def gce(trans=None, flags=None, index=None):
    f = (1 if trans is not None else 0) if flags is None else flags
    return b"\x21\xf9\x04" + bytes([f, 0, 0, (trans or 0) if index is None else index]) + b"\x00"


def write_gif(screen, pos, size, m, stream, gct=None, lct=None, interlace=False, trans=None, sub=255, terminator=True, trailer=True,
              version=b"GIF89a", before=b"", after=b""):
    """one frame of `size` (fw, fh) at pos on `screen`; stream: the LZW bytes before they are cut into sub-blocks"""
    out = bytearray(version)
    flags = 0
    if gct is not None:
        k, tb = table_bytes(gct)
        flags = 0x80 | k | (k << 4)
    out += struct.pack("<HHBBB", screen[0], screen[1], flags, 0, 0)
    if gct is not None:
        out += tb
    out += before
    if trans is not None:
        out += gce(trans)
    flags = 0x40 if interlace else 0
    if lct is not None:
        k, tb = table_bytes(lct)
        flags |= 0x80 | k
    out += b"\x2c" + struct.pack("<HHHHB", pos[0], pos[1], size[0], size[1], flags)
    if lct is not None:
        out += tb
    out.append(m)
    out += sub_blocks(stream, sub, terminator)
    if trailer:
        out += b"\x3b"
    return bytes(out + after)


def gray_palette(n):
    return np.repeat((np.arange(n) * 255 // max(1, n - 1)).astype(np.uint8)[:, None], 3, axis=1)


def colour_palette(n, seed=1):
    return np.random.default_rng(seed).integers(0, 256, (n, 3), dtype=np.uint8)


def image_gif(idx, pal, m=None, screen=None, pos=(0, 0), interlace=False, trans=None, clear="full", eoi=True, local=False, gct=None, **kw):
    """indices (fh, fw) in display order -> (file, expected pixels)"""
    idx = np.asarray(idx, np.uint8)
    fh, fw = idx.shape
    if m is None:
        m = max(2, (len(pal) - 1).bit_length())
    rows = idx[pass_order(fh)] if interlace else idx
    stream = pack_codes(lzw_encode(rows.ravel(), m, clear, eoi), m)
    screen = screen or (fw, fh)
    data = write_gif(screen, pos, (fw, fh), m, stream, gct=gct if local else pal, lct=pal if local else None, interlace=interlace, trans=trans, **kw)
    return data, render(screen, pos, idx, pal, trans)


def frame_stream(data):
    """a file of this writer taken apart again: (m, (fw, fh), the joined LZW bytes of its first frame)"""
    pos = 13 + (3 * (2 << (data[10] & 7)) if data[10] & 0x80 else 0)
    while data[pos] == 0x21:
        pos += 2
        while data[pos]:
            pos += 1 + data[pos]
        pos += 1
    assert data[pos] == 0x2C
    fw, fh, flags = struct.unpack_from("<HHB", data, pos + 5)
    pos += 10 + (3 * (2 << (flags & 7)) if flags & 0x80 else 0)
    m, pos, stream = data[pos], pos + 1, bytearray()
    while pos < len(data) and data[pos]:
        stream += data[pos + 1:pos + 1 + data[pos]]
        pos += 1 + data[pos]
    return m, (fw, fh), bytes(stream)


def raw_gif(codes, m, size, pal=None, **kw):
    """a frame of `size` from raw codes -> (file, expected pixels or None when the rule refuses the stream)"""
    pal = gray_palette(1 << m) if pal is None else pal
    stream = pack_codes(codes, m)
    data = write_gif(size, (0, 0), size, m, stream, gct=pal, **kw)
    idx = lzw_decode(stream, m, size[0] * size[1])
    return data, None if idx is None else render(size, (0, 0), idx.reshape(size[1], size[0]), pal)


# ---- corpus 1: files Pillow writes (expected pixels: Pillow's own, in the test) ----
@functools.lru_cache(maxsize=None)
def pillow_files():
    from PIL import Image

    rng = np.random.default_rng(11)
    out = []

    def save(name, idx, pal, **kw):
        idx = np.ascontiguousarray(idx, np.uint8)
        im = Image.frombytes("P", (idx.shape[1], idx.shape[0]), idx.tobytes())
        im.putpalette(np.asarray(pal, np.uint8).tobytes())
        buf = io.BytesIO()
        im.save(buf, format="GIF", **{"optimize": False, **kw})
        out.append((name, buf.getvalue()))

    for w, h in ((1, 1), (5, 5), (64, 48)):
        save(f"size_{w}x{h}", rng.integers(0, 16, (h, w)), colour_palette(16, w))
    save("noise_300x200", rng.integers(0, 256, (200, 300)), colour_palette(256, 2))  # fills the table: Clears
    for n in (2, 4, 16, 256):  # minimum code sizes 2, 2, 4, 8
        yy, xx = np.mgrid[0:40, 0:52]
        idx = ((xx // 3 + yy // 2) % n) ^ rng.integers(0, 2, (40, 52)) * (n > 2) if n < 256 else rng.integers(0, 256, (40, 52))
        save(f"colours_{n}", idx, colour_palette(n, n), optimize=True)  # (the colour table cut to the colours used)
    # (Pillow's writer never interlaces an image with a side below 16 px: heights 1 .. 9 are written by this helper, interlaced_files())
    for h in (16, 17, 18, 19, 20, 21, 22, 23, 67):
        save(f"interlaced_{h}", rng.integers(0, 64, (h, 33)), colour_palette(64, h), interlace=True)
    save("transparent", rng.integers(0, 8, (20, 30)), colour_palette(8, 5), transparency=3)
    # a two-frame animation: the first frame is decoded
    a = Image.frombytes("P", (32, 24), rng.integers(0, 16, (24, 32), dtype=np.uint8).tobytes())
    b = Image.frombytes("P", (32, 24), rng.integers(0, 16, (24, 32), dtype=np.uint8).tobytes())
    for im in (a, b):
        im.putpalette(colour_palette(16, 9).tobytes())
    buf = io.BytesIO()
    a.save(buf, format="GIF", save_all=True, append_images=[b], duration=40, loop=0, optimize=False)
    out.append(("animation_2_frames", buf.getvalue()))
    return out


@functools.lru_cache(maxsize=None)
def interlaced_files():
    """interlaced frames at every height from 1 to 9 (and 67), from this writer: Pillow reads them, and the restatement has them too"""
    rng = np.random.default_rng(12)
    return [(f"interlaced_h{h}",) + image_gif(rng.integers(0, 16, (h, 7 + h)), colour_palette(16, h), interlace=True) for h in (1, 2, 3, 4, 5, 6, 7, 8, 9, 67)]


# ---- corpus 2: files of the writer, with the pixels the rule gives ----
@functools.lru_cache(maxsize=None)
def valid_files():
    rng = np.random.default_rng(13)
    out = list(interlaced_files())

    def add(name, pair):
        assert pair[1] is not None, name
        out.append((name, pair[0], pair[1]))

    pal16, other16 = colour_palette(16, 21), colour_palette(16, 22)
    idx = rng.integers(0, 16, (12, 20))
    add("local_palette_overrides_global", image_gif(idx, pal16, local=True, gct=other16))
    add("local_palette_only", image_gif(idx, pal16, local=True))
    add("frame_at_offset", image_gif(idx, pal16, screen=(40, 30), pos=(7, 5)))
    add("frame_past_the_screen", image_gif(idx, pal16, screen=(24, 14), pos=(10, 6)))
    add("frame_wholly_outside", image_gif(idx, pal16, screen=(10, 10), pos=(10, 3)))
    add("index_beyond_palette", image_gif(rng.integers(0, 16, (9, 9)), colour_palette(8, 23), m=4))
    add("transparent_index", image_gif(rng.integers(0, 4, (9, 11)), colour_palette(4, 24), trans=2))
    add("transparent_index_interlaced_offset", image_gif(rng.integers(0, 4, (13, 11)), colour_palette(4, 24), trans=0, interlace=True, screen=(20, 20), pos=(3, 4)))
    add("gif87a", image_gif(idx, pal16, version=b"GIF87a"))
    ext = b"\x21\xfe\x05hello\x03abc\x00" + gce(5) + b"\x21\xff\x0bNETSCAPE2.0\x03\x01\x00\x00\x00" + gce(None, flags=1, index=3)
    add("extensions_last_gce_counts", (write_gif((20, 12), (0, 0), (20, 12), 4, pack_codes(lzw_encode(idx.ravel(), 4), 4), gct=pal16, before=ext),
                                       render((20, 12), (0, 0), idx, pal16, 3)))
    for w in (63, 64, 65, 129):  # the expand kernel's 64-pixel steps
        add(f"width_{w}", image_gif(rng.integers(0, 32, (6, w)), colour_palette(32, w), screen=(w + 2, 7), pos=(1, 1)))
    for m in range(2, 9):
        add(f"min_code_size_{m}", image_gif(rng.integers(0, 1 << m, (37, 41)), colour_palette(1 << m, m), m=m))
        add(f"min_code_size_{m}_no_clear", image_gif(rng.integers(0, 1 << m, (23, 19)), colour_palette(1 << m, m), m=m, clear="never"))
    noise = rng.integers(0, 256, (96, 96))  # 9216 noise indices: 4096 entries are reached after ~3840 codes, then width 12 to the end
    add("deferred_clear_8", image_gif(noise, colour_palette(256, 31), clear="never"))
    assert len(lzw_encode(noise.ravel(), 8, "never")) > 2 * ENTRIES
    add("deferred_clear_2", image_gif(rng.integers(0, 4, (180, 180)), colour_palette(4, 32), clear="never"))
    add("deferred_clear_then_clear", image_gif(noise, colour_palette(256, 31), clear=6000))
    add("clear_when_full", image_gif(noise, colour_palette(256, 31), clear="full"))
    add("clear_every_5", image_gif(noise[:20], colour_palette(256, 31), clear=5))
    add("clear_every_300_large", image_gif(rng.integers(0, 3, (150, 200)), colour_palette(4, 33), clear=300))  # > 16 KiB: built in global memory
    # a flat image: every code after the first is the KwKwK code, each copy overlapping its own output; strings of 2 .. 129 bytes, then the
    # entries of 63, 64, 65, 127, 128 and 129 bytes again as plain copies
    first = 6
    codes = [4, 1] + [first + k for k in range(128)] + [first + (n - 2) for n in (63, 64, 65, 127, 128, 129)]
    total = sum(range(1, 130)) + 63 + 64 + 65 + 127 + 128 + 129
    assert total == 87 * 103
    add("flat_kwkwk_chain", raw_gif(codes, 2, (87, 103)))
    add("flat_image_encoded", image_gif(np.full((90, 100), 3), colour_palette(4, 34)))
    add("flat_image_large", image_gif(np.full((200, 300), 1), colour_palette(4, 34), clear="never"))
    # the width steps from 3 to 4 exactly on the last code (the third code adds entry 7): nothing follows, or EOI at 4 bits
    add("width_step_on_last_code", raw_gif([4, 0, 1, 2], 2, (3, 1)))
    add("width_step_on_last_code_eoi", raw_gif([4, 0, 1, 2, 5], 2, (3, 1)))
    add("width_step_then_one_code", raw_gif([4, 0, 1, 2, 3], 2, (4, 1)))
    row = rng.integers(0, 64, (30, 50))
    for sub in (1, 254, 255, [1, 255, 2, 254]):  # sub-blocks that split codes
        add(f"sub_blocks_{sub if isinstance(sub, int) else 'mixed'}", image_gif(row, colour_palette(64, 35), sub=sub))
    add("first_code_not_clear", image_gif(row, colour_palette(64, 35), clear="never"))
    add("clear_clear", raw_gif([4, 4, 0, 1, 6, 4, 4, 4, 2, 8 - 2, 5], 2, (7, 1)))
    add("missing_eoi", image_gif(row, colour_palette(64, 35), eoi=False))
    add("missing_terminator", image_gif(row, colour_palette(64, 35), terminator=False, trailer=False))
    add("missing_eoi_and_terminator", image_gif(row, colour_palette(64, 35), eoi=False, terminator=False, trailer=False))
    add("trailing_junk", image_gif(row, colour_palette(64, 35), after=bytes(rng.integers(0, 256, 100, dtype=np.uint8))))
    add("codes_after_the_frame_is_full", raw_gif([4, 0, 1, 2, 3, 15, 15, 15], 2, (3, 1)))  # (15 would be above the next free entry)
    add("small_1x1", image_gif([[1]], colour_palette(2, 36)))
    add("small_4x9", image_gif(rng.integers(0, 4, (9, 4)), colour_palette(4, 36)))
    add("small_screen_large_frame", image_gif(rng.integers(0, 4, (9, 9)), colour_palette(4, 36), screen=(3, 3), pos=(0, 0)))
    # screens with a side above 512 px: the hasher box-downsamples them to a thumbnail first (Rgba8 at the screen's pitch)
    big = np.random.default_rng(37)  # (a generator of their own: the files above stay what they were)

    def scene(fh, fw, colours):
        yy, xx = np.mgrid[0:fh, 0:fw]
        return ((xx // 23 + 2 * (yy // 17) + (xx * yy) // 4099 + big.integers(0, 2, (fh, fw))) % colours).astype(np.uint8)

    add("above_512_700x90", image_gif(scene(90, 700, 64), colour_palette(64, 38)))
    add("above_512_90x700", image_gif(scene(700, 90, 64), colour_palette(64, 39), interlace=True))
    add("above_512_1024x600_frame_at_offset_transparent", image_gif(scene(500, 900, 32), colour_palette(32, 40), screen=(1024, 600), pos=(61, 37), trans=5))
    return out


# ---- corpus 3: damaged files, one per line of the rule, with their exact status ----
@functools.lru_cache(maxsize=None)
def damaged_files():
    rng = np.random.default_rng(14)
    pal = colour_palette(4, 41)
    idx = rng.integers(0, 4, (10, 12))
    good, _ = image_gif(idx, pal)
    stream = pack_codes(lzw_encode(idx.ravel(), 2), 2)
    long_stream = pack_codes(lzw_encode(rng.integers(0, 4, 600), 2), 2)
    assert len(long_stream) >= 40
    hdr = 13 + 12  # signature, screen descriptor, 4-entry global table
    out = []

    def add(name, data, status):
        out.append((name, bytes(data), status))

    def patch(at, val, base=None):
        d = bytearray(good if base is None else base)
        d[at:at + len(val)] = val
        return d

    # REFUSED
    add("bad_signature", b"GIF88a" + good[6:], INVALID)
    add("short_signature", good[:4], INVALID)
    add("screen_descriptor_cut", good[:11], INVALID)
    add("global_table_cut", good[:hdr - 3], INVALID)
    add("extension_label_cut", good[:hdr] + b"\x21", INVALID)
    add("extension_sub_block_cut", good[:hdr] + b"\x21\xfe\x09abc", INVALID)
    add("extension_without_terminator", good[:hdr] + b"\x21\xfe\x03abc", INVALID)
    add("image_descriptor_cut", good[:hdr + 5], INVALID)
    add("local_table_cut", write_gif((12, 10), (0, 0), (12, 10), 2, stream, lct=pal)[:13 + 10 + 7], INVALID)
    add("code_size_byte_missing", good[:hdr + 10], INVALID)
    add("data_sub_block_cut", good[:hdr + 10 + 1 + 5], INVALID)
    add("no_image_before_trailer", good[:hdr] + gce(1) + b"\x3b", INVALID)
    add("no_image_before_end", good[:hdr] + gce(1), INVALID)
    add("no_image_at_all", good[:hdr], INVALID)
    add("unknown_block_introducer", good[:hdr] + b"\x00" + good[hdr:], INVALID)
    add("zero_screen_width", patch(6, b"\x00\x00"), INVALID)
    add("zero_screen_height", patch(8, b"\x00\x00"), INVALID)
    add("zero_frame_width", patch(hdr + 5, b"\x00\x00"), INVALID)
    add("zero_frame_height", patch(hdr + 7, b"\x00\x00"), INVALID)
    add("no_colour_table", write_gif((12, 10), (0, 0), (12, 10), 2, stream), INVALID)
    add("code_above_next_free", raw_gif([4, 0, 7, 0, 0, 0, 0, 0, 0], 2, (8, 1))[0], INVALID)
    add("code_above_next_free_full_width", raw_gif([4, 0, 1, 2, 3, 0, 15, 0, 0, 0, 0, 0, 0], 2, (12, 1))[0], INVALID)
    add("first_code_above_clear", raw_gif([6, 0, 1, 2], 2, (4, 1))[0], INVALID)
    add("first_code_after_clear_above_clear", raw_gif([4, 0, 1, 4, 6, 0, 0], 2, (6, 1))[0], INVALID)
    add("kwkwk_as_first_code_after_clear", raw_gif([4, 0, 1, 2, 4, 6, 0, 0, 0, 0], 2, (9, 1))[0], INVALID)
    add("out_of_bits", write_gif((12, 10), (0, 0), (12, 10), 2, stream[:len(stream) // 2], gct=pal), INVALID)
    add("eoi_before_the_frame_is_full", raw_gif([4, 0, 1, 2, 5, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0], 2, (8, 1))[0], INVALID)
    add("eoi_first", raw_gif([5, 0, 0, 0], 2, (2, 1))[0], INVALID)
    add("eoi_after_clear", raw_gif([4, 5, 0, 0], 2, (2, 1))[0], INVALID)
    # UNSUPPORTED
    add("code_size_1", patch(hdr + 10, b"\x01"), UNSUPPORTED)
    add("code_size_0", patch(hdr + 10, b"\x00"), UNSUPPORTED)
    add("code_size_9", patch(hdr + 10, b"\x09"), UNSUPPORTED)
    add("code_size_12", patch(hdr + 10, b"\x0c"), UNSUPPORTED)
    add("screen_above_2_28_pixels", patch(6, struct.pack("<HH", 16385, 16384)), UNSUPPORTED)
    add("frame_above_2_28_pixels", write_gif((12, 10), (0, 0), (16385, 16384), 2, bytes(200000), gct=pal), UNSUPPORTED)
    # 40 stream bytes at m = 2 give at most 4091 * floor(320 / 3) = 433646 indices
    add("frame_above_the_expansion_bound", write_gif((12, 10), (0, 0), (700, 620), 2, long_stream[:40], gct=pal), UNSUPPORTED)
    add("frame_without_data", write_gif((12, 10), (0, 0), (12, 10), 2, b"", gct=pal), UNSUPPORTED)
    # where two apply, the first in file order decides
    add("order_zero_screen_before_code_size", patch(6, b"\x00\x00", patch(hdr + 10, b"\x01")), INVALID)
    add("order_screen_limit_before_missing_image", patch(6, struct.pack("<HH", 16385, 16384))[:hdr], UNSUPPORTED)
    add("order_screen_limit_before_global_table_cut", patch(6, struct.pack("<HH", 16385, 16384))[:hdr - 3], UNSUPPORTED)
    add("order_no_colour_table_before_code_size", write_gif((12, 10), (0, 0), (12, 10), 1, stream), INVALID)
    add("order_code_size_before_sub_block_cut", bytes(patch(hdr + 10, b"\x09"))[:hdr + 10 + 1 + 5], UNSUPPORTED)
    add("order_sub_block_cut_before_expansion_bound", write_gif((12, 10), (0, 0), (700, 620), 2, long_stream[:40], gct=pal)[:-10], INVALID)
    add("order_expansion_bound_before_the_stream", write_gif((12, 10), (0, 0), (700, 620), 2, b"\xff" * 40, gct=pal), UNSUPPORTED)
    return out


def expansion_bound(m, n):
    return (ENTRIES - 1 - (1 << m)) * (8 * n // (m + 1))


def dump(directory):
    import os

    os.makedirs(directory, exist_ok=True)
    files = [(n, d) for n, d, _ in valid_files()] + [(n, d) for n, d, _ in damaged_files()] + list(pillow_files())
    for name, data in files:
        with open(os.path.join(directory, name + ".gif"), "wb") as f:
            f.write(data)
    return len(files)


if __name__ == "__main__":
    import sys

    print(dump(sys.argv[1]), "files")
