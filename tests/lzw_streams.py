"""Code-level TIFF LZW streams and byte-level PackBits streams for the device segment sink (DevSegSink, tiff_kernels.hip).  An LZW stream
is a list of codes with CLEAR / EOI markers placed on purpose; write_codes() packs it at the widths a reader is at, and the expected
bytes are the code list expanded here by the table rule, never the written stream decoded.  A PackBits stream is its bytes; expected
bytes by the format's three lines.  Each stream is the strip (or the strips) of a gray 8-bit TIFF.
valid_streams() -> (name, file, expected (h, w) uint8 pixels); refused_streams() -> (name, file); INFO[name]: facts for the corpus'
checks of itself.  Seeded, built once per process."""
import numpy as np

import tiff_util as tu

CLEAR, EOI = 256, 257
INFO = {}


def write_codes(codes):
    """the codes, most significant bit first, each at the width a reader has reached: early change, the reader's own entry counted
    before a Clear, 12 bits once the table is full"""
    w = tu._MsbWriter()
    nxt, width, have_prev = 258, 9, False
    for c in codes:
        w.put(c, width)
        if c == CLEAR:
            nxt, width, have_prev = 258, 9, False
        elif c != EOI:
            if have_prev and nxt < 4096:
                nxt += 1
                if nxt + 1 >= (1 << width) and width < 12:
                    width += 1
            have_prev = True
    return w.done()


def expand(codes, cap, bits=None):
    """the first cap bytes the codes stand for, or None where the rule refuses the stream: a Clear behind a Clear, a first code of 256
    or above, a code above the next free entry, an entry past 4095, EOI or the end of the codes before cap bytes.  bits: how many of
    the codes' bits the input holds (a cut stream).  -> (bytes or None, the highest `next` the table reached)"""
    table, nxt, prev, after_clear, out, top, used, width = {}, 258, None, False, bytearray(), 258, 0, 9
    for c in codes:
        if len(out) >= cap:
            break
        used += width
        if bits is not None and used > bits:
            return None, top
        if c == CLEAR:
            if after_clear:
                return None, top
            table, nxt, prev, after_clear, width = {}, 258, None, True, 9
            continue
        if c == EOI:
            return None, top
        if prev is None or c < 256:
            if c >= 256:
                return None, top
            s = bytes([c])
        elif c < nxt:
            s = table[c]
        elif c == nxt:
            s = prev + prev[:1]
        else:
            return None, top
        after_clear = False
        room = cap - len(out)
        out += s[:room]
        if len(s) >= room:
            break
        if prev is not None:
            if nxt >= 4096:
                return None, top
            table[nxt] = prev + s[:1]
            nxt += 1
            top = max(top, nxt)
            if nxt + 1 >= (1 << width) and width < 12:
                width += 1
        prev = s
    return (bytes(out) if len(out) >= cap else None), top


class Lz:
    """a code list under construction, with the table a reader would hold beside it"""

    def __init__(self, seed=0, first_clear=True):
        self.rng = np.random.default_rng(seed)
        self.codes, self.out = [CLEAR] if first_clear else [], bytearray()
        self._reset()

    def _reset(self):
        self.table, self.rev, self.nxt, self.prev = {}, {}, 258, None

    def clear(self):
        self.codes.append(CLEAR)
        self._reset()
        return self

    def string(self, c):
        return bytes([c]) if c < 256 else self.table[c] if c < self.nxt else self.prev + self.prev[:1]

    def emit(self, c):
        s = self.string(c)
        self.codes.append(c)
        self.out += s
        if self.prev is not None and self.nxt < 4096:
            self.table[self.nxt] = self.prev + s[:1]
            self.rev.setdefault(self.table[self.nxt], self.nxt)
            self.nxt += 1
        self.prev = s
        return self

    def kwkwk(self, n=1):
        for _ in range(n):
            self.emit(self.nxt)
        return self

    def lits(self, n):
        for _ in range(n):
            self.emit(int(self.rng.integers(0, 256)))
        return self

    def until_next(self, target):
        """random literals and short known strings until the next free entry is `target`"""
        if self.prev is None:
            self.lits(1)
        while self.nxt < target:
            self.emit(int(self.rng.integers(0, 256)) if self.rng.integers(0, 3) or self.nxt == 258 else int(self.rng.integers(258, self.nxt)))
        return self

    def long_string(self, n):
        """-> the code of an entry of n random bytes (made one byte longer at a time: string, then the literal that extends it)"""
        self.lits(2)
        c = self.nxt - 1
        while len(self.table[c]) < n:
            self.emit(c).lits(1)
            c = self.nxt - 1  # the string just sent plus that literal
        return c

    def feed(self, data):
        """the bytes as a greedy encoder would send them (the longest known string each time)"""
        i = 0
        while i < len(data):
            j = i + 1
            c = data[i]
            while j < len(data) and data[i:j + 1] in self.rev:
                j += 1
                c = self.rev[data[i:j]]
            if self.nxt >= 4094:
                self.clear()
                c, j = data[i], i + 1
            self.emit(c)
            i = j
        return self


def _shape(n):
    w = max(d for d in range(1, 257) if n % d == 0)
    return w, n // w


def tiff(segments, compression, w, rows_per_strip=None, h=None, lead=0):
    """a gray 8-bit file whose strips are the given compressed segments; lead: bytes in front of a single strip, so that its offset in
    the file is 8 + lead"""
    h = h or rows_per_strip * len(segments)
    override = {tu.T_COMPRESSION: (tu.SHORT, [compression])}  # (the writer is given nothing to compress: the segments replace its own)
    if lead:
        override.update({tu.T_STRIPOFFSETS: (tu.LONG, [8 + lead]), tu.T_STRIPBYTECOUNTS: (tu.LONG, [len(segments[0])])})
        segments = [bytes(lead) + segments[0]]
    return tu.encode(np.zeros((h, w), np.uint8), compression=1, rows_per_strip=rows_per_strip, segment_edit=lambda segs: list(segments), override=override)


_BUILT = {}


def _build():
    valid, refused = [], []

    def lzw(name, codes, cap, cut=0, garbage=b"", lead=0, **info):
        """one strip of cap bytes; cut: bytes taken off the end of the stream"""
        assert name not in INFO, name
        data = write_codes(codes)
        data = data[:len(data) - cut] + garbage
        want, top = expand(codes, cap, 8 * len(data) if cut else None)
        INFO[name] = dict(info, top=top, comp_len=len(data), offset=8 + lead, cap=cap, kind="lzw")
        w, h = _shape(cap)
        f = tiff([data], 5, w, h=h, lead=lead)
        if want is None:
            refused.append((name, f))
        else:
            valid.append((name, f, np.frombuffer(want, np.uint8).reshape(h, w)))
        return want

    def strips(name, kind, segs, w, rows):
        """many strips of rows x w bytes each: [(codes or PackBits bytes, expected bytes)]"""
        INFO[name] = dict(kind=kind, strips=len(segs), cap=w * rows)
        f = tiff([write_codes(s) if kind == "lzw" else s for s, _ in segs], 5 if kind == "lzw" else 32773, w, rows)
        valid.append((name, f, np.frombuffer(b"".join(e for _, e in segs), np.uint8).reshape(-1, w)))

    seeds = iter(range(100, 100000))
    new = lambda **kw: Lz(next(seeds), **kw)

    # ---- the end of the table
    z = new().until_next(4096)
    lzw("table_4095_then_clear", z.codes + [CLEAR] + new(first_clear=False).lits(300).codes + [EOI], len(z.out) + 300)
    lzw("refuse_table_4096_literal", z.codes + [65] + new(first_clear=False).lits(300).codes, len(z.out) + 301)
    lzw("table_4095_segment_ends_on_next_code", z.codes + [4095, 66, 67], len(z.out) + len(z.table[4095]))
    lzw("table_4095_segment_ends_inside_next_code", z.codes + [4095, 66], len(z.out) + 1)

    # ---- where a Clear falls
    lzw("clear_after_first_code", new().lits(1).clear().lits(40).codes + [EOI], 41)
    for n in (510, 511, 512, 1022, 1023, 1024, 2046, 2047, 2048):
        z = new().until_next(n).clear().until_next(300)
        lzw(f"clear_at_next_{n}", z.codes + [EOI], len(z.out))
    z = new().lits(50)
    lzw("clear_last_before_eoi", z.codes + [CLEAR, EOI], 50)
    z = new().lits(30).clear().lits(1).clear().lits(30)
    lzw("clear_literal_clear", z.codes + [EOI], 61)

    # ---- strings
    for n in (63, 64, 65, 127, 128, 129):
        z = new()
        c = z.long_string(n)
        z.emit(c)  # the string of n random bytes, then the code that is not in the table yet: that string and its first byte again
        assert len(z.prev) == n
        z.kwkwk().lits(2)
        lzw(f"kwkwk_prev_{n}", z.codes + [EOI], len(z.out), prev_len=n)
    z = new().lits(2).emit(258).kwkwk(5).lits(2).kwkwk(70).lits(1)
    lzw("kwkwk_on_kwkwk", z.codes + [EOI], len(z.out))
    z = new().lits(1).kwkwk(4095 - 258 + 1)
    assert len(z.string(4095)) == tu.LZW_MAX_STRING and z.nxt == 4096
    lzw("longest_string_3839", z.codes + [CLEAR] + new(first_clear=False).lits(9).codes + [EOI], len(z.out) + 9)
    for room in (1, 63, 64, 65):
        z = new()
        c = z.long_string(100)
        z.lits(5)
        lzw(f"cut_string_room_{room}", z.codes + [c, 65, EOI], len(z.out) + room)
        z = new()
        z.emit(z.long_string(100))
        lzw(f"cut_kwkwk_room_{room}", z.codes + [z.nxt, 65], len(z.out) + room)

    # ---- LDS or global memory, and the write-out
    text = bytes(np.random.default_rng(5).integers(0, 256, 1500).astype(np.uint8))
    for cap in (16383, 16384, 16385, 16400):
        z = new().feed((text * 12)[:cap])
        lzw(f"size_{cap}", z.codes + [EOI], cap)
    z = new()
    c = z.long_string(64)
    z.emit(c).emit(c)  # (the newest entry is now that string and its own first byte)
    lens_ = []
    while len(z.out) < 24000:  # each code is the entry that the code before it made: the bytes just written, and one more
        z.emit(z.nxt - 1 if len(z.prev) < 200 else c)
        lens_.append(len(z.prev))
    lzw("global_repeated_text", z.codes + [EOI], len(z.out), lengths=(min(lens_), max(lens_)))
    z = new().feed(bytes([77]) * 40000)
    lzw("global_one_byte_run", z.codes + [EOI], 40000)
    z = new().feed(text[:150] * 150)
    lzw("refuse_code_above_next_after_20000", z.codes + [4000, 65, 66], 22600, good_bytes=len(z.out), next_there=z.nxt, code=4000)
    for r in range(1, 16):
        segs = []
        for k in range(6):
            z = new().feed((text * 2)[k * 5:k * 5 + 16 + r])
            segs.append((z.codes + [EOI], bytes(z.out)))
        strips(f"strips_mod16_{r}", "lzw", segs, 16 + r, 1)
    segs = []
    for k in range(70):
        z = new().feed(bytes([k]) * 30 + text[k:k + 81])
        segs.append((z.codes + ([EOI] if k % 2 else []), bytes(z.out)))
    strips("lds_70_strips_of_111", "lzw", segs, 37, 3)

    # ---- bit reader
    for lead in (0, 1, 2, 3):
        for k in range(8):  # Clear and 14 .. 21 codes of 9 bits: 17, 18, 20, 21, 22, 23 ... bytes
            z = new().lits(14 + k)
            name = f"bits_offset_{lead}_len_{len(write_codes(z.codes)) % 4}"
            if name not in INFO:
                lzw(name, z.codes, 14 + k, lead=lead)
    z = new().lits(15)  # 16 codes of 9 bits: the last one ends on byte 18's last bit
    assert len(write_codes(z.codes)) * 8 == 9 * 16
    lzw("bits_last_code_ends_on_last_byte", z.codes, 15)
    lzw("refuse_cut_by_needed_byte", z.codes, 15, cut=1)
    z = new().until_next(600).lits(7)
    lzw("refuse_cut_by_needed_byte_10_bits", z.codes, len(z.out), cut=1)
    z = new().lits(40)
    lzw("refuse_eoi_one_code_early", z.codes[:-1] + [EOI, z.codes[-1]], 40)
    lzw("full_then_eoi", z.codes + [EOI], 40)
    lzw("full_without_eoi", z.codes, 40)
    lzw("full_then_garbage", z.codes, 40, garbage=b"\xff\x00\xff\xff\xff")
    lzw("full_then_eoi_and_garbage", z.codes + [EOI], 40, garbage=b"\x80\x00\x01")

    # ---- the rule's bounds
    z = new().lits(5)
    lzw("code_equal_next", z.codes + [z.nxt, 65], len(z.out) + 3)
    lzw("refuse_code_next_plus_1", z.codes + [z.nxt + 1, 65], len(z.out) + 3)
    lzw("first_code_255", [CLEAR, 255, 255, 258], 4)
    lzw("refuse_first_code_258", [CLEAR, 258, 65, 66, 67], 4)

    # ---- random code lists
    for k in range(120):
        r = np.random.default_rng(3000 + k)
        z = Lz(4000 + k)
        bad, late = None, 4096 - int(r.integers(0, 3))
        for _ in range(int(r.integers(4200, 5000) if k % 10 == 0 else r.integers(20, 700))):
            c = int(r.integers(0, 100))
            if z.nxt >= late:  # a late Clear: at the table's last entries, 4096 being the last legal moment
                z.clear()
                late = 4096 - int(r.integers(0, 3))
            elif z.prev is None or c < 30:
                z.lits(1)
            elif c < 55:
                z.kwkwk()
            elif c < 95:
                z.emit(int(r.integers(258, z.nxt)) if z.nxt > 258 and r.integers(0, 2) else z.nxt - 1 if z.nxt > 258 else 65)
            elif c < 97 and k % 10:
                z.clear()
            elif c == 99 and k % 4 == 0 and bad is None:  # one illegal code: above the next entry, EOI, or a second Clear
                bad = len(z.codes)
                z.codes += [[z.nxt + 1 + int(r.integers(0, 3)), EOI][int(r.integers(0, 2))]] if z.codes[-1] != CLEAR else [CLEAR]
                break
        cap = len(z.out) + (int(r.integers(1, 40)) if bad is not None else -int(r.integers(0, min(60, len(z.out) - 1))) if k % 3 else 0)
        lzw(f"random_{k:03d}", z.codes + ([EOI] if k % 2 and bad is None else []), cap)

    # ---- PackBits
    def pack(name, data, cap):
        assert name not in INFO, name
        want = tu_expand_packbits(data, cap)
        INFO[name] = dict(kind="packbits", cap=cap, controls=set(packbits_controls(data, cap)), tokens=len(list(packbits_controls(data, cap))))
        w, h = _shape(cap)
        f = tiff([data], 32773, w, h=h)
        if want is None:
            refused.append((name, f))
        else:
            valid.append((name, f, np.frombuffer(want, np.uint8).reshape(h, w)))

    r = np.random.default_rng(9)
    rb = lambda n: bytes(r.integers(0, 256, n).astype(np.uint8))
    lit = lambda n: bytes([n - 1]) + rb(n)
    run = lambda n, b=None: bytes([257 - n, int(r.integers(0, 256)) if b is None else b])
    every = b"".join(lit(c + 1) if c < 128 else bytes([128]) if c == 128 else run(257 - c) for c in r.permutation(256))
    pack("pb_every_control_byte", every, sum(c + 1 if c < 128 else 0 if c == 128 else 257 - c for c in range(256)))
    for n in (1, 2, 63, 64, 65, 127, 128):
        pack(f"pb_literal_{n}", lit(3) + lit(n) + run(4), n + 7)
        pack(f"pb_run_{n}", lit(3) + run(n) + lit(4), n + 7) if n > 1 else pack("pb_run_2_twice", run(2) + run(2) + lit(1), 5)
        pack(f"pb_literal_{n}_last", run(5) + lit(n), n + 5)
        pack(f"pb_run_{n}_last", lit(5) + run(max(n, 2)), max(n, 2) + 5)
    pack("pb_run_crosses_end", lit(10) + run(100), 50)
    pack("pb_literal_crosses_end_input_holds_it", lit(10) + lit(100), 50)
    cut = lit(10) + lit(100)
    pack("refuse_pb_literal_crosses_end_input_ends_inside", cut[:-30], 50)
    pack("refuse_pb_input_ends_inside_literal", lit(10) + lit(100)[:-1], 110)
    pack("refuse_pb_input_ends_after_run_count", lit(10) + bytes([0x90]), 50)
    pack("refuse_pb_input_ends_early", lit(10) + run(20), 31)
    pack("pb_noops_at_start", bytes([128]) * 128 + lit(20) + run(20), 40)
    pack("pb_noops_in_middle", lit(20) + bytes([128]) * 128 + run(20), 40)
    pack("pb_noops_at_end", lit(20) + run(20) + bytes([128]) * 128, 40)
    pack("pb_trailing_garbage", lit(20) + run(20) + b"\x05\x01", 40)
    many = b"".join(lit(1) if k % 3 else run(2) for k in range(1500))
    pack("pb_1500_short_tokens", many, sum(1 if k % 3 else 2 for k in range(1500)))
    pack("pb_one_byte_literal", lit(1), 1)
    pack("pb_one_byte_run", run(128), 1)
    segs = [((lit(1) if k % 2 else run(2 + k % 5))[:2], None) for k in range(40)]
    strips("pb_40_strips_of_1_byte", "packbits", [(s, tu_expand_packbits(s, 1)) for s, _ in segs], 1, 1)
    for r16 in (1, 7, 15):
        segs = []
        for k in range(66):
            s = lit(5 + k % 9) + run(100) + lit(30)
            segs.append((s, tu_expand_packbits(s, 32 + r16)))
        strips(f"pb_66_strips_mod16_{r16}", "packbits", segs, 32 + r16, 1)
    for k in range(60):
        rr = np.random.default_rng(600 + k)
        data = bytearray()
        for _ in range(int(rr.integers(1, 60))):
            c = int(rr.choice([0, 1, 62, 63, 64, 126, 127, 128, 129, 130, 192, 193, 194, 254, 255, int(rr.integers(0, 256))]))
            data.append(c)
            data += bytes(rr.integers(0, 256, c + 1 if c < 128 else 0 if c == 128 else 1).astype(np.uint8))
        full = len(tu_expand_packbits(bytes(data), 0, whole=True))
        if k % 5 == 4:
            data = data[:len(data) - int(rr.integers(1, 4))]
        cap = max(1, full + int(rr.integers(-40, 1)) if k % 5 != 3 else full + int(rr.integers(1, 9)))
        pack(f"pb_random_{k:02d}", bytes(data), cap)
    return valid, refused


def packbits_controls(data, cap):
    """the control bytes a reader meets before the segment is full"""
    pos, n = 0, 0
    while n < cap and pos < len(data):
        c = data[pos]
        yield c
        pos += 1 + (c + 1 if c < 128 else 0 if c == 128 else 1)
        n += c + 1 if c < 128 else 0 if c == 128 else 257 - c


def tu_expand_packbits(data, cap, whole=False):
    """cap bytes by the format's three lines, or None where the rule refuses: the input ends before the segment is full, inside a
    literal, or behind a run's count.  whole: everything the input holds, however much"""
    out, pos = bytearray(), 0
    while (pos < len(data)) if whole else (len(out) < cap):
        if pos >= len(data):
            return None
        c = data[pos]
        pos += 1
        if c < 128:
            if len(data) - pos < c + 1:
                return out if whole else None
            out += data[pos:pos + c + 1]
            pos += c + 1
        elif c > 128:
            if pos >= len(data):
                return out if whole else None
            out += data[pos:pos + 1] * (257 - c)
            pos += 1
    return out if whole else bytes(out[:cap])


def _all():
    if not _BUILT:
        _BUILT["valid"], _BUILT["refused"] = _build()
    return _BUILT


def valid_streams():
    return _all()["valid"]


def refused_streams():
    return _all()["refused"]


GROUPS = {
    "table_and_clears": ("table_", "clear_", "code_", "first_code_", "full_", "bits_"),
    "strings": ("kwkwk_", "cut_", "longest_"),
    "split": ("size_", "global_", "strips_", "lds_"),
    "random": ("random_",),
    "packbits": ("pb_",),
}
FAMILIES = ["table_4095_then_clear", "table_4095_segment_ends_on_next_code", "clear_after_first_code", "clear_last_before_eoi", "clear_literal_clear"] + \
    [f"clear_at_next_{n}" for n in (510, 511, 512, 1022, 1023, 1024, 2046, 2047, 2048)] + [f"kwkwk_prev_{n}" for n in (63, 64, 65, 127, 128, 129)] + \
    ["kwkwk_on_kwkwk", "longest_string_3839"] + [f"cut_{k}_room_{r}" for k in ("string", "kwkwk") for r in (1, 63, 64, 65)] + \
    [f"size_{n}" for n in (16383, 16384, 16385, 16400)] + [f"strips_mod16_{r}" for r in range(1, 16)] + ["global_repeated_text", "global_one_byte_run", "lds_70_strips"] + \
    [f"bits_offset_{o}_len_{n}" for o in range(4) for n in range(4)] + ["bits_last_code_ends_on_last_byte", "full_then_eoi", "full_without_eoi", "full_then_garbage",
                                                                       "code_equal_next", "first_code_255", "random_"] + \
    ["pb_every_control_byte"] + [f"pb_{k}_{n}" for k in ("literal", "run") for n in (2, 63, 64, 65, 127, 128)] + ["pb_literal_1", "pb_run_crosses_end",
                                                                                                                    "pb_literal_crosses_end_input_holds_it", "pb_noops_at_start",
                                                                                                                    "pb_noops_in_middle", "pb_noops_at_end", "pb_1500_short_tokens",
                                                                                                                    "pb_40_strips_of_1_byte", "pb_random_"]
REFUSED = ["refuse_table_4096_literal", "refuse_cut_by_needed_byte", "refuse_eoi_one_code_early", "refuse_code_next_plus_1", "refuse_first_code_258",
           "refuse_code_above_next_after_20000", "refuse_pb_literal_crosses_end_input_ends_inside", "refuse_pb_input_ends_after_run_count"]
