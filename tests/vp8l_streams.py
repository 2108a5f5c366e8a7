"""Token-level VP8L streams for the device pixel sink (DevPixelSink, webp_kernels.hip): every stream is a list of tokens placed on
purpose (literal, colour-cache slot, copy of a chosen length and distance) and written by webp_util's writer; the expected pixels are
the tokens expanded here in plain Python, never the written file decoded, so that the writer and every reader check each other.
valid_streams() -> (name, file, expected ARGB pixels as an (h, w) uint32 array); refused_streams() -> (name, file).  TOKENS[name] =
(tokens, xsize, cache bits), BITS[name] = (bit_start, bit_end), SYMBOLS[name][(group, alphabet)] = (symbols in use, longest code) and
FACTS[name] (counts of a placement that a loop makes) for the corpus' checks of itself.  Seeded, built once per process."""
import numpy as np

import webp_util as wu

MUL = 0x1e35a7bd
RUNS = (1, 63, 64, 65, 127, 128, 129)
LENS = (1, 2, 63, 64, 65, 127, 128, 129, 4096)
DISTS = (1, 2, 3, 63, 64, 65)
TOKENS, BITS, SYMBOLS, FACTS = {}, {}, {}, {}


def key(v, bits):
    return ((v * MUL) & 0xffffffff) >> (32 - bits)


def colliding(rng, bits, n=2, member=None, slot=None):
    """n distinct ARGB values of one cache slot, largest first (member: one of them, given)"""
    slot = key(member, bits) if member is not None else int(rng.integers(0, 1 << bits)) if slot is None else slot
    got = {member} if member is not None else set()
    while len(got) < n:
        v = int(rng.integers(0, 1 << 32))
        if key(v, bits) == slot:
            got.add(v)
    return sorted(got, reverse=True)


class Stream:
    """tokens and, beside them, the pixels they stand for: the expansion every reader is compared with"""

    def __init__(self, seed, cache_bits=0, xsize=None, palette=None):
        self.rng = np.random.default_rng(seed)
        self.cb, self.w, self.t, self.px = cache_bits, xsize, [], []
        self.cache = [0] * (1 << cache_bits) if cache_bits else None
        self.pal = palette  # literal values are drawn from it (few symbols: short codes)
        self.legal = True

    @property
    def n(self):
        return len(self.px)

    def _put(self, v):
        self.px.append(v)
        if self.cache is not None:
            self.cache[key(v, self.cb)] = v

    def lit(self, v=None, avoid=None):
        """a literal: v, or one of the palette, or (avoid: cache slots it must not fall into) any value outside those slots"""
        while v is None:
            c = int(self.pal[int(self.rng.integers(0, len(self.pal)))]) if self.pal is not None and not avoid else int(self.rng.integers(0, 1 << 32))
            if not (avoid and self.cb and key(c, self.cb) in avoid):
                v = c
        self.t.append(("lit", v))
        self._put(v)
        return self

    def lits(self, k, avoid=None):
        for _ in range(k):
            self.lit(avoid=avoid)
        return self

    def hit(self, slot):
        assert self.cb and 0 <= slot < 1 << self.cb
        self.t.append(("cache", slot))
        self._put(self.cache[slot])
        return self

    def ref(self, length, dist=None, code=None):
        """a copy by its distance (written as the code dist + 120) or by a plane code (the stream's xsize must be set)"""
        if code is None:
            code = dist + 120
        else:
            dist = wu.plane_distance(self.w, code)
        self.t.append(("ref", length, code))
        if dist > self.n:
            self.legal = False
            return self
        for i in range(length):
            self._put(self.px[-dist])
        return self

    def to_residue(self, r):
        """literals and one copy so that the next pixel's position is r mod 64, a copy being the last token"""
        if not self.n:
            self.lits(3)
        k = (r - self.n - 2) % 64 + 2
        return self.ref(k, min(self.n, 2))


def _shape(n, w=None):
    if w is not None:
        assert n % w == 0, (n, w)
        return w, n // w
    cand = [d for d in range(1, 201) if n % d == 0 and n // d <= 16384]
    assert cand, n
    w = cand[len(cand) // 2 + n % (len(cand) - len(cand) // 2)]  # (one of the wider shapes that the pixels fill)
    return w, n // w


def deep_lens(want=None):
    """a lens hook (webp_util.write_pixels): alphabet `want` (or every alphabet) gets a code of depth 15 over 16 symbols, the two codes of
    15 bits going to the rarest symbols in use"""
    def f(g, k, hist, ln):
        used = sorted((s for s, c in enumerate(hist) if c), key=lambda s: (hist[s], s))
        if (want is not None and k != want) or len(used) < 2:
            return ln
        assert len(used) <= 16, (k, len(used))
        fill = [s for s in range(len(hist)) if not hist[s]][:16 - len(used)]
        order = used[:2] + fill + used[2:]  # depth 15, 15, 14, 13, ... 1
        out = [0] * len(hist)
        for i, s in enumerate(order):
            out[s] = 15 if i < 2 else 16 - i
        return out
    return f


def _file(name, s, w=None, shape=None, info=None, **kw):
    """the stream as a file: of the given shape, or of a shape that its pixels fill"""
    w, h = shape or _shape(s.n, s.w if w is None else w)
    info = {} if info is None else info
    lens, seen = kw.pop("lens", None), {}

    def record(g, k, hist, ln):
        ln = lens(g, k, hist, ln) if lens else ln
        seen[(g, k)] = (sum(1 for c in hist if c), max(l for l, c in zip(ln, hist) if c) if any(hist) else 0)  # (of the symbols in use)
        return ln
    data = wu.encode(np.zeros((h, w, 4), np.uint8), tokens=s.t, cache_bits=s.cb, alpha=True, info=info, lens=record, **kw)
    SYMBOLS[name] = seen
    BITS[name] = (info["bit_start"], info["bit_end"])
    TOKENS[name] = (s.t, w, s.cb)
    return data, w, h


def expected_image(argb):
    """(h, w, 4) RGBA uint8 of an (h, w) ARGB array: what a decoder returns for these files (the header's alpha bit is set)"""
    a = np.asarray(argb, np.uint32)
    return np.stack([(a >> 16) & 255, (a >> 8) & 255, a & 255, a >> 24], axis=-1).astype(np.uint8)


_BUILT = {}


def _build():
    valid, refused = [], []

    def add(name, s, transform=None, **kw):
        assert s.legal and name not in TOKENS, name
        data, w, h = _file(name, s, **kw)
        px = np.array(s.px, np.uint32).reshape(h, w)
        if transform == "green":
            g = (px >> 8) & 255
            px = (px & 0xff00ff00) | (((px & 0x00ff00ff) + (g << 16 | g)) & 0x00ff00ff)
        valid.append((name, data, px))
        return data

    def refuse(name, s, w, h, **kw):
        data, _, _ = _file(name, s, shape=(w, h), **kw)
        refused.append((name, data))

    seed = iter(range(1000, 100000))
    pal = lambda r, n=24: r.integers(0, 1 << 32, n, dtype=np.uint64)
    new = lambda cb=0, xsize=None, p=True: (lambda sd: Stream(sd, cb, xsize, pal(np.random.default_rng(sd)) if p else None))(next(seed))

    # ---- pending literals and flush
    for run in RUNS:
        for r in (0, 1, 63):
            s = new().to_residue(r).lits(run).ref(5, 2).lits(2)
            add(f"run_{run}_at_{r}", s)
    for k in (0, 1, 63, 64):
        add(f"tail_{k}_literals", new().lits(7).ref(30, 3).lits(k))
    for n in (64, 65, 127, 128, 129, 191):
        add(f"literals_only_{n}", new().lits(n))

    # ---- a copy reads what was just stored
    for d in DISTS:
        for ln in LENS:
            s = new().to_residue((d * 7 + ln) % 64).lits(max(d, 2)).ref(ln, d).lits(3)
            add(f"copy_d{d}_l{ln}", s)
    for ln in (63, 64, 65, 127, 128, 129, 4096):  # dist >= len over literals wider than the copy
        s = new().lits(ln + 1).ref(ln, ln + 1).lit() if ln < 200 else None
        if ln == 4096:  # (a source of 4096 literals would be most of the file: the copy before it provides them)
            s = new().lits(70).ref(4096, 70).ref(4096, 4096).lits(1)
        add(f"copy_far_l{ln}", s)
    for first, d2, l2 in ((65, 65, 65), (65, 64, 129), (130, 1, 64), (200, 199, 4096), (4096, 4096, 4096), (129, 128, 127)):
        s = new().to_residue(first % 3).lits(4).ref(first, 3).ref(l2, d2).lits(2)
        add(f"copy_of_copy_{first}_d{d2}_l{l2}", s)
    for ln in LENS:
        add(f"copy_to_last_l{ln}", new().lits(5).ref(ln, 4))
    for w in (1, 2, 3):
        s = new(xsize=w).lits(3).ref(4096, 3).ref(4096, 2).lits(5).ref(4096, 7)
        s.lits(-s.n % w)
        add(f"narrow_{w}_copies_4096", s)
        clamp = [c for c in range(1, 121) if wu.PLANE[c - 1][0] + wu.PLANE[c - 1][1] * w < 1]
        assert clamp
        s = new(xsize=w).lits(4)
        for c in clamp:
            s.ref(2, code=c).lit()
        s.lits(-s.n % w)
        add(f"plane_clamp_w{w}", s)
    add("distance_code_121", new().lits(2).ref(70, 1).lit().ref(3, 1))
    # the largest distance the alphabet reaches (symbol 39, 18 extra bits of ones), behind a literal of four 15-bit codes and a length
    # with 10 extra bits; every alphabet of the file 15 bits deep
    top = (1 << 20) - 120
    s = Stream(next(seed), 0, None, pal(np.random.default_rng(1), 6)).lits(16)
    while s.n < top - 41:
        s.ref(min(4096, top - 41 - s.n), 16)
    s.lits(40)
    rare = int(s.rng.integers(0, 1 << 32))
    s.lit(rare)
    assert s.n == top
    s.ref(4095, top)  # from the first pixel: code 2^20, symbol 39 with all 18 extra bits set; 4095: symbol 23 and 10 extra bits
    assert wu._prefix_encode(top + 120) == (39, (1 << 18) - 1, 18) and wu._prefix_encode(4095)[2] == 10
    s.lits(200 - s.n % 200)
    chosen, deep = {}, deep_lens()
    add("dist_max_lit15_copy28", s, w=200, lens=lambda g, k, hist, ln: chosen.setdefault(k, deep(g, k, hist, ln)))
    assert [chosen[k][(rare >> sh) & 255] for k, sh in enumerate((8, 16, 0, 24))] == [15] * 4 and chosen[4][39] + chosen[0][256 + 23] >= 16

    # ---- colour cache
    for cb in (1, 2, 6, 10, 11):
        r = np.random.default_rng(cb)
        for gap, tag in ((1, "same_step"), (70, "other_step")):
            for pair in ("random", "ones", "zero"):
                big, small = colliding(r, cb, 2, {"random": None, "ones": 0xffffffff, "zero": 0}[pair])
                slot = key(big, cb)
                s = new(cb).to_residue(5 * cb % 64).lit(big).lits(gap - 1, avoid={slot}).lit(small).lits(3, avoid={slot})
                s.ref(gap + 4, gap + 4).hit(slot).lits(2)
                assert s.px[-3] == small
                add(f"cache{cb}_copy_collision_{tag}_{pair}", s)
        # a pending (not yet flushed) literal and the copy behind it: the copy brings the smaller value later
        big, small = colliding(r, cb)
        slot = key(big, cb)
        s = new(cb).lit(small).lits(9, avoid={slot}).to_residue(3)
        at = s.n
        s.lit(big)
        s.ref(3, s.n)  # from pixel 0: small, then two others; `big` is pending in its lane when the copy enters `small`
        s.hit(slot).lits(2)
        assert s.px[at + 1] == small and s.px[at + 4] == small, (cb, at)
        add(f"cache{cb}_pending_then_copy", s)
        # who entered the slot last: a literal of another lane of the same block, a copy, a cache token, nobody
        a, b = colliding(r, cb)
        slot = key(a, cb)
        s = new(cb).to_residue(10).lit(a).lits(20, avoid={slot}).hit(slot).lits(2)
        add(f"cache{cb}_hit_literal_other_lane", s)
        s = new(cb).lit(a).lits(5, avoid={slot}).lit(b).ref(70, 7).hit(slot).lits(2)
        add(f"cache{cb}_hit_copy", s)
        s = new(cb).lit(a).hit(slot).lits(66, avoid={slot}).hit(slot).hit(slot).lits(2)
        add(f"cache{cb}_hit_cache_token", s)
        s = new(cb)
        empty = int(s.rng.integers(0, 1 << cb))
        s.lits(3, avoid={empty}).hit(empty).lits(70, avoid={empty}).hit(empty).lits(2, avoid={empty})
        assert s.px[3] == 0
        add(f"cache{cb}_hit_nothing", s)
        s = new(cb).to_residue(40).lits(4)
        for k in range(70):
            s.hit(key(s.px[int(s.rng.integers(0, s.n))], cb))
        add(f"cache{cb}_run_of_70_tokens", s.lits(2))
    vals = [0xffffffff, 0] + [int(v) for v in np.random.default_rng(5).integers(0, 1 << 32, 6)]
    s = Stream(77, 1, None, np.array(vals, np.uint64)).lits(4)
    for k in range(900):
        c = int(s.rng.integers(0, 10))
        if c < 4:
            s.lit()
        elif c < 7:
            s.hit(int(s.rng.integers(0, 2)))
        else:
            s.ref(int(s.rng.choice([1, 2, 3, 63, 64, 65, 70])), int(s.rng.integers(1, min(s.n, 130) + 1)))
    add("cache1_random_mix", s)

    # ---- bit reader and codes
    found, tries = {}, 0
    while len(found) < 32 and tries < 3000:
        tries += 1
        r = np.random.default_rng(50000 + tries)
        w, h = int(r.integers(1, 12)), int(r.integers(1, 9))
        cb = int(r.choice([0, 0, 1, 4, 7, 11]))
        nt = int(r.integers(0, 3))
        trs = [[("green",)], [("cross", 2 + int(r.integers(0, 3)), np.zeros(3, np.int64))]][int(r.integers(0, 2))] if nt == 1 else \
            [("green",), ("cross", 2, np.zeros(3, np.int64))][::int(r.choice([1, -1]))] if nt == 2 else []
        meta = [None, 2, 3][int(r.integers(0, 3))]
        ng = 1 if meta is None else 1 + int(r.integers(0, min(3, wu.sub(w, meta) * wu.sub(h, meta))))
        s = Stream(60000 + tries, cb, w, r.integers(0, 1 << 32, int(r.integers(1, 6)), dtype=np.uint64)).lits(w * h)
        kw = dict(transforms=trs, meta_bits=meta, n_groups=ng, code_kw=dict(simple=bool(r.integers(0, 2))))
        info = {}
        wu.encode(np.zeros((h, w, 4), np.uint8), tokens=s.t, cache_bits=cb, alpha=True, info=info, **kw)
        res = info["bit_start"] % 32
        if res not in found:
            found[res] = (s, kw, any(t[0] == "green" for t in trs))
    for res in sorted(found):
        s, kw, green = found[res]
        add(f"bitstart_{res:02d}", s, transform="green" if green else None, **kw)
        assert BITS[f"bitstart_{res:02d}"][0] % 32 == res
    for k, alpha in enumerate(("green", "red", "blue", "alpha", "distance")):
        shift = {"green": 8, "red": 16, "blue": 0, "alpha": 24}.get(alpha)

        def content(n_sym, k=k, shift=shift):
            """a stream in which alphabet k uses n_sym symbols (16: for the code of depth 15) and the others a few"""
            s = new(p=False)
            base = [int(v) for v in s.rng.integers(0, 1 << 32, 5)]
            for j in range(400):
                v = base[int(s.rng.integers(0, 5))]
                if shift is not None:
                    # symbol j of n_sym, more often the lower ones (so that the rarest are used, though rarely)
                    z = min(n_sym - 1, int(s.rng.geometric(0.35)) - 1) if j >= n_sym else j
                    v = (v & ~(255 << shift)) | ((z * 13 + 1) << shift)
                    s.lit(v)
                    if j % 9 == 8 and k != 0:  # (length symbols belong to the green alphabet: its streams are literals only)
                        s.ref(3, 2)
                else:
                    if not s.n:
                        s.w = 7
                        s.lits(77)
                    s.lit(v)
                    codes = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193][:n_sym]  # the first code of distance symbols 0 .. 15
                    s.ref(2, code=codes[min(n_sym - 1, int(s.rng.geometric(0.35)) - 1) if j >= n_sym else j])
            for _ in range(-s.n % 7 if s.w else 0):
                s.lit(base[0])
            return s
        add(f"code_single_{alpha}", content(1))
        add(f"code_two_{alpha}", content(2))
        add(f"code_deep_{alpha}", content(16), lens=deep_lens(k))
    s = new(p=False)
    s.lits(1)
    s.pal = np.array([s.px[0]], np.uint64)
    add("zero_bits_one_literal", s.lits(149))
    s = new(3)
    for _ in range(96):
        s.hit(0)  # nothing but one cache symbol: every code has one symbol, every pixel is 0x00000000
    add("zero_bits_cache_tokens_only", s)
    # the last symbol ends on the chunk's last bit; the same stream cut by that byte is refused
    two = np.array([0x01010101, 0xfefefefe], np.uint64)  # channels of two symbols each: four bits a literal
    for extra in range(40):  # (a third green value now and then: its code and that of 0xfe take two bits)
        s = Stream(90, 0, None, two).lit(0x01010101).lit(0xfefefefe).lits(40 + extra // 5)
        for _ in range(extra % 5):
            s.lit(0x01013301)
        s.lit(0xfefefefe)
        info = {}
        w, h = _shape(s.n)
        wu.encode(np.zeros((h, w, 4), np.uint8), tokens=s.t, alpha=True, info=info)
        if info["bit_end"] % 8 == 0:
            break
    assert info["bit_end"] % 8 == 0
    data = add("endbit_exact", s)
    n_chunk = info["bit_end"] // 8
    assert int.from_bytes(data[16:20], "little") == n_chunk
    refused.append(("refuse_cut_needed_byte", wu._resize_chunk(data, n_chunk - 1)))
    # a tail of zero bits: cut, the device's zero-padded copy decodes the same legal symbols; only out_of_bits refuses it
    # The refused cuts keep an even count of bytes: behind an odd one the container's pad byte follows, and libwebp reads on through
    # whatever the file holds behind the chunk (PAD_BYTE_CASE, include/rupphash.h)
    for extra in (0, 2):
        s = Stream(99, 0, None, two).lit(0x01010101).lit(0xfefefefe).lits(41)
        s.pal = np.array([0x01010101], np.uint64)
        s.lits(21 + extra)  # 84 or 92 zero bits
        info = {}
        name = "zero_tail" if not extra else "zero_tail_longer"
        data = add(name, s, info=info)
        n_chunk = (info["bit_end"] + 7) // 8
        assert data[20 + n_chunk - 6:20 + n_chunk] == bytes(6) and int.from_bytes(data[16:20], "little") == n_chunk
        if n_chunk % 2:
            refused.append(("refuse_cut_zero_tail_1", wu._resize_chunk(data, n_chunk - 1)))
            refused.append(("refuse_cut_zero_tail_5", wu._resize_chunk(data, n_chunk - 5)))
        else:
            _BUILT["pad_byte_case"] = (name, wu._resize_chunk(data, n_chunk - 1))

    # ---- groups
    for cb in (0, 4):
        for single in (False, True):
            w, h = 22, 20
            bw_, bh_ = wu.sub(w, 2), wu.sub(h, 2)
            r = np.random.default_rng(cb + 2 * single)
            ent = r.integers(0, 4, bw_ * bh_)
            ent[:4] = np.arange(4)
            s = Stream(300 + cb + single, cb, w, pal(r, 10))
            fixed = int(r.integers(0, 1 << 32))
            after_copy = 0  # tokens read from group 3 straight behind a copy that began in another group
            while s.n < w * h:
                y, x = divmod(s.n, w)
                g = int(ent[(y >> 2) * bw_ + (x >> 2)])
                left = w * h - s.n
                c = int(s.rng.integers(0, 10))
                after_copy += g == 3 and bool(s.t) and s.t[-1][0] == "ref"
                if single and g == 3:
                    s.lit(fixed)
                elif c < 4 or s.n < 8 or left < 3:
                    s.lit()
                elif c < 6 and cb:
                    s.hit(key(s.px[int(s.rng.integers(0, s.n))], cb))
                else:
                    s.ref(min(left, int(s.rng.choice([3, 4, 5, 9, 23, 45, 70]))), int(s.rng.integers(1, min(s.n, 70) + 1)))
            name = f"groups_cache{cb}_{'single_symbol_group' if single else 'copies_cross_blocks'}"
            add(name, s, meta_bits=2, n_groups=4, ent_map=ent)
            FACTS[name] = dict(tokens_of_group_3_behind_a_copy=int(after_copy))

    # ---- the rule's bounds, each with its sibling on the allowed side
    add("edge_dist_equal", new().lits(37).ref(9, 37).lits(4))
    b = new().lits(37).ref(9, 38).lits(4)
    refuse("refuse_dist_plus_1", b, 10, 5)
    add("edge_len_equal", new().lits(37).ref(13, 20), w=10)
    refuse("refuse_len_plus_1", new().lits(37).ref(14, 20), 10, 5)
    s = new().lits(50)
    while s.n < 10200:
        s.ref(127, 50)
    s.lits(5)
    n0 = s.n
    s.ref(9, n0 + 1)
    assert not s.legal
    refuse("refuse_dist_plus_1_after_10000", s, 97, -(-(n0 + 40) // 97))
    good = new().lits(50)
    while good.n < 10200:
        good.ref(127, 50)
    good.lits(5)
    good.ref(9, good.n).lits(-good.n % 97)
    add("edge_dist_equal_after_10000", good, w=97)

    # ---- random token sequences
    for k in range(110):
        r = np.random.default_rng(7000 + k)
        cb = k % 12
        ng = 1 + k % 9
        w = int(r.integers(1, 201))
        meta = None if ng == 1 else int(r.integers(2, 5))
        target = int(r.integers(300, 5000))
        h = -(-target // w)
        if meta is not None:
            while wu.sub(w, meta) * wu.sub(h, meta) < ng:
                h += 1 << meta
        members = [0, 0xffffffff]
        if cb:
            members += colliding(r, cb, 3) + colliding(r, cb, 2, 0) + colliding(r, cb, 2, 0xffffffff)
        s = Stream(8000 + k, cb, w, np.array(members + [int(v) for v in r.integers(0, 1 << 32, 8)], np.uint64)).lits(2)
        while s.n < w * h:
            left = w * h - s.n
            c = int(r.integers(0, 10))
            if c < 3:
                s.lit()
            elif c < 5 and cb:
                s.hit(key(int(s.pal[int(r.integers(0, len(s.pal)))]), cb))
            else:
                ln = int(r.choice(LENS[:-1] if r.integers(0, 8) else LENS))
                d = int(r.choice(DISTS + (127, 128, 129, s.n)))
                s.ref(min(ln, left), min(d, s.n))
        kw = {}
        if meta is not None:
            blocks = wu.sub(w, meta) * wu.sub(h, meta)
            ent = r.integers(0, ng, blocks)
            ent[r.permutation(blocks)[:ng]] = np.arange(ng)
            kw = dict(meta_bits=meta, n_groups=ng, ent_map=ent)
        add(f"random_{k:03d}_cache{cb}_groups{ng}", s, **kw)
    return valid, refused


def _all():
    if not _BUILT:
        _BUILT["valid"], _BUILT["refused"] = _build()
    return _BUILT


def pad_byte_case():
    """(name of the valid stream, that file with its chunk cut by its last, all-zero byte to an odd size): refused here, while libwebp
    reads the pad byte behind the chunk in its place"""
    return _all()["pad_byte_case"]


def valid_streams():
    return _all()["valid"]


def refused_streams():
    return _all()["refused"]


# the streams by what they aim at: each GPU test takes one group; FAMILIES below is what the corpus must hold
GROUPS = {
    "flush": ("run_", "tail_", "literals_only_"),
    "copies": ("copy_", "narrow_", "plane_clamp_", "distance_code_121", "edge_"),
    "cache": ("cache",),
    "codes": ("bitstart_", "code_", "zero_", "endbit_", "groups_"),
    "far": ("dist_max_",),
    "random_a": tuple(f"random_{k:03d}" for k in range(0, 55)),
    "random_b": tuple(f"random_{k:03d}" for k in range(55, 110)),
}
FAMILIES = [f"run_{n}_at_{r}" for n in RUNS for r in (0, 1, 63)] + [f"tail_{k}_literals" for k in (0, 1, 63, 64)] + \
    [f"literals_only_{n}" for n in (64, 65, 127)] + [f"copy_d{d}_l{ln}" for d in DISTS for ln in LENS] + ["copy_far_l4096", "copy_of_copy_", "copy_to_last_l4096"] + \
    [f"narrow_{w}_copies_4096" for w in (1, 2, 3)] + [f"plane_clamp_w{w}" for w in (1, 2, 3)] + ["distance_code_121", "dist_max_lit15_copy28"] + \
    [f"cache{cb}_{what}" for cb in (1, 2, 6, 10, 11) for what in (
        "copy_collision_same_step_random", "copy_collision_other_step_random", "copy_collision_same_step_ones", "copy_collision_other_step_zero", "pending_then_copy",
        "hit_literal_other_lane", "hit_copy", "hit_cache_token", "hit_nothing", "run_of_70_tokens")] + ["cache1_random_mix"] + \
    [f"code_{d}_{a}" for d in ("single", "two", "deep") for a in ("green", "red", "blue", "alpha", "distance")] + \
    ["bitstart_00", "bitstart_01", "bitstart_31", "zero_bits_one_literal", "zero_bits_cache_tokens_only", "endbit_exact", "zero_tail",
     "groups_cache0_copies_cross_blocks", "groups_cache4_copies_cross_blocks", "groups_cache0_single_symbol_group", "groups_cache4_single_symbol_group",
     "edge_dist_equal", "edge_len_equal", "edge_dist_equal_after_10000", "random_"]
REFUSED = ["refuse_dist_plus_1", "refuse_len_plus_1", "refuse_cut_needed_byte", "refuse_cut_zero_tail_1", "refuse_dist_plus_1_after_10000"]
