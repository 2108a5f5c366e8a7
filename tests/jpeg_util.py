"""Test helpers for the JPEG path: generated test images, Pillow encodes, and a small baseline JPEG *encoder* for the
sampling layouts Pillow cannot write (4:4:0 = 1x2 luma, all components 2x2, custom restart intervals, 16-bit tables).
Data generation only -- nothing here decodes."""
import io

import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35,
                   42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

# ITU-T T.81 Annex K.3 typical Huffman tables
DC_L = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_C = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_L = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d],
        [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
         0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
         0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
         0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
         0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
         0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
         0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
         0xfa])
AC_C = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
        [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
         0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
         0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
         0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
         0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
         0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
         0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
         0xfa])


def make_image(w, h, mode="RGB", seed=1):
    """smooth structure + noise, so that DC, low and high AC coefficients, EOBs and ZRLs all occur; returns a PIL image"""
    from PIL import Image

    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(np.sin(x / 7.0 + c) + np.cos(y / 5.0 - c)) * 60 + 128 for c in range(3)], -1)
    a = np.clip(base + rng.normal(0, 25, (h, w, 3)), 0, 255).astype(np.uint8)
    im = Image.fromarray(a, "RGB")
    return im.convert("L") if mode == "L" else im


def pillow_jpeg(im, **kw):
    from PIL import ImageFile

    # optimised / progressive encodes are written in one piece: the encoder's buffer must hold the whole (noisy, hence large) stream
    ImageFile.MAXBLOCK = max(ImageFile.MAXBLOCK, 8 * im.size[0] * im.size[1] + (1 << 16))
    buf = io.BytesIO()
    im.save(buf, "JPEG", **kw)
    return buf.getvalue()


def pillow_decode(data):
    from PIL import Image

    return np.array(Image.open(io.BytesIO(data)))


def _codes(counts, symbols):
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            table[symbols[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return table


class _Bits:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, value, nbits):
        self.acc = (self.acc << nbits) | (value & ((1 << nbits) - 1))
        self.n += nbits
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
            self.n -= 8

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _fdct_blocks(plane):
    """plane (multiple of 8 both ways, float) -> (by, bx, 8, 8) DCT-II coefficients, JPEG normalisation"""
    k = np.arange(8)
    c = np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16) * 0.5
    c[0] *= 1 / np.sqrt(2)
    h, w = plane.shape
    b = plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3) - 128.0
    return np.einsum("ux,abxy,vy->abuv", c, b, c)


# DC luma table with categories 12..16 as well (10..14-bit codes): what the faults "dc_cat" and "dc_cat_16" need
DC_L_WIDE = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0], list(range(17)))

# faults encode_baseline can write into ONE block (fault = (kind, block number in coding order[, argument])); what the decoders must
# make of each is the rule list in include/rupphash.h (rph_jpeg_set_entropy)
BASELINE_FAULTS = {
    "bad_code": "refused",      # an AC code the table does not assign (sixteen 1-bits)
    "dc_cat": "decoded",        # DC category 12..15 (argument), a legal code of a widened table
    "dc_cat_16": "refused",     # DC category 16: a code the widened table assigns, a category no decoder takes
    "run_past_63": "refused",   # three ZRLs, then a value with run 15: position 64
    "zrl_past_63": "refused",   # four ZRLs from position 1: position 65
    "zrl_to_64": "decoded",     # a value at 47, then a ZRL that ends the block exactly (no EOB)
}


QL_STD = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62, 18, 22,
                   37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
QC_STD = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)


def grid(w, h, sampling):
    """(hmax, vmax, mcus_x, mcus_y) of a frame; component ci has mcus_y * V by mcus_x * H blocks (the MCU-padded grid)"""
    hmax = max(s[0] for s in sampling)
    vmax = max(s[1] for s in sampling)
    return hmax, vmax, -(-w // (8 * hmax)), -(-h // (8 * vmax))


def _i16(v):
    """v modulo 2^16 into int16's range: what a decoder's (int16_t) store keeps of it"""
    return ((int(v) + 32768) & 0xFFFF) - 32768


def _image_blocks(rgb, sampling, quality_scale, gray, top):
    """the forward half of the encoders: YCbCr, box-averaged chroma, forward DCT, quantisation.  Returns (h, w, sampling, qts, blocks), blocks
    per component (blocks high, blocks wide, 8, 8) int64 over the MCU-padded grid, natural order"""
    rgb = np.asarray(rgb)
    if gray:
        h, w = rgb.shape
        comps = [rgb.astype(np.float64)]
        sampling = ((1, 1),)
    else:
        h, w, _ = rgb.shape
        r, g, b = [rgb[..., i].astype(np.float64) for i in range(3)]
        comps = [0.299 * r + 0.587 * g + 0.114 * b, -0.168736 * r - 0.331264 * g + 0.5 * b + 128, 0.5 * r - 0.418688 * g - 0.081312 * b + 128]
    hmax, vmax, mcus_x, mcus_y = grid(w, h, sampling)
    qts = [np.clip(np.round(q * quality_scale), 1, top).astype(np.int64) for q in (QL_STD, QC_STD)]
    blocks = []
    for ci, (plane, (H, V)) in enumerate(zip(comps, sampling)):
        fx, fy = hmax // H, vmax // V
        pw, ph = mcus_x * 8 * hmax, mcus_y * 8 * vmax
        full = np.pad(plane, ((0, ph - h), (0, pw - w)), mode="edge")
        small = full.reshape(ph // fy, fy, pw // fx, fx).mean(axis=(1, 3))
        q = qts[0 if ci == 0 else 1].reshape(8, 8)
        blocks.append(np.round(_fdct_blocks(small) / q).astype(np.int64))
    return h, w, sampling, qts, blocks


def _dqt(qts, sixteen_bit_tables):
    out = b""
    for t, q in enumerate(qts):
        zz = np.asarray(q).reshape(64)[ZIGZAG]
        body = b"".join(int(v).to_bytes(2, "big") for v in zz) if sixteen_bit_tables else bytes(int(v) for v in zz)
        out += bytes([0xFF, 0xDB]) + (len(body) + 3).to_bytes(2, "big") + bytes([(0x10 if sixteen_bit_tables else 0) | t]) + body
    return out


def _dc_difference(want, pred):
    """the difference that takes a decoder's prediction `pred` to `want` modulo 2^16, in -32767..32767 (categories 0..15)"""
    diff = want - pred
    if not -32767 <= diff <= 32767:
        diff = _i16(diff)
        if diff == -32768:
            raise ValueError(f"DC {want} after {pred}: a difference of 2^15 needs category 16; reach the value over two blocks")
    return diff


def _real_blocks(w, h, sampling, ci, hmax, vmax):
    """blocks (wide, high) of a component's own grid, what a scan of that component alone covers (T.81 A.2.2)"""
    H, V = sampling[ci]
    return -(-(-(-w * H // hmax)) // 8), -(-(-(-h * V // vmax)) // 8)


def encode_baseline_coefficients(blocks, qts, w, h, sampling=((1, 2), (1, 1), (1, 1)), restart_interval=0, interleaved=True, sixteen_bit_tables=False, gray=False,
                                 tables="used", fault=None, mcu_positions=False):
    """The entropy half of a baseline (SOF0) encoder.  blocks: per component an integer array (blocks high, blocks wide, 8, 8) or (.., 64) over
    the MCU-padded grid, natural order, quantised; qts: the quantisation tables (64 entries, natural order) of luma and chroma.
    AC values are int16 except -32768 (categories 1..15).  DC values are what the block is AIMED at: each is coded as the difference from the
    decoder's prediction modulo 2^16, so a chain 32767, -32768, 32767 costs differences of 1, and values beyond int16 are allowed (the decoders
    keep the prediction in 32 bits and narrow at the store).  A difference of exactly 2^15 has no category below 16: ValueError.
    tables: "used" = one table per class and slot, fixed-length codes for the symbols that occur (DC categories to 15 and AC sizes to 15 become
    codable); "annex_k" = T.81 K.3's tables.  fault: as encode_baseline (Annex K tables only).
    Returns (bytes, expected): expected = the (total blocks, 64) int16 coefficients a decoder holds afterwards, component-major, raster over the
    padded grid, natural order -- plain int16 arithmetic on `blocks` (blocks a scan of one component does not cover stay 0).
    mcu_positions: also return, per scan, the bit position (from the scan's first entropy bit, byte stuffing not counted) at which each of
    its MCUs was written, and behind them the position behind the last one -- (bytes, expected, [positions of scan 0, ..])."""
    if gray:
        sampling = ((1, 1),)
    ncomp = len(sampling)
    assert len(blocks) == ncomp and (tables == "annex_k" or not fault)
    hmax, vmax, mcus_x, mcus_y = grid(w, h, sampling)
    blocks = [np.asarray(b).astype(np.int64).reshape(mcus_y * V, mcus_x * H, 64) for b, (H, V) in zip(blocks, sampling)]
    expected = [np.zeros(b.shape, np.int16) for b in blocks]
    dc_l = DC_L_WIDE if fault and fault[0] in ("dc_cat", "dc_cat_16") else DC_L
    pred = [0] * ncomp
    luma_blocks = [0]
    scans = []  # (component indices, tokens): ("s", "dc" | "ac", slot, symbol) | ("b", value, nbits) | ("rst", n) | ("mcu",): an MCU begins

    def put_fault(toks, kind, arg):
        if kind == "dc_cat":  # the block's DC: the largest difference of the category, the prediction follows it
            toks += [("s", "dc", 0, arg), ("b", (1 << arg) - 1, arg), ("s", "ac", 0, 0x00)]
            pred[0] += (1 << arg) - 1
        elif kind == "dc_cat_16":  # (refused at the code: no magnitude bits follow)
            toks.append(("s", "dc", 0, 16))
        elif kind == "bad_code":
            toks.append(("b", 0xFFFF, 16))
        elif kind == "run_past_63":
            toks += [("s", "ac", 0, 0xF0)] * 3 + [("s", "ac", 0, 0xF1), ("b", 1, 1)]
        elif kind == "zrl_past_63":
            toks += [("s", "ac", 0, 0xF0)] * 4
        elif kind == "zrl_to_64":
            toks += [("s", "ac", 0, 0xF0)] * 2 + [("s", "ac", 0, 0xE1), ("b", 1, 1), ("s", "ac", 0, 0xF0)]
        else:
            raise ValueError(kind)

    def put_block(toks, ci, by, bx):
        t = 0 if ci == 0 else 1
        zz = blocks[ci][by, bx][ZIGZAG].tolist()
        if ci == 0:
            luma_blocks[0] += 1
            if fault and luma_blocks[0] - 1 == fault[1]:
                if fault[0] not in ("dc_cat", "dc_cat_16"):
                    toks.append(("s", "dc", 0, 0))  # DC difference 0
                put_fault(toks, fault[0], fault[2] if len(fault) > 2 else 12)
                return
        diff = _dc_difference(zz[0], pred[ci])
        pred[ci] += diff
        s = abs(diff).bit_length()
        toks.append(("s", "dc", t, s))
        if s:
            toks.append(("b", diff if diff >= 0 else diff + (1 << s) - 1, s))
        run = 0
        end = max([k for k in range(1, 64) if zz[k]], default=0)
        for k in range(1, end + 1):
            v = zz[k]
            if v == 0:
                run += 1
                continue
            while run > 15:
                toks.append(("s", "ac", t, 0xF0))
                run -= 16
            s = abs(v).bit_length()
            if s > 15:
                raise ValueError(f"AC {v}: no category below 16")
            toks.append(("s", "ac", t, (run << 4) | s))
            toks.append(("b", v if v >= 0 else v + (1 << s) - 1, s))
            run = 0
        if end < 63:
            toks.append(("s", "ac", t, 0x00))
        expected[ci][by, bx] = [_i16(pred[ci])] + [_i16(v) for v in blocks[ci][by, bx][1:].tolist()]

    def scan(cis):
        nonlocal pred
        toks = []
        pred = [0] * ncomp
        if len(cis) == 1 and ncomp > 1:  # the component's own grid: ceil(samples / 8) blocks each way, one block per MCU
            bw, bh = _real_blocks(w, h, sampling, cis[0], hmax, vmax)
            units = [[(cis[0], by, bx)] for by in range(bh) for bx in range(bw)]
        else:
            units = [[(ci, my * sampling[ci][1] + v, mx * sampling[ci][0] + hh) for ci in cis for v in range(sampling[ci][1]) for hh in range(sampling[ci][0])]
                     for my in range(mcus_y) for mx in range(mcus_x)]
        rst = 0
        for count, unit in enumerate(units):
            if restart_interval and count and count % restart_interval == 0:
                toks.append(("rst", rst & 7))
                rst += 1
                pred = [0] * ncomp
            toks.append(("mcu",))
            for ci, by, bx in unit:
                put_block(toks, ci, by, bx)
        scans.append((cis, toks))

    if interleaved or ncomp == 1:
        scan(list(range(ncomp)))
    else:
        for ci in range(ncomp):
            scan([ci])

    slots = [0] if ncomp == 1 else [0, 1]
    if tables == "annex_k":
        defs = {("dc", 0): dc_l, ("ac", 0): AC_L, ("dc", 1): DC_C, ("ac", 1): AC_C}
    else:
        defs = {(cls, t): _table_for({k[3] for _, toks in scans for k in toks if k[0] == "s" and k[1] == cls and k[2] == t}, False) for t in slots for cls in ("dc", "ac")}
    out = bytearray(b"\xff\xd8")

    def seg(marker, payload):
        out.extend(bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload)

    out.extend(_dqt(qts[:len(slots)], sixteen_bit_tables))
    sof = bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([ncomp])
    for ci, (H, V) in enumerate(sampling):
        sof += bytes([ci + 1, (H << 4) | V, 0 if ci == 0 else 1])
    seg(0xC0, sof)
    for t in slots:
        for cls in ("dc", "ac"):
            counts, symbols = defs[cls, t]
            seg(0xC4, bytes([(0x10 if cls == "ac" else 0) | t]) + bytes(counts) + bytes(symbols))
    if restart_interval:
        seg(0xDD, restart_interval.to_bytes(2, "big"))
    codes = {key: _codes(*d) for key, d in defs.items()}
    positions = []
    for cis, toks in scans:
        sos = bytes([len(cis)])
        for ci in cis:
            sos += bytes([ci + 1, 0x00 if ci == 0 else 0x11])
        seg(0xDA, sos + bytes([0, 63, 0]))
        bits = _Bits()
        written, starts = 0, []  # bits put so far (padding before an RSTn included, markers and stuffing not)
        for k in toks:
            if k[0] == "s":
                bits.put(*codes[k[1], k[2]][k[3]])
                written += codes[k[1], k[2]][k[3]][1]
            elif k[0] == "b":
                bits.put(k[1], k[2])
                written += k[2]
            elif k[0] == "mcu":
                starts.append(written)
            else:
                bits.flush()
                written += -written % 8
                bits.out.extend(bytes([0xFF, 0xD0 + k[1]]))
        starts.append(written)
        positions.append(starts)
        bits.flush()
        out.extend(bits.out)
    out.extend(b"\xff\xd9")
    result = bytes(out), np.concatenate([e.reshape(-1, 64) for e in expected])
    return result + (positions,) if mcu_positions else result


def encode_baseline(rgb, sampling=((1, 2), (1, 1), (1, 1)), quality_scale=1.0, restart_interval=0, gray=False, sixteen_bit_tables=False, interleaved=True,
                    fault=None):
    """A plain baseline (SOF0) encoder: rgb (h, w, 3) uint8 [or (h, w) when gray]; sampling = (H, V) per component.
    Chroma is box-averaged down.  interleaved=False writes one scan per component (each over the component's own block grid,
    T.81 A.2.2).  fault: (kind, block[, argument]) of BASELINE_FAULTS, written into that block of the first scan (luma blocks only).
    Returns the JPEG byte string."""
    h, w, sampling, qts, blocks = _image_blocks(rgb, sampling, quality_scale, gray, 65535 if sixteen_bit_tables else 255)
    return encode_baseline_coefficients(blocks, qts, w, h, sampling, restart_interval, interleaved, sixteen_bit_tables, gray, tables="annex_k", fault=fault)[0]


# ---- a progressive (SOF2) encoder with an arbitrary scan script --------------------------------------------------------------------
# Pillow / libjpeg only write libjpeg's default script.  The decoders' hard cases are elsewhere: bands refined in another order than they
# were first coded, deep successive approximation, end-of-band runs that carry correction bits, sixteen zero-history coefficients stepped
# over inside a refinement scan, codes longer than the lookup tables.  T.81 G.1.2 procedures as libjpeg's encoder arranges them (correction
# bits are held back until the symbol they follow is out).

def _table_for(used, long_codes):
    """a Huffman table (counts[16], symbols) for the symbols in `used`: fixed-length codes (the all-ones code stays free), or -- long_codes --
    the first eight symbols with 2..9 bits and all the others with 16 bits (codes beyond every decoder's lookup table)"""
    used = sorted(used)
    counts = [0] * 16
    if long_codes and len(used) > 8:
        for l in range(2, 10):
            counts[l - 1] = 1
        counts[15] = len(used) - 8
    else:
        length = max(1, int(np.ceil(np.log2(len(used) + 1))))
        counts[length - 1] = len(used)
    return counts, used


# faults encode_progressive can put at the start of one scan (fault = (kind, scan number)); the scan must be of the kind named
PROGRESSIVE_FAULTS = {
    "zrl_past_se": "refused",         # AC first scan: ZRLs that step past Se
    "run_past_se": "refused",         # AC first scan of fewer than 16 coefficients: a value with a run to Se + 1
    "eobrun_overrun": "decoded",      # AC first scan (not refined later): an end-of-band run of 2^15 - 2 blocks, more than the scan has
    "refine_bad_symbol": "refused",   # AC refinement scan: a symbol with a magnitude of 2
}


def encode_progressive_coefficients(blocks, qts, w, h, script, sampling=((2, 2), (1, 1), (1, 1)), gray=False, sixteen_bit_tables=False, long_codes=False,
                                    max_corr_bits=900, fault=None):
    """The entropy half of a progressive (SOF2) encoder.  blocks, qts: as encode_baseline_coefficients, but every value -- AC too -- is what
    the scans AIM at and may lie beyond int16: a first scan codes sign and magnitude >> Al (below 2^15: ValueError otherwise), a refinement
    scan sends bit Al of the magnitude.  What a decoder then holds is worked out alongside, in int16 arithmetic by T.81 G.1.2's rules as
    libjpeg applies them: a first scan stores (int16)(value << Al); a correction bit moves a coefficient that is not 0 away from zero by
    1 << Al unless its bit Al is set already, wrapping at 16 bits; a coefficient that is 0 when a refinement scan passes it -- never coded,
    or wrapped to 0 -- is a zero of the run, or becomes +-(1 << Al) when the bit sent for it is 1.  For values within int16 and scripts
    that refine each band one bit at a time, that is the value itself.  DC: the first scan codes differences of value >> Al modulo 2^16.
    max_corr_bits: an end-of-band run is cut when this many correction bits wait behind it (libjpeg's encoder: 900 of its 1000-bit buffer).
    Returns (bytes, expected) as encode_baseline_coefficients."""
    if gray:
        sampling = ((1, 1),)
    ncomp = len(sampling)
    assert len(blocks) == ncomp
    hmax, vmax, mcus_x, mcus_y = grid(w, h, sampling)
    blocks = [np.asarray(b).astype(np.int64).reshape(mcus_y * V, mcus_x * H, 64)[:, :, ZIGZAG] for b, (H, V) in zip(blocks, sampling)]  # zigzag order
    held = [np.zeros(b.shape, np.int64) for b in blocks]  # the decoder's coefficients, zigzag order
    out = bytearray(b"\xff\xd8")

    def seg(marker, payload):
        out.extend(bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload)

    out.extend(_dqt(qts if ncomp > 1 else qts[:1], sixteen_bit_tables))
    sof = bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([ncomp])
    for ci, (H, V) in enumerate(sampling):
        sof += bytes([ci + 1, (H << 4) | V, 0 if ci == 0 else 1])
    seg(0xC2, sof)

    def units_of(cis):
        if len(cis) == 1:  # the component's own grid (T.81 A.2.2)
            ci = cis[0]
            bw, bh = _real_blocks(w, h, sampling, ci, hmax, vmax) if ncomp > 1 else (-(-w // 8), -(-h // 8))
            return [(ci, by, bx) for by in range(bh) for bx in range(bw)]
        return [(ci, my * sampling[ci][1] + v, mx * sampling[ci][0] + hh) for my in range(mcus_y) for mx in range(mcus_x) for ci in cis
                for v in range(sampling[ci][1]) for hh in range(sampling[ci][0])]

    for scan_no, (cis, ss, se, ah, al) in enumerate(script):
        toks = []  # ('s', component, symbol) | ('b', value, nbits)
        p1 = 1 << al
        if ss == 0:
            pred = [0] * ncomp
            for ci, by, bx in units_of(cis):
                c0 = int(blocks[ci][by, bx, 0])
                if ah == 0:
                    diff = _dc_difference(c0 >> al, pred[ci])  # arithmetic shift: the DC point transform
                    pred[ci] += diff
                    held[ci][by, bx, 0] = _i16(pred[ci] << al)
                    s = abs(diff).bit_length()
                    toks.append(("s", ci, s))
                    if s:
                        toks.append(("b", diff if diff >= 0 else diff + (1 << s) - 1, s))
                else:
                    toks.append(("b", (c0 >> al) & 1, 1))
                    held[ci][by, bx, 0] |= ((c0 >> al) & 1) << al
        else:
            ci = cis[0]
            eobrun = 0
            be = []  # correction bits waiting behind the end-of-band run

            def flush_eobrun():
                nonlocal eobrun, be
                if eobrun:
                    n = eobrun.bit_length() - 1
                    toks.append(("s", ci, n << 4))
                    if n:
                        toks.append(("b", eobrun - (1 << n), n))
                    eobrun = 0
                for bit in be:
                    toks.append(("b", bit, 1))
                be = []

            for _, by, bx in units_of(cis):
                zz = blocks[ci][by, bx].tolist()
                cur = held[ci][by, bx].tolist()
                mag = [abs(v) >> al for v in zz]  # magnitudes are shifted, not the signed values
                if ah == 0:
                    r = 0
                    for k in range(ss, se + 1):
                        t = mag[k]
                        if t == 0:
                            r += 1
                            continue
                        flush_eobrun()
                        while r > 15:
                            toks.append(("s", ci, 0xF0))
                            r -= 16
                        s = t.bit_length()
                        if s > 15:
                            raise ValueError(f"AC {zz[k]} at Al {al}: no category below 16")
                        toks.append(("s", ci, (r << 4) | s))
                        toks.append(("b", t if zz[k] >= 0 else (~t) & ((1 << s) - 1), s))
                        cur[k] = _i16((t if zz[k] >= 0 else -t) << al)
                        r = 0
                    if r > 0:
                        eobrun += 1
                        if eobrun == 0x7FFF:
                            flush_eobrun()
                else:
                    eob = 0
                    for k in range(ss, se + 1):
                        if cur[k] == 0 and mag[k] & 1:
                            eob = k
                    r = 0
                    br = []
                    for k in range(ss, se + 1):
                        t = mag[k]
                        if cur[k] == 0 and not t & 1:
                            r += 1
                            continue
                        while r > 15 and k <= eob:
                            flush_eobrun()
                            toks.append(("s", ci, 0xF0))
                            r -= 16
                            toks.extend(("b", bit, 1) for bit in br)
                            br = []
                        if cur[k] != 0:
                            br.append(t & 1)
                            if t & 1 and cur[k] & p1 == 0:
                                cur[k] = _i16(cur[k] + p1 if cur[k] >= 0 else cur[k] - p1)
                            continue
                        flush_eobrun()
                        toks.append(("s", ci, (r << 4) | 1))
                        toks.append(("b", 0 if zz[k] < 0 else 1, 1))
                        toks.extend(("b", bit, 1) for bit in br)
                        cur[k] = -p1 if zz[k] < 0 else p1
                        br = []
                        r = 0
                    if r > 0 or br:
                        eobrun += 1
                        be.extend(br)
                        if eobrun == 0x7FFF or len(be) > max_corr_bits:
                            flush_eobrun()
                held[ci][by, bx] = cur
            flush_eobrun()
            if fault and fault[1] == scan_no:
                kind = fault[0]
                assert ss > 0 and (ah > 0) == (kind == "refine_bad_symbol"), (kind, script[scan_no])
                if kind == "zrl_past_se":
                    head = [("s", ci, 0xF0)] * ((se - ss + 1) // 16 + 1)
                elif kind == "run_past_se":
                    assert se - ss + 1 <= 15
                    head = [("s", ci, ((se - ss + 1) << 4) | 1), ("b", 1, 1)]
                elif kind == "eobrun_overrun":
                    head = [("s", ci, 14 << 4), ("b", 0x3FFF, 14)]
                elif kind == "refine_bad_symbol":
                    head = [("s", ci, 0x02), ("b", 3, 2)]
                else:
                    raise ValueError(kind)
                toks[:0] = head
        # tables: one per component of the scan (DC first scans) or one (AC scans); none for DC refinement
        slot = scan_no & 1
        codes = {}
        sos = bytes([len(cis)])
        for n_c, ci in enumerate(cis):
            used = {t[2] for t in toks if t[0] == "s" and t[1] == ci}
            tsel = (slot + n_c) & 3
            if used:
                counts, symbols = _table_for(used, long_codes and (scan_no + ci) % 2 == 0)
                seg(0xC4, bytes([(0x10 if ss else 0x00) | tsel]) + bytes(counts) + bytes(symbols))
                codes[ci] = _codes(counts, symbols)
            sos += bytes([ci + 1, (tsel << 4) if ss == 0 else tsel])
        seg(0xDA, sos + bytes([ss, se, (ah << 4) | al]))
        bits = _Bits()
        for t in toks:
            if t[0] == "s":
                bits.put(*codes[t[1]][t[2]])
            else:
                bits.put(t[1], t[2])
        bits.flush()
        out.extend(bits.out)
    out.extend(b"\xff\xd9")
    unzig = np.argsort(ZIGZAG)
    return bytes(out), np.concatenate([e[:, :, unzig].reshape(-1, 64) for e in held]).astype(np.int16)


def encode_progressive(rgb, script, sampling=((2, 2), (1, 1), (1, 1)), quality_scale=1.0, gray=False, long_codes=False, fault=None):
    """script: list of (components, Ss, Se, Ah, Al), components a tuple of indices (several only for DC scans).  Every scan gets its own
    Huffman table (written in front of it, slot 0 / 1 alternating so that slots are redefined between scans).  fault: (kind, scan) of
    PROGRESSIVE_FAULTS, put in front of that scan's symbols."""
    h, w, sampling, qts, blocks = _image_blocks(rgb, sampling, quality_scale, gray, 255)
    return encode_progressive_coefficients(blocks, qts, w, h, script, sampling, gray, long_codes=long_codes, fault=fault)[0]


# scan scripts for encode_progressive (three components unless noted)
SCRIPT_LIBJPEG = [((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1),
                  ((0, 1, 2), 0, 0, 1, 0), ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0)]
SCRIPT_SPECTRAL_ONLY = [((0, 1, 2), 0, 0, 0, 0), ((0,), 1, 63, 0, 0), ((1,), 1, 63, 0, 0), ((2,), 1, 63, 0, 0)]
SCRIPT_DEEP = [((0,), 0, 0, 0, 3), ((1,), 0, 0, 0, 2), ((2,), 0, 0, 0, 2), ((0,), 1, 2, 0, 3), ((0,), 3, 9, 0, 3), ((0,), 10, 63, 0, 3), ((0,), 1, 63, 3, 2),
               ((0,), 0, 0, 3, 2), ((0,), 1, 63, 2, 1), ((1,), 1, 63, 0, 2), ((1,), 1, 63, 2, 1), ((0,), 0, 0, 2, 1), ((1, 2), 0, 0, 2, 1), ((2,), 1, 63, 0, 0),
               ((0,), 1, 63, 1, 0), ((0, 1, 2), 0, 0, 1, 0), ((1,), 1, 63, 1, 0)]
SCRIPT_REFINE_BEFORE_OTHER_BANDS = [((0, 1, 2), 0, 0, 0, 0), ((0,), 1, 8, 0, 1), ((0,), 1, 8, 1, 0), ((0,), 9, 63, 0, 2), ((1,), 1, 63, 0, 1), ((0,), 9, 63, 2, 1),
                                    ((1,), 1, 63, 1, 0), ((2,), 1, 30, 0, 0), ((0,), 9, 63, 1, 0), ((2,), 31, 63, 0, 1), ((2,), 31, 63, 1, 0)]
SCRIPT_MANY_BANDS = [((0, 1, 2), 0, 0, 0, 0)] + [((c,), a, min(a + 2, 63), 0, 0) for a in range(1, 64, 3) for c in (0, 1, 2)]
SCRIPT_GRAY = [((0,), 0, 0, 0, 1), ((0,), 1, 63, 0, 2), ((0,), 1, 63, 2, 1), ((0,), 0, 0, 1, 0), ((0,), 1, 63, 1, 0)]


# ---- damaged streams ------------------------------------------------------------------------------------------------------------------
# What the decoders must make of a damaged stream is written down in include/rupphash.h (rph_jpeg_set_entropy): every entropy path and the
# CPU oracle must agree on it.  damaged_corpus() gives (name, bytes, expected) with expected "refused", "decoded" or None (random damage:
# only agreement is asserted), deterministic for a seed.

def _entropy_start(data):
    sos = data.find(b"\xff\xda")
    return sos + 2 + int.from_bytes(data[sos + 2:sos + 4], "big")


def restart_fault(data, kind, which=1):
    """a file with restart markers, RSTn number `which` (0-based) missing, renumbered, or replaced by a COM marker; or restart interval
    number `which` emptied (its entropy bytes removed: the RSTn behind it follows the SOS header or the RSTn before it at once)"""
    start = _entropy_start(data)
    pos = [i for i in range(start, len(data) - 1) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7]
    if kind == "interval_emptied":
        first = pos[which - 1] + 2 if which else start
        return data[:first] + data[pos[which]:]
    i = pos[which]
    if kind == "rst_missing":
        return data[:i] + data[i + 2:]
    if kind == "rst_renumbered":
        return data[:i + 1] + bytes([0xD0 + ((data[i + 1] - 0xD0 + 3) & 7)]) + data[i + 2:]
    if kind == "rst_replaced":
        return data[:i + 1] + b"\xfe" + data[i + 2:]
    raise ValueError(kind)


RESTART_FAULTS = {"rst_missing": "refused", "rst_renumbered": "decoded", "rst_replaced": "refused", "interval_emptied": "decoded"}


def _layouts(rng):
    """small clean files of every layout the device has special cases for: (name, bytes)"""
    a = np.array(make_image(45, 37, seed=int(rng.integers(1 << 30))))
    out = []
    for name, samp in [("444", ((1, 1), (1, 1), (1, 1))), ("422", ((2, 1), (1, 1), (1, 1))), ("420", ((2, 2), (1, 1), (1, 1))), ("440", ((1, 2), (1, 1), (1, 1)))]:
        out.append(("base" + name, encode_baseline(a, samp)))
        out.append(("base" + name + "_rst", encode_baseline(a, samp, restart_interval=2)))
    out.append(("gray", encode_baseline(a[..., 0], gray=True)))
    out.append(("gray_rst", encode_baseline(a[..., 0], gray=True, restart_interval=3)))
    out.append(("noninterleaved", encode_baseline(a, ((2, 2), (1, 1), (1, 1)), interleaved=False)))
    for name, script in [("libjpeg", SCRIPT_LIBJPEG), ("spectral", SCRIPT_SPECTRAL_ONLY), ("deep", SCRIPT_DEEP), ("refine_first", SCRIPT_REFINE_BEFORE_OTHER_BANDS)]:
        out.append(("prog_" + name, encode_progressive(a, script, ((2, 1), (1, 1), (1, 1)))))
    out.append(("prog_gray", encode_progressive(a[..., 0], SCRIPT_GRAY, gray=True)))
    return out


def _pillow_layouts(rng, w, h):
    from PIL import Image

    a = np.array(make_image(w, h, seed=int(rng.integers(1 << 30))))
    out = []
    for sub in (0, 1, 2):
        im = Image.fromarray(a)
        out.append((f"pil_s{sub}", pillow_jpeg(im, quality=85, subsampling=sub)))
        out.append((f"pil_s{sub}_prog", pillow_jpeg(im, quality=85, subsampling=sub, progressive=True)))
        out.append((f"pil_s{sub}_rst", pillow_jpeg(im, quality=85, subsampling=sub, restart_marker_blocks=2)))
    g = Image.fromarray(a).convert("L")
    out.append(("pil_gray", pillow_jpeg(g, quality=85)))
    out.append(("pil_gray_prog", pillow_jpeg(g, quality=85, progressive=True)))
    return out


def random_damage(data, rng):
    """bytes behind the first SOS overwritten, inserted or deleted (1..5 of them), or the file cut short"""
    start = _entropy_start(data)
    if len(data) - start < 8:
        return data[:start + 1]
    kind = int(rng.integers(0, 4))
    if kind == 3:
        return data[:int(rng.integers(start + 1, len(data) - 2))]
    b = bytearray(data)
    for _ in range(int(rng.integers(1, 6))):
        i = int(rng.integers(start, len(b) - 2))
        if kind == 0:
            b[i] = int(rng.integers(0, 256))
        elif kind == 1:
            b.insert(i, int(rng.integers(0, 256)))
        else:
            del b[i]
    return bytes(b)


def damaged_corpus(seed=2024, n_random=120):
    """(name, bytes, expected) -- one targeted file per rule and layout, then n_random randomly damaged ones"""
    rng = np.random.default_rng(seed)
    clean = _layouts(rng)
    a = np.array(make_image(40, 33, seed=int(rng.integers(1 << 30))))
    out = []
    for kind, want in BASELINE_FAULTS.items():
        for name, samp in [("444", ((1, 1), (1, 1), (1, 1))), ("420", ((2, 2), (1, 1), (1, 1))), ("440", ((1, 2), (1, 1), (1, 1)))]:
            for blk in (0, 5):
                f = (kind, blk, 12 + blk % 4 if blk else 15)
                out.append((f"{kind}_{name}_b{blk}", encode_baseline(a, samp, fault=f), want))
        out.append((f"{kind}_gray", encode_baseline(a[..., 0], gray=True, fault=(kind, 3, 13)), want))
        out.append((f"{kind}_noninterleaved", encode_baseline(a, ((2, 1), (1, 1), (1, 1)), interleaved=False, fault=(kind, 2, 14)), want))
        out.append((f"{kind}_rst", encode_baseline(a, ((2, 2), (1, 1), (1, 1)), restart_interval=2, fault=(kind, 9, 12)), want))
    for kind, want in PROGRESSIVE_FAULTS.items():
        # SCRIPT_LIBJPEG: scan 1 = luma 1..5 (first), scan 4 = luma 6..63 (first), scan 9 = luma 1..63 (refinement)
        # (an end-of-band run that skips coefficients a later scan refines makes that scan garbage: SCRIPT_SPECTRAL_ONLY has no refinement)
        script = SCRIPT_SPECTRAL_ONLY if kind == "eobrun_overrun" else SCRIPT_LIBJPEG
        scans = {"refine_bad_symbol": [9], "run_past_se": [1], "eobrun_overrun": [1, 3]}.get(kind, [1, 4])
        for sc in scans:
            out.append((f"{kind}_s{sc}", encode_progressive(a, script, ((2, 2), (1, 1), (1, 1)), fault=(kind, sc)), want))
        if kind != "run_past_se":  # (SCRIPT_GRAY has no band of fewer than 16 coefficients)
            gscript = SCRIPT_GRAY[:2] if kind == "eobrun_overrun" else SCRIPT_GRAY
            out.append((f"{kind}_gray", encode_progressive(a[..., 0], gscript, gray=True, fault=(kind, 2 if kind == "refine_bad_symbol" else 1)), want))
    for kind, want in RESTART_FAULTS.items():
        for name, data in clean:
            if name.endswith("_rst"):
                out.append((f"{kind}_{name}", restart_fault(data, kind), want))
                if kind == "interval_emptied":  # the first interval: its bound is byte 0 of the scan
                    out.append((f"{kind}0_{name}", restart_fault(data, kind, 0), want))
    for name, data in clean:
        # the first scan cut short mid-MCU, a marker inside its entropy data: decoded with zeros fed -- unless a restart boundary
        # follows, which then has no RSTn behind it (rule 5)
        st = _entropy_start(data)
        end = st
        while not (data[end] == 0xFF and data[end + 1] != 0 and not 0xD0 <= data[end + 1] <= 0xD7):
            end += 1
        cut = st + (end - st) // 3
        cut += data[cut - 1] == 0xFF  # (not between the two bytes of a stuffed 0xFF)
        rst = name.endswith("_rst")
        out.append((f"truncated_{name}", data[:cut], "refused" if rst else "decoded"))
        for m in (0xD9, 0xD3, 0xFE):
            out.append((f"marker_{m:02x}_{name}", data[:cut] + bytes([0xFF, m]) + data[cut:], "refused" if rst and m != 0xD3 else (None if m == 0xFE else "decoded")))
        out.append((f"fill_{name}", data[:cut] + b"\xff\xff" + data[cut:], None))
    pool = clean + _pillow_layouts(rng, 61, 45)
    for i in range(n_random):
        name, data = pool[i % len(pool)]
        out.append((f"random{i}_{name}", random_damage(data, rng), None))
    return out
