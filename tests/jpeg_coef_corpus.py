"""JPEG files written from COEFFICIENTS, not from pictures: what the arithmetic side of the decoders (dequantise, both integer IDCTs, range
limiting, chroma upsampling, colour, luma) and the int16 coefficient store never get from an encoder.  corpus() gives
name -> (bytes, expected coefficients or None, in_range); the name's part before "/" is the class:

  impulse       one coefficient per block: every position x {+-1, +-255, +-1023, +-2047, +-16384, 32767, -32768} x quantiser {1, 255, 65535}
  dc_sweep      DC-only blocks, the dequantised DC stepping through -16384..16383 (every output residue modulo 1024) and beyond
  overshoot     rounded forward DCTs of sample blocks from [-256, 511], quantisers 1..16 (in_range: 16-bit decoders agree, Pillow is asserted)
  random_heavy  mostly small coefficients, a few per block anywhere in int16; every sampling, table width, restart interval, scan layout
  dc_pred       DC chains that take the prediction far beyond +-32767, with restarts, one scan per component, progressive Al = 1, 5, 13
  prog_extreme  progressive scans whose value << Al wraps in int16, refinements of -32768 / 32767 / +-2^k / +-(2^k - 1), repeated refinement
                scans, end-of-band runs with r = 14 over blocks that carry correction bits, the band layouts of ju.SCRIPT_*
  chroma_edges  chroma planes alternating 0 / 255 per sample, row, column and 2x2 cell under luma 0, 255 and noise, at sizes that put the
                chroma edge rules and the fused kernel's tile borders inside, on and outside the image

Seeded: the same files on every call."""
import functools

import numpy as np

import jpeg_util as ju

S444, S422, S440, S420 = ((1, 1), (1, 1), (1, 1)), ((2, 1), (1, 1), (1, 1)), ((1, 2), (1, 1), (1, 1)), ((2, 2), (1, 1), (1, 1))
SAMPLINGS = {"444": S444, "422": S422, "440": S440, "420": S420, "gray": ((1, 1),)}
CLASSES = ("impulse", "dc_sweep", "overshoot", "random_heavy", "dc_pred", "prog_extreme", "chroma_edges")
IMPULSE_VALUES = (1, -1, 255, -255, 1023, -1023, 2047, -2047, 16384, -16384, 32767, -32768)
LARGE = ("prog_extreme/eobrun_r14",)  # files of more than 160 x 96 pixels (a run of 2^14 blocks needs that many)


def shapes(w, h, sampling):
    """(blocks high, blocks wide) of every component's MCU-padded grid"""
    _, _, mx, my = ju.grid(w, h, sampling)
    return [(my * V, mx * H) for H, V in sampling]


def _flat_q(v):
    return [np.full(64, v, np.int64)] * 2


def _baseline(files, name, blocks, qts, w, h, samp, in_range=False, **kw):
    data, exp = ju.encode_baseline_coefficients(blocks, qts, w, h, samp, gray=len(samp) == 1, **kw)
    files[name] = (data, exp, in_range)


def _progressive(files, name, blocks, qts, w, h, script, samp, **kw):
    data, exp = ju.encode_progressive_coefficients(blocks, qts, w, h, script, samp, gray=len(samp) == 1, **kw)
    files[name] = (data, exp, False)


def _impulse(files):
    # DC cases first, in an order whose differences all have a category below 16 (32767 -> -32768 is +1 modulo 2^16; -32768 -> 0 would be 2^15)
    cases = [(0, v) for v in (1, -1, 255, -255, 1023, -1023, 2047, -2047, 16384, 32767, -32768, -16384)]
    cases += [(p, v) for p in range(1, 64) for v in IMPULSE_VALUES if v != -32768]  # an AC of -32768 has no sequential code: progressive, below
    for qname, q, t16 in (("q1", 1, False), ("q255", 255, False), ("q65535", 65535, True)):
        for part in range(0, len(cases), 240):
            blk = np.zeros((12, 20, 64), np.int64)
            for i, (p, v) in enumerate(cases[part:part + 240]):
                blk[i // 20, i % 20, p] = v
            _baseline(files, f"impulse/{qname}_{part // 240}", [blk], _flat_q(q), 160, 96, SAMPLINGS["gray"], sixteen_bit_tables=t16)
        blk = np.zeros((7, 9, 64), np.int64)
        for p in range(1, 64):
            blk[(p - 1) // 9, (p - 1) % 9, p] = -32768  # -16384 << 1
        _progressive(files, f"impulse/{qname}_min", [blk], _flat_q(q), 72, 56, [((0,), 0, 0, 0, 0), ((0,), 1, 63, 0, 1)], SAMPLINGS["gray"], sixteen_bit_tables=t16)


def _dc_only(values):
    blk = np.zeros((12, 20, 64), np.int64)
    blk.reshape(240, 64)[:len(values), 0] = values
    return [blk]


def _dc_sweep(files):
    dcs = np.arange(-16384, 16384, 7)
    for part in range(0, len(dcs), 240):
        _baseline(files, f"dc_sweep/q1_{part // 240:02d}", _dc_only(dcs[part:part + 240]), _flat_q(1), 160, 96, SAMPLINGS["gray"])
    _baseline(files, "dc_sweep/q255", _dc_only(np.arange(-120, 120)), _flat_q(255), 160, 96, SAMPLINGS["gray"])
    _baseline(files, "dc_sweep/q65535", _dc_only(np.arange(-120, 120)), _flat_q(65535), 160, 96, SAMPLINGS["gray"], sixteen_bit_tables=True)
    _baseline(files, "dc_sweep/int16", _dc_only(-32767 + 273 * np.arange(240)), _flat_q(1), 160, 96, SAMPLINGS["gray"])


def fdct_quantised(samples, q):
    """round(forward DCT of the sample plane (level shift 128 taken off) / q): (blocks high, blocks wide, 8, 8) int64"""
    return np.round(ju._fdct_blocks(samples.astype(np.float64) + 128.0) / np.asarray(q, np.float64).reshape(8, 8)).astype(np.int64)


def _overshoot_samples(kind, rows, cols, rng):
    """a plane of level-shifted samples in [-384, 383] (= [-256, 511] as pixel values)"""
    y, x = np.mgrid[0:rows, 0:cols]
    if kind == "flat":
        v = rng.integers(-384, 384, (rows // 8, cols // 8))
        return np.repeat(np.repeat(v, 8, 0), 8, 1)
    if kind == "checker":
        return np.where((x + y) & 1, 383, -384)
    if kind == "hot":
        out = np.repeat(np.repeat(rng.integers(-100, 100, (rows // 8, cols // 8)), 8, 0), 8, 1)
        hot = rng.integers(0, 64, (rows // 8, cols // 8))
        sel = ((y % 8) * 8 + x % 8) == np.repeat(np.repeat(hot, 8, 0), 8, 1)
        return np.where(sel, np.where((x // 8 + y // 8) & 1, 383, -384), out)
    if kind == "ramps":
        return np.where((y // 8) & 1, -384 + (767 * x) // max(cols - 1, 1), 383 - (767 * y) // max(rows - 1, 1))
    return rng.integers(-384, 384, (rows, cols))


def _overshoot(files, rng):
    sizes = [(160, 96), (77, 51), (45, 37), (129, 65), (24, 17)]
    for si, (sname, samp) in enumerate(SAMPLINGS.items()):
        for ki, kind in enumerate(("flat", "checker", "hot", "ramps", "noise")):
            w, h = sizes[(si + ki) % 5]
            qts = [rng.integers(1, 17, 64) for _ in range(2)]
            blocks = [fdct_quantised(_overshoot_samples(kind, 8 * bh, 8 * bw, rng), qts[min(ci, 1)]) for ci, (bh, bw) in enumerate(shapes(w, h, samp))]
            _baseline(files, f"overshoot/{kind}_{sname}", blocks, qts, w, h, samp, in_range=True, restart_interval=(0, 0, 2)[ki % 3], interleaved=ki != 3)


def heavy_blocks(shape, rng, top=32767):
    """(.., 64) coefficients: most 0 or small, one to four per block anywhere in -top..top"""
    n = int(np.prod(shape))
    blk = rng.integers(-3, 4, (n, 64)) * (rng.random((n, 64)) < 0.3)
    for b in range(n):
        for p in rng.integers(0, 64, int(rng.integers(1, 5))):
            blk[b, p] = rng.integers(-top, top + 1)
    return blk.reshape(*shape, 64)


def _random_heavy(files, rng):
    w, h = 45, 37
    for sname, samp in SAMPLINGS.items():
        for t16 in (False, True):
            for rst in (0, 1, 3):
                for il in ((True,) if sname == "gray" else (True, False)):
                    qts = [rng.integers(1, 65536 if t16 else 256, 64) for _ in range(2)]
                    blocks = [heavy_blocks(s, rng) for s in shapes(w, h, samp)]
                    _baseline(files, f"random_heavy/{sname}_{'q16' if t16 else 'q8'}_rst{rst}_{'il' if il else 'ni'}", blocks, qts, w, h, samp,
                              restart_interval=rst, interleaved=il, sixteen_bit_tables=t16)


def _chain(n, step, turn):
    """n values walking up by `step` to `turn`, down to -turn, and up again"""
    out, v, d = [], 0, step
    for _ in range(n):
        v += d
        if abs(v) >= turn:
            d = -d
        out.append(v)
    return np.array(out, np.int64)


def _dc_pred(files, rng):
    def blocks_for(w, h, samp, turn, low_bits=0):
        out = []
        for bh, bw in shapes(w, h, samp):
            blk = rng.integers(-2, 3, (bh, bw, 64)) * (rng.random((bh, bw, 64)) < 0.1)
            blk[..., 0] = (_chain(bh * bw, 30000, turn).reshape(bh, bw) << low_bits) | rng.integers(0, 1 << low_bits, (bh, bw))
            out.append(blk)
        return out

    q = [rng.integers(1, 20, 64) for _ in range(2)]
    for name, samp, w, h, kw in (("gray", SAMPLINGS["gray"], 64, 48, {}), ("gray_rst5", SAMPLINGS["gray"], 64, 48, {"restart_interval": 5}),
                                 ("444_rst2", S444, 48, 40, {"restart_interval": 2}), ("420", S420, 61, 45, {}),
                                 ("422_ni", S422, 61, 45, {"interleaved": False}), ("440_ni_rst3", S440, 40, 61, {"interleaved": False, "restart_interval": 3})):
        _baseline(files, f"dc_pred/{name}", blocks_for(w, h, samp, 240000), q, w, h, samp, **kw)
    for al in (1, 5, 13):  # (prediction * 2^Al stays within 32 bits: the prediction turns at +-120000)
        refine = [al - k for k in range(al)]
        gray = [((0,), 0, 0, 0, al)] + [((0,), 0, 0, a, a - 1) for a in refine] + [((0,), 1, 63, 0, 0)]
        _progressive(files, f"dc_pred/prog_gray_al{al}", blocks_for(64, 48, SAMPLINGS["gray"], 120000, al), q, 64, 48, gray, SAMPLINGS["gray"])
        colour = [((0, 1, 2), 0, 0, 0, al)]
        for a in refine:  # all three components in one scan, or in two
            colour += [((0, 1, 2), 0, 0, a, a - 1)] if a & 1 else [((2, 0), 0, 0, a, a - 1), ((1,), 0, 0, a, a - 1)]
        colour += [((c,), 1, 63, 0, 0) for c in range(3)]
        _progressive(files, f"dc_pred/prog_420_al{al}", blocks_for(45, 37, S420, 120000, al), q, 45, 37, colour, S420)


def _prog_extreme(files, rng):
    gray = SAMPLINGS["gray"]
    q = [rng.integers(1, 30, 64) for _ in range(2)]

    def down(c, ss, se, al):  # the refinement scans from Al to 0
        return [((c,), ss, se, a, a - 1) for a in range(al, 0, -1)]

    # value << Al in every category up to 15, then refined bit by bit: what the first scan stores wraps in int16
    for al in (1, 5, 9, 13):
        blk = np.zeros((3, 4, 64), np.int64)
        for b in range(12):
            for p in range(1, 64):
                if rng.random() < 0.5:
                    mag = int(rng.integers(1 << (b + 3), 1 << (b + 4)))  # block b: category b + 4
                    blk[b // 4, b % 4, p] = (-1) ** int(rng.integers(2)) * ((mag << al) | int(rng.integers(0, 1 << al)))
        blk[..., 0] = rng.integers(-1000, 1000, (3, 4))
        _progressive(files, f"prog_extreme/cat15_al{al}", [blk], q, 32, 24, [((0,), 0, 0, 0, 0), ((0,), 1, 63, 0, al)] + down(0, 1, 63, al), gray)
        _progressive(files, f"prog_extreme/cat15_al{al}_split", [blk], q, 32, 24,
                     [((0,), 0, 0, 0, 0), ((0,), 1, 20, 0, al), ((0,), 21, 63, 0, al)] + down(0, 1, 20, al) + down(0, 21, 63, al), gray, long_codes=True)
    # a refinement scan arriving at +-2^k (+ correction bit 0 and 1), 32767 and -32768: the last one leaves int16 on the far side
    special = [s * ((1 << k) + d) for k in range(1, 16) for d in (0, 1) for s in (1, -1)] + [32767, -32767, -32769, 32766, -32766]
    blk = np.zeros((2, 4, 64), np.int64)
    blk.reshape(8, 64)[:, 1:].flat[:len(special)] = special
    blk.reshape(8, 64)[:, 1:].flat[len(special):2 * len(special)] = special[::-1]
    _progressive(files, "prog_extreme/refine_powers", [blk], q, 32, 16, [((0,), 0, 0, 0, 0), ((0,), 1, 63, 0, 1), ((0,), 1, 63, 1, 0)], gray)
    blk3 = [blk] + [np.roll(blk, 1 + c, axis=2) * np.array([0] + [1] * 63) for c in range(2)]
    _progressive(files, "prog_extreme/refine_powers_444", blk3, q, 32, 16,
                 [((0, 1, 2), 0, 0, 0, 0)] + [((c,), 1, 63, 0, 1) for c in range(3)] + [((c,), 1, 63, 1, 0) for c in (2, 0, 1)], S444)
    # ... and at +-(2^k - 1), 32767: a refinement at the first scan's own Al finds the bit set already wherever it is sent as 1
    special = [s * ((1 << k) - d) for k in range(1, 16) for d in (0, 1) for s in (1, -1) if (1 << k) - d < 32768]
    blk = np.zeros((2, 4, 64), np.int64)
    blk.reshape(8, 64)[:, 1:].flat[:len(special)] = special
    _progressive(files, "prog_extreme/bit_already_set", [blk], q, 32, 16, [((0,), 0, 0, 0, 0), ((0,), 1, 63, 0, 0), ((0,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0)], gray)
    # a first scan whose value << Al is 0 modulo 2^16: the decoders' store holds 0, and the next refinement scan meets a coefficient without history
    blk = np.zeros((2, 4, 64), np.int64)
    flat = blk.reshape(8, 64)
    for b in range(8):
        for p in range(1, 64):
            u = rng.random()
            if u < 0.25:
                flat[b, p] = (-1) ** p * (65536 * int(rng.integers(1, 4)) + int(rng.integers(0, 4)) * 2048)  # held 0 after the first scan
            elif u < 0.5:
                flat[b, p] = (-1) ** b * int(rng.integers(1, 1 << 18))
    _progressive(files, "prog_extreme/wrap_to_zero", [blk], q, 32, 16, [((0,), 0, 0, 0, 0), ((0,), 1, 63, 0, 13)] + down(0, 1, 63, 13)[:3], gray)
    _progressive(files, "prog_extreme/wrap_to_zero_422", [np.zeros((2, 6, 64), np.int64), blk[:, :3], blk[:, 1:]], q, 40, 16,
                 [((0, 1, 2), 0, 0, 0, 0), ((1,), 1, 63, 0, 13), ((2,), 1, 30, 0, 13), ((2,), 1, 30, 13, 12), ((1,), 1, 63, 13, 12), ((1,), 1, 63, 12, 11)], S422)
    # every refinement scan twice
    for sname, samp in (("gray", gray), ("420", S420)):
        blocks = [heavy_blocks(s, rng) for s in shapes(45, 37, samp)]
        script = [(tuple(range(len(samp))), 0, 0, 0, 0)]
        for c in range(len(samp)):
            script += [((c,), 1, 63, 0, 2), ((c,), 1, 63, 2, 1), ((c,), 1, 63, 2, 1), ((c,), 1, 63, 1, 0), ((c,), 1, 63, 1, 0)]
        _progressive(files, f"prog_extreme/refine_twice_{sname}", blocks, q, 45, 37, script, samp)
    # the band layouts of the scan scripts, on heavy-tailed int16 coefficients
    for name, script in (("deep", ju.SCRIPT_DEEP), ("refine_first", ju.SCRIPT_REFINE_BEFORE_OTHER_BANDS), ("many_bands", ju.SCRIPT_MANY_BANDS)):
        for sname in ("444", "422", "440", "420"):
            samp = SAMPLINGS[sname]
            _progressive(files, f"prog_extreme/{name}_{sname}", [heavy_blocks(s, rng) for s in shapes(45, 37, samp)], q, 45, 37, script, samp, long_codes=sname == "422")
    # end-of-band runs with r = 14 (16384..32767 blocks): one over blocks without coefficients in a first scan, one in a refinement scan over
    # blocks that all carry correction bits (the writer does not cut the run at libjpeg's 900 waiting bits)
    bh, bw = 128, 129
    blk = np.zeros((bh, bw, 64), np.int64)
    n = bh * bw
    flat = blk.reshape(n, 64)
    flat[::3, 1] = rng.integers(2, 8, len(flat[::3])) * (-1) ** np.arange(len(flat[::3]))
    flat[1::5, 2] = rng.integers(2, 4, len(flat[1::5]))
    flat[:, 0] = rng.integers(-40, 40, n)
    _progressive(files, "prog_extreme/eobrun_r14", [blk], _flat_q(3), 8 * bw, 8 * bh,
                 [((0,), 0, 0, 0, 0), ((0,), 1, 2, 0, 1), ((0,), 3, 63, 0, 0), ((0,), 1, 2, 1, 0)], gray, max_corr_bits=1 << 30)


def _chroma_edges(files, rng):
    patterns = {"sample": lambda x, y: (x + y) & 1, "row": lambda x, y: y & 1, "column": lambda x, y: x & 1, "cell": lambda x, y: ((x >> 1) + (y >> 1)) & 1}
    i = 0
    for sname in ("444", "422", "440", "420"):
        samp = SAMPLINGS[sname]
        hs, vs = samp[0]
        sizes = [(127, 63), (128, 64), (129, 65), (136, 72)]
        # chroma planes of 1, 2 and 3 columns / rows (an odd count under a factor of 2 comes from an odd luma size).  An image below 5 pixels
        # either way has no PDQ hash, so the planes of 1 and 2 are seen through the pixels and the pixel hash alone; those of 3 under a
        # factor of 2 are 5 pixels, with 9 chroma samples the other way: the fused kernel has them too
        sizes += [(nc * hs - (hs - 1) * (nc & 1), nr * vs - (vs - 1) * (nr & 1)) for nc, nr in ((1, 9), (2, 7), (3, 9), (9, 1), (7, 2), (9, 3))]
        for w, h in sizes:
            for pname, pat in patterns.items():
                luma, inverted = ("y0", "y255", "ynoise")[i % 3], (i // 3) & 1
                (lh, lw), (ch, cw) = shapes(w, h, samp)[:2]
                y, x = np.mgrid[0:8 * ch, 0:8 * cw]
                cb = np.where(pat(x, y), 383, -384)  # 511 and -256 as pixel values: they saturate at 255 and 0 whatever the IDCT's last bit
                cr = -1 - cb if inverted else cb
                ysamp = {"y0": np.full((8 * lh, 8 * lw), -384), "y255": np.full((8 * lh, 8 * lw), 383)}.get(luma)
                if ysamp is None:
                    # under noise the chroma levels are 0..3 and 252..255, not saturated: 0 and 255 alone cannot tell the upsamplers'
                    # rounding constants apart ((3 * 0 + 255 + 1) >> 2 = (3 * 0 + 255 + 2) >> 2), sums of every residue modulo 4 and 16 can
                    ysamp = rng.integers(-384, 384, (8 * lh, 8 * lw))
                    cb = np.where(pat(x, y), 124 + rng.integers(0, 4, cb.shape), -128 + rng.integers(0, 4, cb.shape))
                    cr = np.where(pat(x, y) ^ inverted, 124 + rng.integers(0, 4, cb.shape), -128 + rng.integers(0, 4, cb.shape))
                one = np.ones(64)
                blocks = [fdct_quantised(p, one) for p in (ysamp, cb, cr)]
                _baseline(files, f"chroma_edges/{sname}_{w}x{h}_{pname}_{luma}_{'inv' if inverted else 'same'}", blocks, _flat_q(1), w, h, samp,
                          restart_interval=(0, 0, 0, 4)[i % 4])
                i += 1


@functools.lru_cache(maxsize=None)
def corpus(seed=20260):
    rng = np.random.default_rng(seed)
    files = {}
    _impulse(files)
    _dc_sweep(files)
    _overshoot(files, rng)
    _random_heavy(files, rng)
    _dc_pred(files, rng)
    _prog_extreme(files, rng)
    _chroma_edges(files, rng)
    return files


def klass(name):
    return name.split("/")[0]
