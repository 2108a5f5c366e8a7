"""Coefficient vectors that no image produces but a cache file can hold (rph_coeff_record_decode hands back any 32 bits): NaNs, infinities,
subnormals, signed zeros, ties at the median's rank and pairs of values one key bit apart.  test_coeff_bits_cpu.py pins the corpus and
compares four host forms on it; test_coeff_bits_gpu.py runs from_coeffs_kernel and the grouping on it.  Everything is seeded and held as
uint32 bit patterns, so that no conversion on the way quiets a signalling NaN.

The order f32::total_cmp sorts by is the unsigned order of key = bits ^ (sign ? 0xFFFFFFFF : 0x80000000)."""
import functools
from collections import namedtuple

import numpy as np

SPECIALS = {
    "+qnan": 0x7FC00000, "-qnan": 0xFFC00000, "+snan": 0x7F800001, "-snan": 0xFF800001, "+nan-all-ones": 0x7FFFFFFF, "-nan-all-ones": 0xFFFFFFFF,
    "+inf": 0x7F800000, "-inf": 0xFF800000,
    "+min-subnormal": 0x00000001, "-min-subnormal": 0x80000001, "+max-subnormal": 0x007FFFFF, "-max-subnormal": 0x807FFFFF,
    "+min-normal": 0x00800000, "-min-normal": 0x80800000,
    "+0": 0x00000000, "-0": 0x80000000,
    "+max-finite": 0x7F7FFFFF, "-max-finite": 0xFF7FFFFF,
}
SIGN = np.uint32(0x80000000)
RADIX_A = 0xA2AAAAAA  # key of the float 0x22AAAAAA (exponent field 0x45): no single bit flip of it reaches exponent 0x00 or 0xFF
ADJACENT = {
    "1.0-and-successor": (0x3F800000, 0x3F800001), "two-smallest-subnormals": (0x00000001, 0x00000002), "+inf-and-+qnan": (0x7F800000, 0x7FC00000),
    "-qnan-and--inf": (0xFFC00000, 0xFF800000), "0-and-smallest-subnormal": (0x00000000, 0x00000001),
}

Vector = namedtuple("Vector", "name bits")  # bits: 256 uint32, row-major 16 x 16


def key_of(bits):
    bits = np.asarray(bits, np.uint32)
    return bits ^ np.where(bits >> 31, np.uint32(0xFFFFFFFF), SIGN)


def bits_of(key):
    key = np.asarray(key, np.uint32)
    return np.where(key >> 31, key ^ SIGN, ~key)


def _normal(rng):
    return rng.normal(0, 20, 256).astype(np.float32).view(np.uint32)


def _two_values(rng, lower_key, higher_key, n_lower):
    k = np.full(256, higher_key, np.uint32)
    k[:n_lower] = lower_key
    return bits_of(rng.permutation(k))


def vectors():
    rng = np.random.default_rng(1270)
    special = np.array(list(SPECIALS.values()), np.uint32)
    # ---- specials
    for t, k in enumerate(np.linspace(1, 200, 64).astype(int)):
        b = _normal(rng)
        b[rng.choice(256, k, replace=False)] = special[rng.integers(0, len(special), k)]
        yield Vector(f"normal-with-{k}-specials-{t}", b)
    for name, s in SPECIALS.items():
        yield Vector(f"all-{name}", np.full(256, s, np.uint32))
    r, c = np.divmod(np.arange(256), 16)
    where = {"even-rows": r % 2 == 0, "even-cols": c % 2 == 0, "even-rows-and-cols": (r % 2 == 0) | (c % 2 == 0)}
    for name, s in SPECIALS.items():
        for w, sel in where.items():  # the sign patterns of apply_sign flip exactly these positions
            b = _normal(rng)
            b[sel] = s
            yield Vector(f"{name}-on-{w}", b)
    # ---- rank boundary, in key space: `below` keys under a tie of `tie` equal keys, the rest above
    tie_key = int(key_of(np.float32(1.5).view(np.uint32)))
    for below in (126, 127, 128, 129):
        for tie in (1, 2, 100):
            above = 256 - below - tie
            k = np.concatenate([tie_key - 1 - rng.choice(1 << 20, below, replace=False), np.full(tie, tie_key),
                                tie_key + 1 + rng.choice(1 << 20, above, replace=False)]).astype(np.uint32)
            yield Vector(f"rank-{below}-below-tie-of-{tie}", bits_of(rng.permutation(k)))
    # ---- one pair per radix bit: two keys that agree above bit b
    for b in range(32):
        lo, hi = RADIX_A & ~(1 << b), RADIX_A | (1 << b)
        yield Vector(f"radix-bit-{b}-128-128", _two_values(rng, lo, hi, 128))  # median = the lower key: the bit is not set
        yield Vector(f"radix-bit-{b}-127-129", _two_values(rng, lo, hi, 127))  # median = the higher key
    for n_lower in (128, 127):  # the sign boundary itself: total_cmp orders -0.0 < +0.0, `>` does not
        yield Vector(f"minus-zero-plus-zero-{n_lower}-{256 - n_lower}", _two_values(rng, 0x7FFFFFFF, 0x80000000, n_lower))
    # ---- neighbours in the order: one key apart, or an infinity and the quiet NaN beyond it (only signalling NaNs lie between)
    for name, (x, y) in ADJACENT.items():
        kx, ky = sorted((int(key_of(x)), int(key_of(y))))
        for n_lower in (127, 128):
            yield Vector(f"{name}-{n_lower}-{256 - n_lower}", _two_values(rng, kx, ky, n_lower))
    # ---- positive magnitudes, all distinct: the four sign patterns have four medians
    # A flipped pattern's median is minus the smallest magnitude it flips.  The three patterns flip (even, even) + (even, odd), (even, even) +
    # (odd, even) and (even, odd) + (odd, even) positions, so the smallest of those three classes is the median of two of them: three
    # different medians with the identity's is the most there can be.  Under such a median a flipped pattern's hash is the pattern of the
    # unflipped positions itself, so the eight rows hold five different hashes.
    for t in range(6):
        b = np.abs(rng.normal(0, 20, 256).astype(np.float32)).view(np.uint32)
        assert len(np.unique(b)) == 256
        yield Vector(f"positive-distinct-{t}", b)
    for t in range(6):  # the same among the subnormals only: a compare that flushes them sees 256 zeros
        yield Vector(f"positive-distinct-subnormal-{t}", (1 + rng.choice(0x7FFFFF, 256, replace=False)).astype(np.uint32))


@functools.lru_cache(maxsize=None)
def corpus():
    """(names, bits (n, 256) uint32); .view(np.float32) of the bits is what the entry points take"""
    v = list(vectors())
    bits = np.stack([x.bits for x in v]).astype(np.uint32)
    bits.setflags(write=False)
    return [x.name for x in v], bits


# ---------------------------------------------------------------- the bit-level restatement
def signed(bits, neg_rows, neg_cols):
    """apply_sign on all 256 positions: an xor of the sign bit where exactly one of (row flips, column flips) holds; a row or a column
    flips when its index is even (its DCT frequency, index + 1, is odd)"""
    r, c = np.divmod(np.arange(256), 16)
    flip = (neg_rows & (r % 2 == 0)) ^ (neg_cols & (c % 2 == 0))
    return np.where(flip, bits ^ SIGN, bits).astype(np.uint32)


def median_bits(bits):
    """the value a sort by total_cmp puts at index 127"""
    return bits_of(np.sort(key_of(bits))[127])


def bit_rows(bits, neg_rows=False, neg_cols=False):
    s = signed(bits, neg_rows, neg_cols)
    med = np.array(median_bits(s), np.uint32)
    with np.errstate(invalid="ignore"):
        above = s.view(np.float32) > med.view(np.float32)  # IEEE `>`: false with a NaN on either side, -0 == +0, subnormals as they are
    return above.reshape(16, 16)  # [r][c] = bit c of row r


def pack(rows):
    """pack_bit_rows: row r -> hash[31 - 2r] (bits 0..7), hash[30 - 2r] (bits 8..15)"""
    words = (rows.astype(np.uint32) << np.arange(16, dtype=np.uint32)).sum(axis=1)
    out = np.zeros(32, np.uint8)
    for r in range(16):
        out[31 - 2 * r], out[30 - 2 * r] = words[r] & 0xFF, words[r] >> 8
    return out


def to_hash(bits):
    return pack(bit_rows(bits))


def dihedral(bits):
    ident, nc, nr, nb = bit_rows(bits), bit_rows(bits, neg_cols=True), bit_rows(bits, neg_rows=True), bit_rows(bits, True, True)
    return np.stack([pack(x) for x in (ident, nr.T, nb, nc.T, nc, nr, ident.T, nb.T)])
