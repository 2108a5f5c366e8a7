"""Corpus of the streaming PDQ kernels' seam tests (csrc/pdq_stream.hip: pdq_stream_kernel; csrc/pdq_ragged.hip: pdq_stream_ragged_kernel;
both run the stages of csrc/pdq_stream_stages.hpp).

Three things, none of which needs a GPU or the oracle:
  * a plain-Python restatement of the GEOMETRY of one axis, written from st_geo, st_emit_mask, the flush rule of the strip loop and the
    kept-row rule of the band loop.  Every one of these is decided by W alone or by H alone, so the kernel has 385 + 385 behaviours,
    not 385^2.  The model only accounts for coverage (test_stream_grid_cpu.py holds the sweep lists below to it); it knows nothing of
    the arithmetic and never judges a GPU result;
  * the sweep lists test_stream_grid_gpu.py hashes: two pairings of every width with every height, and the rare widths against the
    rare heights;
  * the image contents, seeded by (w, h, kind).
"""
import functools
from collections import namedtuple

import numpy as np

LO, HI = 128, 512           # the sides the streaming kernels take
SIDES = HI - LO + 1         # 385
STRIP = 64                  # columns per strip
BAND = 56                   # ST_BAND: recurrence steps (rows) per band
FILE = 32                   # kept columns the register file holds (f32x32 smp), kept rows edge[] holds
SAMPLES = 64                # decimate_float keeps 64 columns and 64 rows (pdqhash.rs:428-443)


# ---------------------------------------------------------------------------------------------------------------------------------
# geometry model
# ---------------------------------------------------------------------------------------------------------------------------------
Axis = namedtuple("Axis", "len win lead a")
Width = namedtuple("Width", "W win lead a ns_b ns_c emit per_strip flushes past")
Height = namedtuple("Height", "H win lead nb per_band steady")


def axis(n):
    """window = ceil(n / 64) (pdqhash.rs:246-247); half = (win + 2) / 2, lead = half - 1 steps before the first output, a = win - half
    (pdqhash.rs:351-357): output o is the mean of inputs o - a .. o + lead and leaves the recurrence at step o + lead"""
    win = (n + 63) // 64
    half = (win + 2) // 2
    return Axis(n, win, half - 1, win - half)


def sample_pos(j, n):
    """decimate_float's source index of sample j along an axis of n (pdqhash.rs:435, :439)"""
    return ((2 * j + 1) * n) // (2 * SAMPLES)


@functools.lru_cache(maxsize=None)
def width_model(W):
    """st_geo and the strip loop along a row of W pixels: the strips that hold pixels (ns_b) and the strips the row recurrence walks
    (ns_c); the step at which each of the 64 kept columns leaves the recurrence (st_emit_mask); how many fall into each strip; the
    `cnt` of every D pass of a band (a pass runs after strip s when the register file could not take strip s + 1's kept columns as
    well, cnt + popcount(em) > 32, and after the last strip); the emitted steps past the last pixel (st_c_stage's t > W - 1)."""
    ax = axis(W)
    ns_b = (W + 63) // 64
    ns_c = ((127 * W) // 128 + ax.lead) // 64 + 1
    emit = tuple(sample_pos(j, W) + ax.lead for j in range(SAMPLES))
    per_strip = [0] * ns_c
    for t in emit:
        per_strip[t // STRIP] += 1  # (an emit step past the last walked strip would raise here)
    flushes, cnt = [], 0
    for s in range(ns_c):
        cnt += per_strip[s]
        nxt = per_strip[s + 1] if s + 1 < ns_c else 0
        if cnt > 0 and (s == ns_c - 1 or cnt + nxt > FILE):
            flushes.append(cnt)
            cnt = 0
    return Width(W, ax.win, ax.lead, ax.a, ns_b, ns_c, emit, tuple(per_strip), tuple(flushes), sum(t > W - 1 for t in emit))


@functools.lru_cache(maxsize=None)
def height_model(H):
    """st_geo and the band loop along a column of H pixels: bands of 56 steps of the pass-1 column recurrence; kept row ri leaves the
    pass-2 column recurrence at band step ri + 2 lead - T0, so a band keeps the rows with ri + 2 lead in [T0, T0 + 56); a band is
    steady when every one of its steps divides by the full window (T0 >= win - 1 and T0 + 55 <= H - 1)."""
    ax = axis(H)
    nb = (H + 2 * ax.lead + BAND - 1) // BAND
    per_band = [0] * nb
    for i in range(SAMPLES):
        per_band[(sample_pos(i, H) + 2 * ax.lead) // BAND] += 1
    steady = tuple(BAND * k >= ax.win - 1 and BAND * k + BAND - 1 <= H - 1 for k in range(nb))
    return Height(H, ax.win, ax.lead, nb, tuple(per_band), steady)


def band_cursor(H):
    """the band loop's own bookkeeping, as the kernels write it: `ni` (next kept row) at the start of every band, advanced after a band by
    `while ni < 64 and pos(ni) + 2 lead < T0 + 56`; and the rows a D pass of that band emits (it starts at ni and takes every step
    whose row is the next kept one).  Must agree with height_model's per_band."""
    m = height_model(H)
    ni, starts, emitted = 0, [], []
    for k in range(m.nb):
        T0 = BAND * k
        starts.append(ni)
        n, got = ni, 0
        for step in range(BAND):
            if n < SAMPLES and T0 + step - 2 * m.lead == sample_pos(n, H):
                n, got = n + 1, got + 1
        emitted.append(got)
        while ni < SAMPLES and sample_pos(ni, H) + 2 * m.lead < T0 + BAND:
            ni += 1
        assert ni == n, (H, k)  # the cursor lands where the pass stopped
    return starts, emitted, ni


def empty_last_band(H):
    """the last band keeps no row: it exists only for the trailing 2 lead recurrence steps"""
    return height_model(H).per_band[-1] == 0


def two_trailing_bands(H):
    """the last two bands both take the divisor table (neither is steady)"""
    s = height_model(H).steady
    return len(s) >= 2 and not s[-1] and not s[-2]


def one_more_strip(W):
    """ns_c = ns_b + 1: a strip past the last pixel, through which the row recurrence only subtracts"""
    m = width_model(W)
    return m.ns_c == m.ns_b + 1


ALL = range(LO, HI + 1)


def reached(geoms):
    """what the model tells apart among the geometries (w, h) of `geoms`: the behaviours of their widths and of their heights"""
    ws, hs = {w for w, _ in geoms}, {h for _, h in geoms}
    return {
        "flush patterns": {width_model(W).flushes for W in ws},
        "strip distributions": {width_model(W).per_strip for W in ws},
        "band distributions": {height_model(H).per_band for H in hs},
        "empty last band": {H for H in hs if empty_last_band(H)},
        "two trailing bands": {H for H in hs if two_trailing_bands(H)},
        "one more strip": {W for W in ws if one_more_strip(W)},
        "steps past the last pixel": {W for W in ws if width_model(W).past},
    }


def census():
    """the same over all 385 widths and heights"""
    return reached([(n, n) for n in ALL])


def widths_of_pattern():
    """flush pattern -> the widths that have it"""
    out = {}
    for W in ALL:
        out.setdefault(width_model(W).flushes, []).append(W)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# sweep lists, (w, h)
# ---------------------------------------------------------------------------------------------------------------------------------
def _pairing(p, c):
    return [(LO + k, LO + (k * p + c) % SIDES) for k in range(SIDES)]


# p coprime to 385 = 5 * 7 * 11: every height once.  103 - 233 = -130 is a multiple of 5 and 1 - 0 is not: k (103 - 233) = 1 (mod 385)
# has no solution, so no geometry is in both lists.  Both p are > 64: the heights of neighbours differ in window almost everywhere.
PAIRING_A = _pairing(103, 0)
PAIRING_B = _pairing(233, 1)

RAGGED_STEP = 89  # (coprime to 385, > 64 and < 385 - 64) the order of a list in a ragged call: neighbours 89 widths apart, so of different window


def ragged_order(geoms):
    assert len(geoms) == SIDES
    return [geoms[(i * RAGGED_STEP) % SIDES] for i in range(SIDES)]


# widths whose flush pattern no other width has (test_stream_grid_cpu.py checks that against the model) ...
UNIQUE_PATTERN_WIDTHS = [179, 187, 194, 204, 215, 227, 327, 472]
# ... one width of each family of neighbours that share a pattern of their own: 180-182, 228-233, 241-246 ...
PATTERN_FAMILIES = {181: range(180, 183), 230: range(228, 234), 243: range(241, 247)}
# ... and the widths at which ns_c = ns_b + 1
CROSS_WIDTHS = UNIQUE_PATTERN_WIDTHS + sorted(PATTERN_FAMILIES) + sorted(W for W in ALL if one_more_strip(W))


def _cross_heights():
    """every height whose last band is empty, and per window the first height that ends in two non-steady bands (and is not among the
    former already)"""
    hs = sorted(H for H in ALL if empty_last_band(H))
    for win in range(2, 9):
        two = [H for H in ALL if axis(H).win == win and two_trailing_bands(H)]
        fresh = [H for H in two if H not in hs]
        if fresh:
            hs.append(fresh[0])
    return hs


CROSS_HEIGHTS = _cross_heights()
# thinned to every other cell of the widths x heights table: a checkerboard, so that every width still meets half the heights and
# every height half the widths
CROSS = [(w, h) for i, w in enumerate(CROSS_WIDTHS) for j, h in enumerate(CROSS_HEIGHTS) if (i + j) % 2 == 0]


# ---------------------------------------------------------------------------------------------------------------------------------
# contents
# ---------------------------------------------------------------------------------------------------------------------------------
KINDS = ("a", "b", "c")
KIND_NAMES = {"a": "full-range noise over a gradient", "b": "sparse points on black", "c": "255 with sparse zeros"}


POINT_PEAK = 8  # what a seam point leaves in the 64 x 64 buffer, about: a gradient term of 3


def seam_points(w, h, rng):
    """[(row, column, value)] of content b.  The quality output is min(sum of truncated gradients / 90, 1) (pdqhash.rs:445-460): it says
    something only while that sum stays under 90, so the points are few and faint -- a point of value v leaves a peak of about
    v / (win_r win_c) in the 64 x 64 buffer, here POINT_PEAK -- and they lie where only the quality output looks: per D-pass boundary of
    the width (kept column `base` takes its left neighbour from edge[], not from a lane) one point on kept column base - 1 in the
    first kept row of a band and one on kept column base in another kept row; then the two corners and three points anywhere.  (Two
    passes of a window that reaches from o - a to o + lead weigh input o + lead - a most: that is where the point of a kept row or
    column goes.  Under the widest windows one pixel cannot leave such a peak: a block of n x n pixels does.)"""
    wm, hm = width_model(w), height_model(h)
    mass = POINT_PEAK * wm.win * hm.win
    n = 1
    while mass > 255 * n * n:
        n += 1
    v = mass // (n * n)
    band_starts = [sum(hm.per_band[:b]) for b in range(hm.nb) if hm.per_band[b]]

    def block(i, j):
        y0, x0 = sample_pos(i, h) + hm.lead - (hm.win - hm.lead - 1), sample_pos(j, w) + wm.lead - wm.a
        return [(min(y0 + dy, h - 1), min(x0 + dx, w - 1), v) for dy in range(n) for dx in range(n)]

    pts, base = [], 0
    for cnt in wm.flushes[:-1]:
        base += cnt
        i1 = band_starts[int(rng.integers(0, len(band_starts)))]
        i2 = (i1 + 1 + int(rng.integers(0, SAMPLES - 1))) % SAMPLES
        pts += block(i1, base - 1) + block(i2, base)
    pts += [(0, 0, 1 + v // 4), (h - 1, w - 1, 1 + v // 3)]
    pts += [(int(rng.integers(0, h)), int(rng.integers(0, w)), int(rng.integers(1, v + 1))) for _ in range(3)]
    return pts


def image(w, h, kind, channel=0):
    """(h, w) uint8, seeded by (w, h, kind[, channel]):
    a  a gradient along both axes under noise of the full range: every window sum differs from its neighbours';
    b  sparse points on black (seam_points): the sums are tiny, so the rounding residues of the running sums travel along whole rows and
       columns and across every strip and band hand-off, and the quality stays below its clamp;
    c  255 with sparse zeros (one pixel in about 300, and two corners): the largest sums a window can hold, 8 x 255."""
    rng = np.random.default_rng([w, h, KINDS.index(kind), channel])
    if kind == "a":
        yy, xx = np.mgrid[0:h, 0:w]
        grad = (xx * 150) // (w - 1) + (yy * 70) // (h - 1) + 18
        img = np.clip(grad + rng.integers(-128, 129, (h, w)), 0, 255).astype(np.uint8)
    elif kind == "b":
        img = np.zeros((h, w), np.uint8)
        for y, x, v in seam_points(w, h, rng):
            img[y, x] = v
    else:
        n = max((w * h) // 300, 16)
        img = np.full((h, w), 255, np.uint8)
        img.reshape(-1)[rng.integers(0, h * w, n)] = 0
        img[0, 0] = img[-1, -1] = 0
    return img


def image_rgb(w, h, kind="a"):
    """(h, w, 3): the content of `kind` per channel, each channel with its own seed"""
    return np.stack([image(w, h, kind, ch) for ch in (1, 2, 3)], axis=2)
