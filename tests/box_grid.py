"""Corpus of the multi-pass PDQ kernels' seam tests (csrc/pdq_kernels.hip: box_rows_tiled_kernel, box_cols_kernel, tail_sampled_kernel).

Three things, none of which needs a GPU:
  * a model of the kernels' CONTROL FLOW (which tile is loaded, which takes the fast path, how many steps it walks, which decimation
    samples leave it and from which LDS slot), written from the kernels and their comments.  It knows nothing of the arithmetic.  From it
    the seam classes of a line length are derived, and test_box_grid_cpu.py holds the geometry lists below to them;
  * the geometry lists and image contents that test_box_grid_gpu.py hashes;
  * a float32 restatement of one box pass in the one-loop form the tiled kernels rely on, and one of the four-phase form of
    box_one_d_float (pdqhash.rs:341-396) that it must equal.
"""
import functools
import os
import re
from collections import namedtuple

import numpy as np

TILE = 64       # columns per LDS tile, rows per chunk of the column pass, lines per workgroup
HIST = 8        # BT_HIST: slots of the previous tile kept in front of the current one
SAMPLES = 64    # decimate_float keeps 64 columns and 64 rows


def stream_min_images():
    """RPH_STREAM_MIN_IMAGES (csrc/rph_internal.h), the call size from which automatic dispatch leaves the multi-pass kernels for the
    streaming one; include/rupphash.h documents it under rph_pdq_set_kernel ("from 384 images per call")."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rupphash_amd", "csrc", "rph_internal.h")
    with open(path) as f:
        return int(re.search(r"constexpr\s+uint32_t\s+RPH_STREAM_MIN_IMAGES\s*=\s*(\d+)\s*;", f.read()).group(1))


# ---------------------------------------------------------------------------------------------------------------------------------
# control-flow model
# ---------------------------------------------------------------------------------------------------------------------------------
Geo = namedtuple("Geo", "len win half lead total")
Sample = namedtuple("Sample", "j col step slot")  # sample j = column `col` of the line, emitted by step `step` of its tile from slot `slot`
Tile = namedtuple("Tile", "c0 loaded prefetched fetches_next fast steps extra samples")


def box_geo(length, win=None):
    """box_geo() of the kernels: the window (ceil(len / 64) unless given) clamped to 1..max(len, 1), half = (win + 2) / 2, lead = half - 1"""
    if win is None:
        win = (length + TILE - 1) // TILE
    win = max(1, min(win, max(length, 1)))
    half = (win + 2) // 2
    return Geo(length, win, half, half - 1, length + half - 1)


def sample_pos(j, length):
    return ((2 * j + 1) * length) // (2 * SAMPLES)


def line_tiles(length):
    """The tiles box_rows_tiled_kernel<., true> walks along a line of `length` columns -- and, read as 64-row chunks, the chunks of
    tail_sampled_kernel along a column of `length` rows (same loop bounds, same history; it has no fast path and no prefetch).
    A sample whose column is kept more than once (length < 64) appears once per keeping."""
    g = box_geo(length)
    tiles, nxt = [], 0
    for c0 in range(0, g.total, TILE):
        steps = min(TILE, g.total - c0)
        samples = []
        while nxt < SAMPLES and sample_pos(nxt, length) + g.lead < c0 + steps:
            col = sample_pos(nxt, length)
            s = col + g.lead - c0
            assert 0 <= s < steps, (length, nxt, s)  # a sample is emitted by the tile its step falls in, never later
            samples.append(Sample(nxt, col, s, s - g.win))
            nxt += 1
        tiles.append(Tile(c0=c0, loaded=c0 < length, prefetched=0 < c0 < length, fetches_next=c0 + TILE < length,
                          fast=c0 >= g.win and c0 + TILE <= length, steps=steps, extra=c0 >= length, samples=tuple(samples)))
    assert nxt == SAMPLES, length
    return g, tiles


def has_extra_tile(length):
    g = box_geo(length)
    return (length + g.lead - 1) // TILE > (length - 1) // TILE


def row_classes(w):
    """seam classes of the row pass at line length w"""
    g, tiles = line_tiles(w)
    out = {f"window {g.win}"}
    loaded = [t for t in tiles if t.loaded]
    if w < TILE:
        out.add("one partial tile")
        assert g.win == 1 and g.lead == 0 and len(tiles) == 1
        if len({s.col for s in tiles[0].samples}) < SAMPLES:
            out.add("several samples on one column")
    if w == TILE:
        out.add("exactly one tile")
    if len(loaded) == 2 and not any(t.fast for t in tiles):
        out.add("partial second tile, no fast path")
    if any(t.fast for t in tiles):
        out.add("fast tile")
    if w % TILE:
        out.add("columns clamped in the last fetch")
    for t in tiles:
        if t.extra:
            out.add(f"extra tile of {t.steps} steps")
            if t.samples:
                out.add("sample from the extra tile")
        if not t.samples:
            out.add("tile without a sample")
        if len(t.samples) == SAMPLES:
            out.add("tile with all 64 samples")
        for s in t.samples:
            if s.slot in (-HIST, -1, 0):
                out.add(f"sample from slot {s.slot}")
            if s.step in (0, TILE - 1):
                out.add(f"sample at step {s.step}")
            out.add("sample in a fast tile" if t.fast else "sample in a slow tile")
    return out


ROW_CLASSES = (["one partial tile", "several samples on one column", "exactly one tile", "partial second tile, no fast path", "fast tile",
                "columns clamped in the last fetch", "sample from the extra tile", "tile without a sample", "tile with all 64 samples",
                "sample in a fast tile", "sample in a slow tile"]
               + [f"extra tile of {k} steps" for k in (1, 2, 3, 4)] + [f"sample from slot {k}" for k in (-HIST, -1, 0)]
               + [f"sample at step {k}" for k in (0, TILE - 1)] + [f"window {k}" for k in range(1, 9)])


def col_classes(h):
    """seam classes of tail_sampled_kernel (the second column pass on the kept columns, 64 rows at a time) at column length h"""
    g, chunks = line_tiles(h)
    out = set()
    kept = {}
    for c in chunks:
        for s in c.samples:
            kept[s.col] = kept.get(s.col, 0) + 1
    if h < TILE:
        if 2 in kept.values():
            out.add("a row kept twice")
        if max(kept.values()) >= 3:
            out.add("a row kept three or more times")
    if h == TILE:
        out.add("exactly one chunk")
    if TILE < h < 2 * TILE:
        out.add("partial second chunk")
    if h <= 4:
        out.add(f"h = {h}")
    for c in chunks:
        if c.extra:
            out.add("extra chunk after a full one" if h % TILE == 0 else "extra chunk after a partial one")
            if c.samples:
                out.add("sample from the extra chunk")
    return out


COL_CLASSES = ["a row kept twice", "a row kept three or more times", "exactly one chunk", "partial second chunk", "extra chunk after a full one",
               "extra chunk after a partial one", "sample from the extra chunk"]
THUMB_COL_CLASSES = [f"h = {k}" for k in (1, 2, 3, 4)]  # only a thumbnail can be that thin


def cols_kernel_classes(h):
    """box_cols_kernel walks a column with box_one_d: its bulk (phase 3, h - win steps) runs eight steps at a time, the rest one by one"""
    g = box_geo(h)
    phase_3 = h - g.win if h > g.win else 0
    out = {f"bulk remainder {phase_3 % 8}"}
    if phase_3 < 8:
        out.add("bulk shorter than one unrolled round")
    return out


COLS_KERNEL_CLASSES = [f"bulk remainder {k}" for k in range(8)] + ["bulk shorter than one unrolled round"]


def witnesses(lengths, classes_of):
    """class -> sorted lengths of `lengths` that have it"""
    out = {}
    for n in sorted(set(lengths)):
        for c in classes_of(n):
            out.setdefault(c, []).append(n)
    return out


def batch_blocks(n, h):
    """the workgroups of box_rows_tiled_kernel over the n * h lines of a call: (first line, lines, first image, last image)"""
    lines = n * h
    return [(l0, min(TILE, lines - l0), l0 // h, (min(l0 + TILE, lines) - 1) // h) for l0 in range(0, lines, TILE)]


# ---------------------------------------------------------------------------------------------------------------------------------
# geometries (w, h)
# ---------------------------------------------------------------------------------------------------------------------------------
SMALL = [5, 6, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 66, 71, 72, 73, 95, 96, 97, 126, 127]  # the range only these kernels serve
LARGE = [128, 129, 191, 192, 193, 255, 256, 257, 319, 320, 321, 382, 383, 384, 385, 446, 447, 448, 449, 508, 509, 510, 511, 512]


def _grid():
    g = []
    for a in SMALL:
        g += [(a, a), (a, 64), (64, a), (a, 127), (127, a), (a, 300), (300, a), (a, 512), (512, a)]
    for b in LARGE:
        g += [(b, 37), (37, b), (b, 200), (200, b)]
    g.append((512, 512))  # only under the modes that keep it off the fused kernel, and under the default for the comparison with them
    return sorted(set(g))


GRID = _grid()
GRID_WIDTHS = sorted({w for w, _ in GRID})


def grid_heights(w):
    return [h for gw, h in GRID if gw == w]


# colour (SRC = 3): every class of the row axis once more, a handful of heights
_COLOUR_W = [5, 6, 9, 17, 33, 63, 64, 65, 97, 127, 128, 129, 191, 192, 193, 255, 256, 257, 319, 320, 321, 382, 383, 384, 385, 446, 447, 448, 449, 509, 510,
             511, 512]
_COLOUR_H = [5, 37, 64, 65, 127, 9, 100]
COLOUR_GRID = [(w, _COLOUR_H[i % len(_COLOUR_H)]) for i, w in enumerate(_COLOUR_W)] + [(37, 300), (100, 512), (64, 64), (200, 192), (40, 256), (512, 509),
                                                                                        (512, 512)]

# batch seams: workgroups of 64 consecutive lines of n * h
BATCH_H, BATCH_W, BATCH_N = [5, 37, 63, 65, 100], [40, 100], [1, 2, 3, 7, 13, 64, 65, 129]
BATCH_COLOUR_N = [13, 65]

# sources whose <= 512 px thumbnail has a side no caller can pass (1..4) or one at a seam of the grid above: (w, h) -> thumbnail (w, h)
THUMBS = {(2048, 5): (512, 1), (1024, 5): (512, 2), (1024, 7): (512, 3), (1024, 9): (512, 4), (1024, 10): (512, 5), (1024, 126): (512, 63),
          (1024, 128): (512, 64), (1024, 130): (512, 65), (1024, 254): (512, 127)}
THUMBS.update({(h, w): (nh, nw) for (w, h), (nw, nh) in list(THUMBS.items())})


# ---------------------------------------------------------------------------------------------------------------------------------
# contents
# ---------------------------------------------------------------------------------------------------------------------------------
CONTENT_NAMES = ["noise", "gradient", "black", "white", "sparse points", "checkerboard", "32x32 blocks", "step at w/3"]


def contents(rng, h, w):
    """The 8 images of test_stream_gpu.contents at any size from 1 x 1: noise, a gradient, flat black / white, sparse points on black (tiny
    rounding residues run along whole lines), a period-1 checkerboard, 32 x 32 blocks, a step.  The order is fixed: neighbouring lines of a
    workgroup that straddles images carry different data."""
    imgs = rng.integers(0, 256, (8, h, w), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    imgs[1] = ((xx * 200) // max(w - 1, 1) + (yy * 55) // max(h - 1, 1)).astype(np.uint8)
    imgs[2] = 0
    imgs[3] = 255
    imgs[4] = 0
    npts = min(40, h * w)
    pts = rng.integers(0, h * w, npts)
    imgs[4].reshape(-1)[pts] = rng.integers(1, 256, npts, dtype=np.uint8)
    imgs[5] = (((xx + yy) & 1) * 255).astype(np.uint8)
    blocks = rng.integers(0, 256, ((h + 31) // 32, (w + 31) // 32), dtype=np.uint8)
    imgs[6] = np.kron(blocks, np.ones((32, 32), np.uint8))[:h, :w]
    imgs[7] = np.where(xx < w // 3, 250, 3).astype(np.uint8)
    return imgs


def luma601(r, g, b):
    return (299 * r + 587 * g + 114 * b + 500) // 1000


@functools.lru_cache(maxsize=None)
def luma_residue_triples(per_residue=96):
    """(r, g, b) triples whose 299 r + 587 g + 114 b + 500 falls on k * 1000 - 1, k * 1000 and k * 1000 + 1 -- where the integer division of
    to_luma601 decides -- found by enumeration: {-1: [...], 0: [...], 1: [...]}, `per_residue` of each, spread over the whole range of r"""
    found = {-1: [], 0: [], 1: []}
    g, b = np.mgrid[0:256, 0:256]
    gb = 587 * g + 114 * b + 500
    for r in range(256):
        v = (299 * r + gb) % 1000
        for res, key in ((999, -1), (0, 0), (1, 1)):
            gg, bb = np.nonzero(v == res)
            found[key] += [(r, int(y), int(x)) for y, x in zip(gg[::61], bb[::61])]
    out = {}
    for key, lst in found.items():
        step = max(len(lst) // per_residue, 1)
        out[key] = lst[::step][:per_residue]
    return out


def residue_image(h, w):
    """an (h, w, 3) image made only of luma_residue_triples, the three residues side by side along every row"""
    t = luma_residue_triples()
    table = np.array([t[(-1, 0, 1)[i % 3]][(i // 3) % len(t[0])] for i in range(3 * len(t[0]))], np.uint8)
    idx = (np.arange(h)[:, None] * 7 + np.arange(w)[None, :]) % len(table)
    return table[idx]


def colour_contents(rng, h, w, ch):
    """9 images of 3 or 4 channels: the 8 contents with the channels rolled against each other (so that R, G and B differ at every pixel
    that is not flat), and the luma residue image.  Alpha bytes differ from pixel to pixel and are never zero."""
    base = contents(rng, h, w)
    imgs = np.zeros((9, h, w, ch), np.uint8)
    imgs[:8, ..., 0] = base
    imgs[:8, ..., 1] = np.roll(base, 1, axis=2)
    imgs[:8, ..., 2] = np.roll(base, 1, axis=1)
    imgs[0, ..., :3] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    imgs[8, ..., :3] = residue_image(h, w)
    if ch == 4:
        imgs[..., 3] = (1 + (np.arange(9 * h * w) * 37) % 255).astype(np.uint8).reshape(9, h, w)
    return imgs


def embed(imgs, row_pad, image_gap, lead=0, fill=0xA5):
    """images (n, h, w[, ch]) in one byte buffer with `row_pad` bytes behind every row, `image_gap` behind every image and `lead` bytes in
    front; the filler is not zero.  Returns (buffer, row_stride, image_stride)."""
    n, h = imgs.shape[:2]
    row = int(np.prod(imgs.shape[2:]))
    row_stride = row + row_pad
    image_stride = row_stride * h + image_gap
    buf = np.full(lead + n * image_stride, fill, np.uint8)
    view = buf[lead:].reshape(n, image_stride)[:, :row_stride * h].reshape(n, h, row_stride)
    view[:, :, :row] = imgs.reshape(n, h, row)
    return buf, row_stride, image_stride


# ---------------------------------------------------------------------------------------------------------------------------------
# float32 restatements of one box pass; x: (lines, len) float32, all lines walked in step
# ---------------------------------------------------------------------------------------------------------------------------------
def box_one_loop(x, win):
    """The form the tiled kernels use (the comment in front of BT_HIST), one loop over t = index of the incoming sample:
    t < len: sum += in[t] (cur += 1 while t < win);  t >= win: sum -= in[t - win] (cur -= 1 once t >= len);  t >= lead: emit sum / cur."""
    x = np.asarray(x, np.float32)
    length = x.shape[1]
    g = box_geo(length, win)
    out = np.zeros_like(x)
    s = np.zeros(x.shape[0], np.float32)
    cur = np.float32(0)
    one = np.float32(1)
    for t in range(g.total):
        if t < length:
            s = s + x[:, t]
            if t < g.win:
                cur = cur + one
        if t >= g.win:
            s = s - x[:, t - g.win]
            if t >= length:
                cur = cur - one
        if t >= g.lead:
            out[:, t - g.lead] = s / cur
    return out


def box_four_phase(x, win):
    """box_one_d_float as the reference states it (pdqhash.rs:341-396): fill without output, fill with output, slide, drain"""
    x = np.asarray(x, np.float32)
    length = x.shape[1]
    g = box_geo(length, win)
    phase_1, phase_2, phase_3, phase_4 = g.half - 1, g.win - g.half + 1, max(length - g.win, 0), g.half - 1
    out = np.zeros_like(x)
    s = np.zeros(x.shape[0], np.float32)
    cur = np.float32(0)
    one = np.float32(1)
    li = ri = oi = 0
    for _ in range(phase_1):
        s = s + x[:, ri]
        cur = cur + one
        ri += 1
    for _ in range(phase_2):
        s = s + x[:, ri]
        cur = cur + one
        out[:, oi] = s / cur
        ri += 1
        oi += 1
    for _ in range(phase_3):
        s = s + x[:, ri]
        s = s - x[:, li]
        out[:, oi] = s / cur
        li += 1
        ri += 1
        oi += 1
    for _ in range(phase_4):
        s = s - x[:, li]
        cur = cur - one
        out[:, oi] = s / cur
        li += 1
        oi += 1
    return out


def buffer64_one_loop(luma):
    """generate_pdq_from_luma up to its 64 x 64 buffer with box_one_loop: two rounds of rows then columns, then decimate_float"""
    p = np.asarray(luma, np.float32)
    h, w = p.shape
    for _ in range(2):
        p = box_one_loop(p, (w + 63) // 64)
        p = np.ascontiguousarray(box_one_loop(np.ascontiguousarray(p.T), (h + 63) // 64).T)
    rows = [sample_pos(i, h) for i in range(SAMPLES)]
    cols = [sample_pos(j, w) for j in range(SAMPLES)]
    return p[np.ix_(rows, cols)]


def probe_lines(rng, length):
    """lines on which a wrong order of the one loop's operations shows: sparse (one point, a point at either end), flat, saturated, a
    step, and noise"""
    x = np.zeros((8, length), np.float32)
    x[0, length // 2] = 255
    x[1, 0] = 1
    x[2, length - 1] = 3
    x[3] = 255
    x[4] = 77
    x[5, length // 3:] = 250
    x[6] = rng.integers(0, 256, length)
    x[7] = rng.integers(0, 256, length) * (rng.integers(0, 8, length) == 0)
    return x
