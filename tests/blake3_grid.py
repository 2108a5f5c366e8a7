"""Corpus of the BLAKE3 kernels' seam tests (csrc/blake3_kernels.hip: b3_plan_kernel, b3_bytes_kernel, b3_fold_kernel, b3_pixels_kernel<1|3|4>,
b3_pixels_ragged_kernel).  Not a test module.

Three things, none of which needs a GPU:
  * a model of the kernels' CONTROL FLOW, restated from the .hip file: which thread of the plan kernel scans which strings and how the
    scan runs across lanes and waves; which wave of the grid-stride loop takes which group of which string, with how many chunks and
    whether it is the whole string; how many levels and rounds the fold kernel walks and where it carries an odd node; which of a pixel
    chunk's sixteen blocks take the aligned fast path, at which address & 3, and which are read pixel by pixel.  From it the seam classes of a
    call are derived, and test_blake3_grid_cpu.py holds the case lists below to them;
  * the same schedule executed on chaining values (wave_fold, fold_kernel): the tree the kernels build, which must be BLAKE3's;
  * the case lists that test_blake3_grid_gpu.py hashes.
"""
import functools
from collections import namedtuple

import numpy as np

import blake3_util as b3

CHUNK, BLOCK = b3.CHUNK_LEN, b3.BLOCK_LEN
WAVE = 64                        # lanes; GROUP_CHUNKS: chunks per wave
GROUP_BYTES = WAVE * CHUNK       # bytes per group of a byte string
PX_PER_CHUNK = CHUNK // 8        # RGBA16 pixels per chunk
GROUP_PX = WAVE * PX_PER_CHUNK   # pixels per group of an image
PLAN_THREADS = 1024              # b3_plan_kernel: one block
WAVES_PER_BLOCK = 4              # b3_bytes_kernel and the pixel kernels: 256 threads
KEY = b"whats the Elvish word for friend"
LAYOUTS = (1, 2, 3, 4, 17, 18, 19, 20)   # RPH_LAYOUT_*: channels + 16 for u16 samples
UNIFORM_CHANNELS = (1, 3, 4)


def groups_of(length):
    return -(-length // GROUP_BYTES) if length else 1


def chunks_of(length):
    return -(-length // CHUNK) if length else 1


# ---------------------------------------------------------------------------------------------------------------------------------
# byte strings: b3_plan_kernel, b3_bytes_kernel
# ---------------------------------------------------------------------------------------------------------------------------------
Plan = namedtuple("Plan", "n per s0 s1 sums wave_total group_first")


def plan(lengths):
    """b3_plan_kernel: thread t sums the groups of strings s0[t] .. s1[t], the sums are scanned across the lanes of a wave (shfl_up by 1, 2,
    .. 32) and over the 16 wave totals, and every thread writes group_first for its strings; thread 1023 writes group_first[n]"""
    n = len(lengths)
    g = np.array([groups_of(x) for x in lengths], np.int64)
    per = (n + PLAN_THREADS - 1) // PLAN_THREADS
    t = np.arange(PLAN_THREADS)
    lane, wv = t & 63, t >> 6
    s0 = np.minimum(n, t * per)
    s1 = np.minimum(n, s0 + per)
    sums = np.array([g[a:b].sum() for a, b in zip(s0, s1)], np.int64)
    x = sums.copy()
    d = 1
    while d < WAVE:
        y = np.roll(x, d)  # __shfl_up: lane l reads lane l - d (lanes below d read something they do not use)
        x = np.where(lane >= d, x + y, x)
        d *= 2
    wave_total = x[63::WAVE].copy()
    before = np.array([wave_total[:w].sum() for w in wv], np.int64)
    acc = before + x - sums
    first = np.full(n + 1, -1, np.int64)
    for k in range(PLAN_THREADS):
        a = acc[k]
        for s in range(s0[k], s1[k]):
            first[s] = a
            a += g[s]
    first[n] = before[PLAN_THREADS - 1] + x[PLAN_THREADS - 1]
    return Plan(n, per, s0, s1, sums, wave_total, first)


Waves = namedtuple("Waves", "waves cap total pass_no string k in_group whole")


def bytes_launch(n, total_bytes, cus):
    """(waves of the b3_bytes_kernel launch, cap) as rph_blake3_batch_dev sizes them"""
    cap = n + total_bytes // GROUP_BYTES + 1
    blocks = max(1, min((cap + WAVES_PER_BLOCK - 1) // WAVES_PER_BLOCK, cus * 16))
    return blocks * WAVES_PER_BLOCK, cap


def bytes_waves(lengths, cus):
    """b3_bytes_kernel: for every group g of the call its pass of the grid-stride loop, its string (the kernel's binary search in group_first),
    its number k within the string, the chunks the wave holds and whether that is the whole string"""
    n = len(lengths)
    first = plan(lengths).group_first
    waves, cap = bytes_launch(n, int(sum(lengths)), cus)
    total = int(min(first[n], cap))
    g = np.arange(total, dtype=np.int64)
    lo, hi = np.zeros(total, np.int64), np.full(total, n, np.int64)
    while (hi - lo > 1).any():
        go = hi - lo > 1
        mid = (lo + hi) // 2
        le = first[mid] <= g
        lo, hi = np.where(go & le, mid, lo), np.where(go & ~le, mid, hi)
    nch = np.array([chunks_of(x) for x in lengths], np.int64)[lo]
    k = g - first[lo]
    return Waves(waves, cap, total, g // waves, lo, k, np.minimum(WAVE, nch - k * WAVE), nch <= WAVE)


# ---------------------------------------------------------------------------------------------------------------------------------
# b3_fold_kernel
# ---------------------------------------------------------------------------------------------------------------------------------
Level = namedtuple("Level", "cnt next rounds carry_round root")


def fold_levels(cnt):
    """the levels b3_fold_kernel walks over `cnt` group values: `next` nodes written by `rounds` passes of the 64 lanes (i = lane, lane + 64,
    ..), the odd last node carried in pass carry_round (0: the level has no odd node), ROOT on the level that leaves one node"""
    out = []
    while cnt > 1:
        nxt = (cnt + 1) // 2
        out.append(Level(cnt, nxt, -(-nxt // WAVE), ((nxt - 1) // WAVE + 1) if cnt & 1 else 0, nxt == 1))
        cnt = nxt
    return out


def fold_classes(cnt):
    out = set()
    lv = fold_levels(cnt)
    for a in lv:
        out.add(f"fold level with {a.rounds} round{'s' if a.rounds > 1 else ''}")
        if a.carry_round:
            out.add(f"carry in round {a.carry_round}")
        if a.next > WAVE:
            out.add("in-place write of nodes[i] for i >= 64")
    if any(a.carry_round and b.carry_round for a, b in zip(lv, lv[1:])):
        out.add("carries on two levels running")
    return out


FOLD_CLASSES = (["fold level with 1 round", "fold level with 2 rounds", "fold level with 3 rounds", "in-place write of nodes[i] for i >= 64",
                 "carries on two levels running"] + [f"carry in round {r}" for r in (1, 2, 3)])


# ---------------------------------------------------------------------------------------------------------------------------------
# the schedule executed on chaining values: (8, N) uint32 arrays as in blake3_util
# ---------------------------------------------------------------------------------------------------------------------------------
def _parents(kw, base, left, right, root):
    n = left.shape[1]
    return b3.compress(np.repeat(kw[:, None], n, axis=1), np.concatenate([left, right], axis=0), np.zeros(n, np.uint64), BLOCK,
                       base | b3.PARENT | (b3.ROOT if root else 0))


def wave_fold(cv, cnt, root, kw, base):
    """wave_fold: node i in lane i of 64, `cnt` of them; every lane computes the parent of lanes min(2 l, 63) and min(2 l + 1, 63) and keeps
    it if 2 l + 1 < cnt, the left one otherwise; ROOT on the fold of two nodes when the group is the whole input.  Lane 0's value."""
    assert cv.shape == (8, WAVE)
    lane = np.arange(WAVE)
    while cnt > 1:
        l, r = cv[:, np.minimum(2 * lane, 63)], cv[:, np.minimum(2 * lane + 1, 63)]
        p = _parents(kw, base, l, r, root and cnt == 2)
        cv = np.where((2 * lane + 1 < cnt)[None, :], p, l)
        cnt = (cnt + 1) // 2
    return cv[:, 0].copy()


def fold_kernel(nodes, kw, base):
    """b3_fold_kernel on the (8, cnt) group values of one input, in place as the kernel does it: per level, per round of 64 lanes, read nodes
    2 i and 2 i + 1, write node i (or the digest on the last level)"""
    nodes = nodes.copy()
    cnt = nodes.shape[1]
    assert cnt > 1
    while True:
        nxt = (cnt + 1) // 2
        for r0 in range(0, nxt, WAVE):
            i = np.arange(r0, min(nxt, r0 + WAVE))
            l, r = nodes[:, 2 * i].copy(), nodes[:, np.minimum(2 * i + 1, cnt - 1)].copy()
            out = np.where((2 * i + 1 < cnt)[None, :], _parents(kw, base, l, r, nxt == 1), l)
            if nxt == 1:
                return out[:, 0].astype("<u4").tobytes()
            nodes[:, i] = out
        cnt = nxt


def model_digest(data, key=None):
    """the digest of a byte string as the kernels build it: chunk values, one wave_fold per group of 64 (idle lanes hold the key words),
    fold_kernel over the group values of an input of more than one group"""
    cv, kw, base = b3.chunk_cvs(data, key)
    nch = cv.shape[1]
    vals = []
    for c0 in range(0, nch, WAVE):
        part = cv[:, c0:c0 + WAVE]
        lanes = np.repeat(kw[:, None], WAVE, axis=1)
        lanes[:, :part.shape[1]] = part
        vals.append(wave_fold(lanes, part.shape[1], nch <= WAVE, kw, base))
    if nch <= WAVE:
        return vals[0].astype("<u4").tobytes()
    return fold_kernel(np.stack(vals, axis=1), kw, base)


# ---------------------------------------------------------------------------------------------------------------------------------
# seam classes of a byte-string call
# ---------------------------------------------------------------------------------------------------------------------------------
COUNT_CLASSES = [f"in-wave count {c} as root" for c in range(1, 65)] + [f"in-wave count {c}, not root" for c in range(1, 65)]
BLOCK_CLASSES = ([f"full block at address & 3 == {r}" for r in range(4)] + ["last block full", "last block of 1 byte", "last block of 63 bytes",
                                                                            "empty string"])
PASS_CLASSES = ["group in the second grid pass", "string straddling the grid pass"]
PLAN_CLASSES = (["plan thread with 0 strings", "plan thread with 1 string", "plan thread with 2 strings", "plan thread with 3 strings", "per = 1", "per = 2",
                 "per = 3", "multi-group string last in a thread range", "multi-group string first in a thread range", "multi-group string at lane 63",
                 "multi-group string at lane 0 of a later wave", "multi-group string in the last thread that has strings"])


def byte_classes(lengths, cus=256, start=0):
    """class -> witnesses of one call: strings as 'index:length', plan threads as 't<thread>'.  `start`: offsets[0] (the blob base is
    256-aligned, so it is the first string's address & 255)."""
    lengths = [int(x) for x in lengths]
    n = len(lengths)
    out = {}

    def add(c, s):
        out.setdefault(c, []).append(f"{s}:{lengths[s]}")

    wv = bytes_waves(lengths, cus)
    assert wv.total == sum(groups_of(x) for x in lengths)
    for whole in (True, False):
        for c in np.unique(wv.in_group[wv.whole == whole]):
            for s in np.unique(wv.string[(wv.whole == whole) & (wv.in_group == c)])[:8]:
                add(f"in-wave count {c} as root" if whole else f"in-wave count {c}, not root", s)
    p_lo, p_hi = np.full(n, 1 << 30), np.full(n, -1)
    np.minimum.at(p_lo, wv.string, wv.pass_no)
    np.maximum.at(p_hi, wv.string, wv.pass_no)
    for s in np.flatnonzero(p_hi >= 1)[:8]:
        add("group in the second grid pass", s)
    for s in np.flatnonzero(p_hi > p_lo):
        add("string straddling the grid pass", s)
    at = start
    for s, x in enumerate(lengths):
        if groups_of(x) > 1:
            for c in fold_classes(groups_of(x)):
                add(c, s)
        if x >= BLOCK:
            add(f"full block at address & 3 == {at & 3}", s)
        tail = x % BLOCK
        add("empty string" if x == 0 else "last block full" if tail == 0 else f"last block of {tail} byte{'s' if tail > 1 else ''}", s)
        at += x
    p = plan(lengths)
    out[f"per = {p.per}"] = [f"n={n}"]
    last_busy = max((t for t in range(PLAN_THREADS) if p.s1[t] > p.s0[t]), default=0)
    for t in range(PLAN_THREADS):
        k = int(p.s1[t] - p.s0[t])
        out.setdefault(f"plan thread with {k} string{'' if k == 1 else 's'}", []).append(f"t{t}")
        multi = [s for s in range(p.s0[t], p.s1[t]) if groups_of(lengths[s]) > 1]
        for s in multi:
            if s == p.s1[t] - 1:
                add("multi-group string last in a thread range", s)
            if s == p.s0[t]:
                add("multi-group string first in a thread range", s)
            if t & 63 == 63:
                add("multi-group string at lane 63", s)
            if t & 63 == 0 and t >= WAVE:
                add("multi-group string at lane 0 of a later wave", s)
            if t == last_busy:
                add("multi-group string in the last thread that has strings", s)
    return out


def merge(tables):
    """class -> witnesses over several calls, each witness prefixed with its call's name (a witness "-" is the call itself)"""
    out = {}
    for name, table in tables:
        for c, w in table.items():
            out.setdefault(c, []).extend(name if x == "-" else f"{name} {x}" if name else x for x in w)
    return out


def report(wit, wanted):
    return "\n".join(f"  {c}: {wit.get(c, [])[:6]}" + (f" (+{len(wit[c]) - 6})" if len(wit.get(c, [])) > 6 else "") for c in wanted)


# ---------------------------------------------------------------------------------------------------------------------------------
# byte-string case lists
# ---------------------------------------------------------------------------------------------------------------------------------
TAILS = (0, 1, 960, 961, 1023)  # k * 1024 - d ends on: a full chunk; a 63-byte block; one full block; 63 bytes; 1 byte


def _in_wave_lengths():
    out = []
    for k in range(1, WAVE + 1):
        out += [k * CHUNK - d for d in TAILS]                                                   # k chunks, the whole string
        out += [GROUP_BYTES + k * CHUNK - d for d in (TAILS[k % 5], TAILS[(k + 2) % 5])]       # k chunks in the second of two groups
    return [out[i] for i in np.random.default_rng(64).permutation(len(out))]


IN_WAVE_LENGTHS = _in_wave_lengths()
IN_WAVE_START = 3   # offsets[0] of the _dev form

FOLD_GROUPS = (2, 3, 5, 64, 65, 127, 128, 129, 131, 193, 257)


def fold_length(g):
    """a string of g groups whose last group holds (37 g mod 64) + 1 chunks and ends in a partial block"""
    return (g - 1) * GROUP_BYTES + ((g * 37) % WAVE) * CHUNK + 1 + (g % 3) * 31


FOLD_LENGTHS = [fold_length(g) for g in FOLD_GROUPS]

PLAN_SIZES = (1, 2, 1023, 1024, 1025, 2047, 2048, 2049)
PLAN_LONG = GROUP_BYTES + 1   # two groups, the second of one byte


def plan_lengths(n):
    """n strings of 0..3 bytes with two-group strings on the edges of the plan kernel's thread ranges: last of lane 63's range, first of
    the next wave's lane 0, last of lane 127's, the call's last string, and the first thread's last"""
    per = (n + PLAN_THREADS - 1) // PLAN_THREADS
    lengths = [(7 * s + n) % 4 for s in range(n)]
    s0 = lambda t: min(n, t * per)
    s1 = lambda t: min(n, s0(t) + per)
    for s in {s1(63) - 1, s0(64), s1(127) - 1, n - 1} | ({s1(0) - 1} if n > 2 else set()):
        if 0 <= s < n:
            lengths[s] = PLAN_LONG
    return lengths


GRID_PASS_CUS = (64, 256, 304)


def grid_pass_lengths(cus):
    """cus * 64 + 64 + 3 strings of 0..199 bytes -- more groups than the cus * 64 waves of the launch -- with one three-group string whose
    groups are cus * 64 - 1 (first pass), cus * 64 and cus * 64 + 1 (second pass)"""
    n = cus * 64 + 64 + 3
    lengths = np.random.default_rng(cus).integers(0, 200, n).tolist()
    lengths[cus * 64 - 1] = 2 * GROUP_BYTES + 777
    return lengths


def blob_of(lengths, seed, start=0):
    """(blob, offsets uint64): `start` filler bytes, then the strings, random bytes throughout"""
    off = np.concatenate([[start], start + np.cumsum(np.asarray(lengths, np.int64))]).astype(np.uint64)
    return np.random.default_rng(seed).integers(0, 256, int(off[-1]), dtype=np.uint8), off


def strings_of(blob, off):
    return [blob[int(a):int(b)].tobytes() for a, b in zip(off[:-1], off[1:])]


# ---------------------------------------------------------------------------------------------------------------------------------
# pixels: b3_pixels_kernel<CH> and layout_chunk<L> of b3_pixels_ragged_kernel walk a chunk the same way
# ---------------------------------------------------------------------------------------------------------------------------------
def layout_bytes(layout):
    """(channels, bytes per sample, bytes per pixel)"""
    ch, bps = layout & 15, 2 if layout > 16 else 1
    return ch, bps, ch * bps


def pixel_groups(w, h):
    """[(in_group, whole)] per wave of one image"""
    npx = w * h
    nch = -(-npx // PX_PER_CHUNK) if npx else 1
    return [(min(WAVE, nch - c0), nch <= WAVE) for c0 in range(0, nch, WAVE)]


Block = namedtuple("Block", "chunk bk fast bpx addr3 ends_row rows mid_row_chunk")


def pixel_walk(w, h, layout, row_stride, address):
    """The chunk loop of the pixel kernels for one image at byte address `address`: every block with its class, and the byte address of
    every pixel it reads, in the order the pixels enter the message (blocks, offsets)"""
    _, _, bpp = layout_bytes(layout)
    npx = w * h
    nch = -(-npx // PX_PER_CHUNK) if npx else 1
    blocks, offs = [], []
    for c in range(nch):
        p0 = c * PX_PER_CHUNK
        cpx = min(PX_PER_CHUNK, npx - min(npx, p0))
        nb = (cpx + 7) // 8 if cpx else 1
        y = p0 // w if w else 0
        x = p0 - y * w if w else 0
        mid = x != 0
        row = address + y * row_stride
        for bk in range(nb):
            bpx = min(8, cpx - min(cpx, bk * 8))
            if bpx == 8 and x + 8 <= w:
                p = row + x * bpp
                offs += [p + i * bpp for i in range(8)]
                x += 8
                ends = x == w
                if ends:
                    x, row = 0, row + row_stride
                blocks.append(Block(c, bk, True, 8, p & 3, ends, 1, mid))
            else:
                rows = set()
                for _ in range(bpx):
                    offs.append(row + x * bpp)
                    rows.add(row)
                    x += 1
                    if x == w:
                        x, row = 0, row + row_stride
                blocks.append(Block(c, bk, False, bpx, None, False, len(rows), mid))
    return blocks, np.array(offs, np.int64)


def layout_rgba16(samples, layout):
    """(npx, channels) samples -> the RGBA16 bytes of layout_words / px_words: u8 v widens as v * 257, gray goes into R, G and B, a missing
    alpha is 65535"""
    ch, bps, _ = layout_bytes(layout)
    s = samples.astype(np.uint32) * (257 if bps == 1 else 1)
    r = s[:, 0]
    g, b = (s[:, 1], s[:, 2]) if ch >= 3 else (r, r)
    a = s[:, 1] if ch == 2 else s[:, 3] if ch == 4 else np.full_like(r, 65535)
    return np.stack([r, g, b, a], axis=1).astype("<u2").tobytes()


def gather(buf, offs, layout):
    """the samples at the byte offsets `offs` of buf: (npx, channels)"""
    ch, bps, bpp = layout_bytes(layout)
    raw = buf[offs[:, None] + np.arange(bpp)[None, :]] if len(offs) else np.zeros((0, bpp), np.uint8)
    return np.ascontiguousarray(raw).view(np.uint16 if bps == 2 else np.uint8).reshape(len(offs), ch)


def pixel_classes(w, h, layout, row_stride, address):
    blocks, _ = pixel_walk(w, h, layout, row_stride, address)
    out = set()
    if w * h == 0:
        out.add("zero area")
    for b in blocks:
        if b.fast:
            out.add(f"fast block at address & 3 == {b.addr3}")
            if b.ends_row:
                out.add("fast block ending at the row end")
                if b.bk < 15 and any(o.chunk == b.chunk and o.bk == b.bk + 1 for o in blocks):
                    out.add("fast block ending at the row end, blocks behind it in the chunk")
        elif b.bpx:
            if b.bpx < 8:
                out.add(f"partial last block of {b.bpx} pixel{'s' if b.bpx > 1 else ''}")
            if b.bpx == 8 and b.rows == 2:
                out.add("slow block crossing one row end")
            if b.rows >= 3:
                out.add("slow block holding several rows")
        if b.chunk and b.bk == 0:
            out.add("chunk starting mid-row" if b.mid_row_chunk else "chunk starting at a row start")
    return out


def pixel_block_classes(wide):
    return ([f"fast block at address & 3 == {r}" for r in ((0, 2) if wide else (0, 1, 2, 3))]
            + ["fast block ending at the row end", "fast block ending at the row end, blocks behind it in the chunk", "slow block crossing one row end",
               "slow block holding several rows", "chunk starting mid-row", "chunk starting at a row start", "zero area"]
            + [f"partial last block of {k} pixel{'s' if k > 1 else ''}" for k in range(1, 8)])


PIXEL_COUNT_CLASSES = COUNT_CLASSES + ["8192 pixels", "8193 pixels"] + [f"n * G mod 4 == {r}" for r in range(4)]


def pixel_count_classes(w, h, n=1):
    out = {f"in-wave count {c} as root" if whole else f"in-wave count {c}, not root" for c, whole in pixel_groups(w, h)}
    if w * h in (GROUP_PX, GROUP_PX + 1):
        out.add(f"{w * h} pixels")
    out.add(f"n * G mod 4 == {n * len(pixel_groups(w, h)) % 4}")
    out |= {c for c in fold_classes(len(pixel_groups(w, h)))}
    return out


# (w, h): widths 1, 2, 3 and 7 put several rows into a block; 8, 16, 24, 128 and 136 end fast blocks on the row end; 5, 9, 11, 43 and 129
# cross one row end per block; the pixel counts leave last blocks of 1..7 pixels; both zero areas
BLOCK_GEOS = [(1, 130), (2, 67), (3, 50), (7, 19), (8, 17), (9, 15), (16, 9), (24, 11), (43, 3), (5, 26), (128, 3), (129, 2), (3, 1), (7, 12), (11, 1), (136, 2),
              (0, 5), (5, 0)]
COUNT_WIDTHS = (5, 7, 9, 11, 13, 16, 33, 128)


def count_geo(c, root):
    """(w, h) whose last wave holds c chunks: the whole image (root) or the second of two groups"""
    w = COUNT_WIDTHS[(c + (0 if root else 3)) % len(COUNT_WIDTHS)]
    lo = (c - 1) * PX_PER_CHUNK + 1 + (0 if root else GROUP_PX)
    return w, -(-lo // w)


COUNT_GEOS = [count_geo(c, root) for root in (True, False) for c in range(1, WAVE + 1)]
EDGE_GEOS = [(128, 64), (64, 128), (8193, 1), (2731, 3)]          # 8192 and 8193 pixels
NG_CASES = [(n, w, h) for w, h in ((9, 15), (129, 129)) for n in (1, 2, 3, 4)]   # one and three groups per image: n * G mod 4 takes every value twice
BIG_GEOS = [(1031, 1018), (1451, 1446)]                            # 129 and 257 groups per image


def uniform_strides(w, h, ch):
    """(row_stride, image_stride): rows padded to an odd stride, an odd gap behind every image (an image without rows still takes one:
    the library wants image_stride >= w * channels whatever h is)"""
    row = w * ch
    rs = row + (1 if row % 2 == 0 else 2)
    return rs, rs * max(h, 1) + 5 + 2 * (w % 2)


def embed_uniform(imgs, lead):
    """images (n, h, w[, ch]) uint8 in one buffer of 0xA5 with uniform_strides and `lead` bytes in front: (buffer, row_stride, image_stride)"""
    n, h, w = imgs.shape[:3]
    ch = 1 if imgs.ndim == 3 else imgs.shape[3]
    rs, st = uniform_strides(w, h, ch)
    buf = np.full(lead + n * st + 8, 0xA5, np.uint8)
    if h and w:
        view = buf[lead:lead + n * st].reshape(n, st)[:, :rs * h].reshape(n, h, rs)
        view[:, :, :w * ch] = imgs.reshape(n, h, w * ch)
    return buf, rs, st


def uniform_images(w, h, ch, n, seed=0):
    return np.random.default_rng([w, h, ch, n, seed]).integers(0, 256, (n, h, w) if ch == 1 else (n, h, w, ch), dtype=np.uint8)


def ragged_image(layout, w, h, seed=0):
    ch, bps, _ = layout_bytes(layout)
    return np.random.default_rng([layout, w, h, seed]).integers(0, 256 ** bps, (h, w) if ch == 1 else (h, w, ch), dtype=np.uint16 if bps == 2 else np.uint8)


def ragged_place(specs, lead=1):
    """(offsets, row strides, end) of images (layout, w, h) in one buffer: u8 rows padded to an odd stride and images wherever the ones in
    front end (every address & 3 comes up), u16 rows padded to a stride = 2 mod 4 and images at even addresses"""
    offs, strides, at = [], [], lead
    for layout, w, h, *_ in specs:
        _, bps, bpp = layout_bytes(layout)
        row = w * bpp
        if bps == 2:
            strides.append(row + (2 if row % 4 == 0 else 4))
            at += at & 1
        else:
            strides.append(row + (1 if row % 2 == 0 else 2))
        offs.append(at)
        at += strides[-1] * h + 3
    return offs, strides, at


def embed_ragged(specs, lead=1):
    """(buffer of 0xA5, views, offsets, strides): image k of ragged_image(*specs[k]) at offsets[k]"""
    offs, strides, end = ragged_place(specs, lead)
    buf = np.full(end + 16, 0xA5, np.uint8)
    views = []
    for (layout, w, h, *rest), o, st in zip(specs, offs, strides):
        ch, bps, _ = layout_bytes(layout)
        v = np.ndarray((h, w, ch), np.uint16 if bps == 2 else np.uint8, buffer=buf, offset=o, strides=(st, ch * bps, bps))
        v[...] = ragged_image(layout, w, h, *rest).reshape(h, w, ch)
        views.append(v[:, :, 0] if ch == 1 else v)
    return buf, views, offs, strides


def ragged_block_specs():
    """every layout at every geometry of BLOCK_GEOS, interleaved"""
    return [(lay, w, h) for w, h in BLOCK_GEOS for lay in LAYOUTS]


def ragged_count_specs():
    """in-wave counts 1..64 as root and not, the layouts taking turns; 8192 and 8193 pixels in every layout"""
    out = [(LAYOUTS[(k + k // 64) % 8],) + geo for k, geo in enumerate(COUNT_GEOS)]
    return out + [(lay, w, h) for w, h in EDGE_GEOS[:3] for lay in LAYOUTS]


# one, two and more than 128 groups as neighbours in the prefix table of groups; the two large images are the fold's 129 and 257
RAGGED_BIG_SPECS = [(3, 9, 15), (17, 1031, 1018), (2, 100, 90), (4, 5, 26), (1, 1451, 1446), (20, 129, 129), (19, 1, 1)]


@functools.lru_cache(maxsize=None)
def uniform_walk_classes(w, h, ch, n, lead):
    rs, st = uniform_strides(w, h, ch)
    out = set()
    for i in range(n):
        out |= pixel_classes(w, h, ch, rs, lead + i * st)
    return out
