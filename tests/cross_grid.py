"""Grids of hashes for the cross-set Hamming sweeps (every pair of TWO sets: hamming_cross_pairs, hamming_variant_cross_pairs, their _dev
forms) and plain numpy references of what such a sweep reports.  The cross sweeps are instantiations of their own with a block prologue
of their own (a rectangle of tile pairs), passes and waves that are skipped when their rows lie past the end of the ROW set, padded rows
that are copies of row 0 of the row set, a launcher that swaps the sides when A has one variant and is the smaller set, and a completion
without the i < j rule and with one low-confidence array per side.  A grid puts near duplicates where that can go wrong instead of leaving
positions to chance.  Seeded, built once per process, read-only, no GPU and no oracle: the references are pinned against the C oracle in
test_cross_grid_cpu.py and the device is compared with them in test_cross_grid_gpu.py.

Geometry (rupphash_amd/csrc/hamming_kernels.hip): a tile is 1024 rows or columns; a row block is 32 rows, the lane that sees pair
(row, col) is (col mod 32, bit 2 of row mod 32); a wave owns 256 rows per pass (fp4 at prefix width above 4: 128, in two passes of 512);
columns are expanded in chunks of 128 or 256; a wave queues at most one entry per lane and chunk and drains at 64 entries, so a drain
meets 64 .. 127 of them.  With one variant per file the larger set becomes the rows; with 8 variants A stays on the rows.

Set A is var_a uint8[n_a, nv, 32] (nv = 1 or 8; variant 0 is the file's own hash), set B is b uint8[n_b, 32]."""
import numpy as np

from sweep_grid import RPH_EDGE_VARIANT_SHIFT, TILE, _flags, flip, lane_of, pack

T = TILE
N_A = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025)
N_B = (1, 33, 129, 257, 1025, 2049)
THR = {"positions": (0, 40, 50, 60, 75, 100), "dense": (0, 4, 40), "sizes": (0, 40, 50, 60, 75, 100)}
THR_SMALL_SIZES = (200, 256)  # sizes grid, n_a and n_b <= 129 only: nearly every pair is an edge
VARIANT_SIMS = (0, 31, 40, 63)

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _freeze(*arrays):
    for x in arrays:
        x.setflags(write=False)
    return arrays


class _Planter:
    """plants pairs (a_i, b_j) at a chosen distance by making one of the two a flip of the other; a hash that a pair has used is never
    written again, so an earlier distance cannot be spoilt by a later pair"""

    def __init__(self, rng, a, b):
        self.rng, self.a, self.b = rng, a, b
        self.used_a, self.used_b = set(), set()

    def b_from_a(self, i, j, d):
        assert j not in self.used_b, ("b", j)
        self.b[j] = flip(self.a[i], d, self.rng)
        self.used_a.add(i)
        self.used_b.add(j)
        return (i, j, d)

    def a_from_b(self, i, j, d):
        assert i not in self.used_a, ("a", i)
        self.a[i] = flip(self.b[j], d, self.rng)
        self.used_a.add(i)
        self.used_b.add(j)
        return (i, j, d)


# ------------------------------------------------------------------ G1: an edge at every position of a 3 x 3 rectangle of tiles
POS_NA, POS_NB = 2 * T + 37, 2 * T + 41
POS_EQUAL = tuple(sorted({0, 31, 32, 1023} | {k for k in range(T) if k % 9 == 4}))  # the (k, k) pairs of block (0, 0)
POS_A_NEAR_MISS = (14, 21, 26)  # rows of a's short tile planted just outside the main threshold (41, 42, 43) ...
POS_B_NEAR_MISS = (15, 22, 27)  # ... and columns of b's short tile (44, 45, 46)
POS_TRIPLES = 230


def block00_partner():
    """the column of b's tile 0 that is a flip of row i of a's tile 0.  With i = 32 q + r the column is 32 ((7 q + r) mod 32) +
    (q + 6 r + 11) mod 32: a bijection (the determinant 41 is odd) under which every row residue meets every column residue, so all 64
    (column mod 32, row half) lanes occur whichever side becomes the rows.  The rows of POS_EQUAL are then made fixed points: the
    pairs (k, k) that the square sweeps' rule `col <= owner` would drop."""
    q, r = np.divmod(np.arange(T), 32)
    p = 32 * ((7 * q + r) % 32) + (q + 6 * r + 11) % 32
    inv = np.empty(T, np.int64)
    inv[p] = np.arange(T)
    for k in POS_EQUAL:
        m, old = inv[k], p[k]
        if m != k:
            p[m], inv[old] = old, m
            p[k] = inv[k] = k
    return p


def positions_triples():
    """(i, v, j, d): variant v in 1 .. 7 of a_i is a flip by d bits of b_j.  Blocks (0,0), (0,2), (2,0), (2,2) and (1,1) in turn; (i, v)
    distinct; d cycles over 0 .. 45"""
    out = []
    for t in range(POS_TRIPLES):
        c, k = t % 5, t // 5
        v = 1 + t % 7
        if c == 0:
            i, j = (379 * k + 5) % T, (131 * k + 7) % T
        elif c == 1:
            i, j = (379 * k + 5 + 512) % T, 2 * T + k % 41
        elif c == 2:
            i, v, j = 2 * T + k % 37, 1 + k // 37, (131 * k + 70) % T
        elif c == 3:
            i, v, j = 2 * T + k % 37, 3 + k // 37, 2 * T + (k + 20) % 41
        else:
            i, j = T + (379 * k + 1) % T, T + (131 * k + 2) % T
        out.append((i, v, j, t % 46))
    return out


def positions():
    """(var_a uint8[POS_NA, 8, 32], b uint8[POS_NB, 32], low_a, low_b, info).  info: 'pairs' the planted (i, j, d) of variant 0,
    'near_miss' those of them at 41 .. 46, 'triples' positions_triples(), 'exceptions' the four planted pairs with a low-confidence
    side as (i, j, d, side)"""
    def make():
        rng = np.random.default_rng(2101)
        a = rng.integers(0, 256, (POS_NA, 32), dtype=np.uint8)
        b = rng.integers(0, 256, (POS_NB, 32), dtype=np.uint8)
        pl = _Planter(rng, a, b)
        pairs, near = [], []
        # (a) block (0, 0): every row and every column, distances cycling over 0 .. 40; row 0 <-> column 0 at distance 0: a[0] == b[0]
        for i, j in enumerate(block00_partner().tolist()):
            pairs.append(pl.b_from_a(i, j, i % 41))
        # (d) copies of hash 0 in every tile of the other side: one equal, one in the last column / row
        pairs += [pl.b_from_a(0, 2 * T, 0), pl.b_from_a(0, POS_NB - 1, 5), pl.b_from_a(0, T + 500, 3)]
        pairs += [pl.a_from_b(2 * T, 0, 0), pl.a_from_b(POS_NA - 1, 0, 7), pl.a_from_b(T + 300, 0, 2)]
        # (b) the short x short corner
        for t in range(1, 13):
            pairs.append(pl.b_from_a(2 * T + t, 2 * T + t, (3 * t + 1) % 41))
        # (c) the rest of a's short tile against b's tiles 0 and 1, the rest of b's short tile against a's tiles 0 and 1
        for t in range(13, 36):
            miss = t in POS_A_NEAR_MISS
            p = pl.a_from_b(2 * T + t, (97 * t + 5) % T + T * (1 - t % 2), 41 + POS_A_NEAR_MISS.index(t) if miss else (7 * t + 2) % 41)
            (near if miss else pairs).append(p)
        for u in range(13, 40):
            miss = u in POS_B_NEAR_MISS
            p = pl.b_from_a((89 * u + 3) % T + T * (1 - u % 2), 2 * T + u, 44 + POS_B_NEAR_MISS.index(u) if miss else (5 * u + 1) % 41)
            (near if miss else pairs).append(p)
        # (b) blocks (0, 1), (1, 0) and (1, 1)
        for t in range(10):
            pairs.append(pl.b_from_a((101 * t + 50) % T, T + 40 + 13 * t, (4 * t + 1) % 41))
            pairs.append(pl.a_from_b(T + 60 + 17 * t, (203 * t + 9) % T, (5 * t + 2) % 41))
        block11 = [pl.b_from_a(T + 400 + 7 * t, T + 420 + 9 * t, t % 41) for t in range(60)]
        pairs += block11
        # (e) variants 1 .. 7
        var = rng.integers(0, 256, (POS_NA, 8, 32), dtype=np.uint8)
        var[:, 0] = a
        triples = positions_triples()
        assert len({(i, v) for i, v, _, _ in triples}) == len(triples)
        for i, v, j, d in triples:
            var[i, v] = flip(b[j], d, rng)
        # (f) low-confidence flags: ~30 % of the files, cleared on every planted one (~15 % remain) ...
        low_a = (rng.random(POS_NA) < 0.30).astype(np.uint8)
        low_b = (rng.random(POS_NB) < 0.30).astype(np.uint8)
        low_a[sorted(pl.used_a | {i for i, _, _, _ in triples})] = 0
        low_b[sorted(pl.used_b | {j for _, _, j, _ in triples})] = 0
        # ... but for an equal pair with a low A side, one with a low B side (both still reported), and two near pairs likewise (dropped)
        exceptions = [block11[0] + ("a",), block11[41] + ("b",), block11[5] + ("a",), block11[46] + ("b",)]
        for i, j, d, side in exceptions:
            assert not any(i == x for x, _, _, _ in triples) and not any(j == y for _, _, y, _ in triples)
            if side == "a":
                low_a[i] = 1
            else:
                low_b[j] = 1
        _freeze(var, b, low_a, low_b)
        return var, b, low_a, low_b, {"pairs": pairs, "near_miss": near, "triples": triples, "exceptions": exceptions}
    return _cached(("positions",), make)


# ------------------------------------------------------------------ G2: families of near duplicates (many candidates per lane, chunk and queue)
DENSE_NA, DENSE_NB = T + 380, T + 360  # a is the larger set: it rides on the rows in either order of the arguments
DENSE_RUNS = ((97, 63, 128), (T + 224, 64, 256), (480, 65, 512))  # (first column, length, tile column it straddles)
QUEUE_WAVE_ROWS = (512, 768)  # the wave whose queue is filled: rows 512 .. 767 of a's tile 0
QUEUE_HUB, QUEUE_LONE_COLUMN = 648, 240
_LANE_TAKEN = {3, 4, 7, 8, 15, 16}  # columns 5 + 32 t that belong to a run or to the queue-fill family


def dense_families():
    """name -> (rows of a, columns of b); every row of a family is a near duplicate of every column of it (distances 0 .. 4).
    'queue2' without its hub row and lone column, which are 21 and 42 bits away from the family hash"""
    fam = {"lane": ([4 + 32 * t + s for t in range(4) for s in range(4)], [5 + 32 * t for t in range(32) if t not in _LANE_TAKEN][:24]),
           "runs": (list(range(221, 291)), [c for start, length, _ in DENSE_RUNS for c in range(start, start + length)]),
           "seam": (list(range(1000, 1048)), list(range(1000, 1048))),
           "tail": ([0] + list(range(DENSE_NA - 40, DENSE_NA)), [0] + list(range(DENSE_NB - 40, DENSE_NB))),
           # two rows of opposite halves near all 32 columns 256 .. 287: 64 (lane, chunk) entries in the chunk that starts at 256
           "queue1": ([520, 525], list(range(256, 288))),
           # another row-block pair of the same wave: row 653 near 31 of the columns 224 .. 255 ...
           "queue2": ([653], [c for c in range(224, 256) if c != QUEUE_LONE_COLUMN])}
    return fam


def prefix_distances(rows, cols):
    """distances over the first 128 bits: what the screen of prefix width 4 sees"""
    return _distance_matrix(np.ascontiguousarray(rows[:, :16]), np.ascontiguousarray(cols[:, :16]))


def dense():
    """(a uint8[DENSE_NA, 32], b uint8[DENSE_NB, 32])"""
    def make():
        rng = np.random.default_rng(2201)
        a = rng.integers(0, 256, (DENSE_NA, 32), dtype=np.uint8)
        b = rng.integers(0, 256, (DENSE_NB, 32), dtype=np.uint8)
        bases = {}
        for name, (rows, cols) in dense_families().items():
            base = bases[name] = rng.integers(0, 256, 32, dtype=np.uint8)
            for m, (side, idx) in enumerate([(a, r) for r in rows] + [(b, c) for c in cols]):
                # every other member differs from the family hash only in the second 128 bits (the first 128 are the prefix the screen
                # looks at): screen and exact completion see different distances.  Member 0 equals the family hash.
                side[idx] = flip(base, (m // 2) % 3, rng, lo=128 if m % 2 else 0)
        # ... and the hub row 648 (other half) near all 32 of them: 21 prefix bits from the family hash, the lone column 240 another 21
        # from the hub.  The hub is within 23 bits of the 31 columns and 21 of the lone one; row 653 (the family hash itself) is 42 from
        # the lone column, in the prefix alone: 32 + 31 = 63 (lane, chunk) entries in the chunk that ends at 256
        bits = rng.choice(128, 42, replace=False)
        for side, idx, mine in ((a, QUEUE_HUB, bits[:21]), (b, QUEUE_LONE_COLUMN, bits)):
            side[idx] = bases["queue2"]
            for k in mine:
                side[idx, k >> 3] ^= np.uint8(1 << (k & 7))
        # no chance candidate in the queue-fill wave: an unrelated row of it that the screen would queue against a column of tile 0 is redrawn
        family_rows = {520, 525, 653, QUEUE_HUB}
        lo, hi = QUEUE_WAVE_ROWS
        while True:
            bad = [lo + r for r in np.nonzero((prefix_distances(a[lo:hi], b[:T]) <= 40).any(1))[0].tolist() if lo + r not in family_rows]
            if not bad:
                break
            a[bad] = rng.integers(0, 256, (len(bad), 32), dtype=np.uint8)
        return _freeze(a, b)
    return _cached(("dense",), make)


def queue_fill(chunk):
    """number of (lane, chunk) queue entries of the queue-fill wave per chunk of `chunk` columns of b's tile 0, at threshold 40 and
    prefix width 4: a lane queues one entry per chunk however many of its pairs pass the screen"""
    a, b = dense()
    lo, hi = QUEUE_WAVE_ROWS
    r, c = np.nonzero(prefix_distances(a[lo:hi], b[:T]) <= 40)
    entries = {(cc // chunk,) + lane_of(lo + rr, cc) for rr, cc in zip(r.tolist(), c.tolist())}
    return [sum(1 for e in entries if e[0] == k) for k in range(T // chunk)]


# ------------------------------------------------------------------ G3: sizes around every pass, wave, block and tile edge
def sizes_pairs(n_a, n_b):
    """(i, j, distance) planted into sizes(n_a, n_b): those of (0, 0), (0, n_b-1), (n_a-1, 0), (n_a-1, n_b-1), (n_a//2, n_b//2) whose
    indices do not repeat an earlier pair"""
    out = []
    for (i, j), d in zip(((0, 0), (0, n_b - 1), (n_a - 1, 0), (n_a - 1, n_b - 1), (n_a // 2, n_b // 2)), (0, 40, 41, 7, 3)):
        if (i, j) not in [(x, y) for x, y, _ in out]:
            out.append((i, j, d))
    return out


def sizes(n_a, n_b):
    """(var_a uint8[n_a, 8, 32], b uint8[n_b, 32]); the one-variant form is var_a[:, :1].  The four corner pairs share files, so their
    distances are fixed together: b[n_b-1] = a[0] ^ S, a[n_a-1] = a[0] ^ S' with |S| = 40, |S'| = 41 and 37 bits in common (7 apart)."""
    def make():
        rng = np.random.default_rng(2301 + 7 * n_a + 100_003 * n_b)
        a = rng.integers(0, 256, (n_a, 32), dtype=np.uint8)
        b = rng.integers(0, 256, (n_b, 32), dtype=np.uint8)
        perm = rng.permutation(256)

        def flipped(h, bits):
            v = h.copy()
            for k in bits:
                v[k >> 3] ^= np.uint8(1 << (k & 7))
            return v

        b[0] = a[0]
        if n_b > 1:
            b[n_b - 1] = flipped(a[0], perm[:40])
        if n_a > 1:
            a[n_a - 1] = flipped(a[0], perm[3:44])
        i, j = n_a // 2, n_b // 2
        if j not in (0, n_b - 1):
            b[j] = flip(a[i], 3, rng)
        elif i not in (0, n_a - 1):
            a[i] = flip(b[j], 3, rng)
        var = rng.integers(0, 256, (n_a, 8, 32), dtype=np.uint8)
        var[:, 0] = a
        var[n_a - 1, 7] = flip(b[n_b - 1], 5, rng)
        return _freeze(var, b)
    return _cached(("sizes", n_a, n_b), make)


# ------------------------------------------------------------------ references
def _distance_matrix(x, y):
    """int16[len(x), len(y)] Hamming distances of two byte matrices, from the bit-matrix product (exact: integers <= 256 in float32)"""
    bx = np.unpackbits(np.ascontiguousarray(x, np.uint8), axis=1).astype(np.float32)
    by = np.unpackbits(np.ascontiguousarray(y, np.uint8), axis=1).astype(np.float32)
    return (bx.sum(1)[:, None] + by.sum(1)[None, :] - 2.0 * (bx @ by.T)).astype(np.int16)


_DIST = {}  # the distance matrices of the last few (var_a, b) asked for: a grid is swept at all its thresholds in a row


def distances(var_a, b):
    """int16[n_a, nv, n_b]: distance(variant v of a_i, b_j)"""
    key = (id(var_a), id(b))
    if key not in _DIST:
        var = np.ascontiguousarray(var_a, np.uint8)
        d = _distance_matrix(var.reshape(-1, 32), np.ascontiguousarray(b, np.uint8).reshape(-1, 32)).reshape(var.shape[0], var.shape[1], -1)
        while len(_DIST) >= 8:
            del _DIST[next(iter(_DIST))]
        _DIST[key] = (var_a, b, d)  # (the arrays are kept with the entry: their ids stay theirs)
    return _DIST[key][2]


def brute(var_a, b, low_a, low_b, thr):
    """int64[m, 4]: the (i, j, v, d) with distance(variant v of a_i, b_j) <= limit, the limit 0 where low_a[i] | low_b[j] and thr otherwise;
    ascending in (i, v, j).  low_a / low_b: uint8 arrays or None"""
    d = distances(var_a, b)
    n_a, _, n_b = d.shape
    la = np.zeros(n_a, np.uint8) if low_a is None else np.asarray(low_a, np.uint8)
    lb = np.zeros(n_b, np.uint8) if low_b is None else np.asarray(low_b, np.uint8)
    limit = np.where((la[:, None] | lb[None, :]) != 0, 0, thr).astype(np.int16)
    i, v, j = np.nonzero(d <= limit[:, None, :])
    return np.stack([i, j, v, d[i, v, j]], axis=1).astype(np.int64).reshape(-1, 4)


def expected(var_a, b, low_a, low_b, thr):
    """sorted keys pack(i, j, d, flags) of what a cross sweep must report: the brute force, the variant in bits 9 .. 11 of the flags and
    the restated probe key of (variant v of a_i, b_j) below it"""
    e = brute(var_a, b, low_a, low_b, thr)
    i, j, v = e[:, 0], e[:, 1], e[:, 2]
    flags = (v << RPH_EDGE_VARIANT_SHIFT) | _flags(np.asarray(var_a)[i, v] ^ np.asarray(b)[j], 16, 16, thr).astype(np.int64)
    return pack(i, j, e[:, 3], flags)


def expected_once(tag, var_a, b, low_a, low_b, thr):
    """expected() of a form of a grid that several tests share, computed once; tag names the form and the flags passed"""
    return _cached(("expected", tag, thr), lambda: expected(var_a, b, low_a, low_b, thr))


# ------------------------------------------------------------------ the forms in which a grid is swept
def _rows(h):
    return _freeze(np.ascontiguousarray(h, np.uint8).reshape(-1, 1, 32).copy())[0]


def positions_forms():
    """name -> (var_a, b, low_a, low_b): 'ab' one variant, a against b (a is the smaller set: swapped), 'ba' one variant, b against a
    (not swapped), 'var' 8 variants of a against b (never swapped)"""
    def make():
        var, b, low_a, low_b, _ = positions()
        a = _freeze(var[:, 0].copy())[0]
        return {"ab": (_rows(a), b, low_a, low_b), "ba": (_rows(b), a, low_b, low_a), "var": (var, b, low_a, low_b)}
    return _cached(("positions", "forms"), make)


def dense_forms():
    def make():
        a, b = dense()
        return {"ab": (_rows(a), b), "ba": (_rows(b), a)}
    return _cached(("dense", "forms"), make)


def sizes_forms(n_a, n_b):
    """'one': the one-variant form (variant 0 alone), 'var': the 8-variant form"""
    def make():
        var, b = sizes(n_a, n_b)
        return {"one": (_rows(var[:, 0]), b), "var": (var, b)}
    return _cached(("sizes", "forms", n_a, n_b), make)
