"""Grids of hashes for the square Hamming sweeps (all pairs of ONE set: hamming_all_pairs, hamming_all_pairs64, hamming_variant_pairs)
and plain numpy references of what a sweep reports.  A grid puts near duplicates where the tiled kernels can go wrong -- every row and
every column position of a 1024-file tile, the last 32-row block of a wave, the short last tile, near duplicates of hash 0 in that tile
(rows past the end are loaded as copies of hash 0), families that fill the candidate queue, sizes around every tile / chunk / block
edge -- instead of leaving positions to chance.  Seeded, built once per process, no GPU and no oracle: the references are pinned against
the C oracle in test_sweep_grid_cpu.py and the device is compared with them in test_sweep_grid_gpu.py.

Hashes are uint8[n, 32] (256 bits) or, for the u64 twins (`bits=64`), uint64[n]; a u64 hash is built as its 8 little-endian bytes."""
import numpy as np

# ------------------------------------------------------------------ geometry of the kernels (rupphash_amd/csrc/hamming_kernels.hip)
TILE = 1024            # files per row tile and per column tile
ROW_BLOCK = 32         # rows (and columns) of one MFMA tile; a wave owns 8 (or 4) row blocks per pass
CHUNKS = (128, 256)    # columns expanded into LDS at a time (which of the two depends on format and prefix width)
RPH_EDGE_MIH_R1 = 0x8000
RPH_EDGE_PROBE_MASK = 0x01FF
RPH_EDGE_VARIANT_SHIFT = 9

SIZES = (2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049)
# thresholds the GPU tests run (the CPU tests pin the references at the same ones)
THR = {("positions", 256): (0, 40, 50, 60, 75, 100), ("dense", 256): (0, 4, 40), ("sizes", 256): (0, 40, 50, 60, 75, 100),
       ("positions", 64): (0, 7, 8, 16, 31, 40), ("dense", 64): (0, 4, 16), ("sizes", 64): (0, 8, 20, 40)}
THR_SMALL_SIZES = (200, 256)  # 256-bit sizes grid, n <= 129 only: nearly every pair is an edge
VARIANT_SIMS = (0, 31, 40, 63)

_CACHE = {}


def lane_of(row, col):
    """the MFMA kernel's lane that sees pair (row, col) of a tile: (column mod 32, bit 2 of row mod 32)"""
    return col % 32, (row % 32 >> 2) & 1


def _cycle(bits):
    """planted distances cycle over 0 .. 40 (u64: 0 .. 16): all within the main threshold, 40 (u64: 16)"""
    return 41 if bits == 256 else 17


def _near_miss(bits, t):
    """distances just above the main threshold: 41 .. 46 (u64: 17 .. 20; its flips stay within 0 .. 20 bits)"""
    return 41 + t % 6 if bits == 256 else 17 + t % 4


def flip(h, d, rng, lo=0):
    """a copy of hash h (uint8[bits / 8]) with d distinct bits flipped, taken from bit lo upwards"""
    v = np.array(h, np.uint8, copy=True)
    for b in rng.choice(np.arange(lo, 8 * len(v)), int(d), replace=False):
        v[b >> 3] ^= np.uint8(1 << (b & 7))
    return v


def _finish(h, bits):
    h = np.ascontiguousarray(h)
    if bits == 64:
        h = h.view("<u8").reshape(-1).astype(np.uint64)
    h.setflags(write=False)
    return h


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ------------------------------------------------------------------ G1: an edge at every tile position
POSITIONS_N = 3 * TILE + 37
POSITIONS_EXPLICIT = ((2 * TILE + 1022, 2 * TILE + 1023), (2 * TILE, 2 * TILE + 1023))
POSITIONS_NEAR_MISS = (3, 9, 15, 21, 27, 33)  # tail entries planted just outside the main threshold


def tile1_partner(i):
    """the column of tile 1 that is a flip of row i of tile 0: a bijection that mixes (column mod 32, row) combinations"""
    return TILE + (37 * i + 11) % TILE


def tile2_matching(seed=1102):
    """perfect matching of tile 2's positions 2 .. 1021 (0, 1, 1022, 1023 form the explicit family): one pair inside every 32-row block
    first, so that every block owns an edge, the rest at random.  Returns (smaller, larger) position pairs."""
    rng = np.random.default_rng(seed)
    free = np.ones(TILE, bool)
    free[[0, 1, 1022, 1023]] = False
    pairs = []
    for b in range(TILE // ROW_BLOCK):
        cand = np.arange(b * ROW_BLOCK, (b + 1) * ROW_BLOCK)
        a, c = rng.choice(cand[free[cand]], 2, replace=False)
        free[[a, c]] = False
        pairs.append((min(a, c), max(a, c)))
    rest = rng.permutation(np.nonzero(free)[0])
    pairs += [(min(a, c), max(a, c)) for a, c in zip(rest[0::2], rest[1::2])]
    return [(int(a), int(c)) for a, c in pairs]


def tail_source(t):
    """the file that tail hash t (index 3 * TILE + t) is a flip of: hash 0 for the first and the last, spread over tiles 0 .. 2 between"""
    return 0 if t in (0, 36) else (997 * t + 13) % (3 * TILE)


def tail_distance(bits, t):
    if t in POSITIONS_NEAR_MISS:
        return _near_miss(bits, POSITIONS_NEAR_MISS.index(t))
    return 0 if t == 0 else (7 * t + 2) % _cycle(bits)  # the first tail hash EQUALS hash 0


def positions(bits=256):
    def make():
        rng = np.random.default_rng(1101 + bits)
        nb, cyc = bits // 8, _cycle(bits)
        h = rng.integers(0, 256, (POSITIONS_N, nb), dtype=np.uint8)
        for i in range(TILE):
            h[tile1_partner(i)] = flip(h[i], i % cyc, rng)
        t2 = 2 * TILE
        for t, (a, c) in enumerate(tile2_matching()):
            h[t2 + c] = flip(h[t2 + a], t % cyc, rng)
        h[t2 + 1] = flip(h[t2], 3, rng)
        h[t2 + 1023] = flip(h[t2], 5, rng)
        h[t2 + 1022] = flip(h[t2 + 1023], 7, rng)
        for t in range(37):
            h[3 * TILE + t] = flip(h[tail_source(t)], tail_distance(bits, t), rng)
        return _finish(h, bits)
    return _cached(("positions", bits), make)


# ------------------------------------------------------------------ G2: families of near duplicates (many candidates per lane, chunk and queue)
DENSE_N = 2 * TILE + 300
DENSE_RUNS = ((TILE + 97, 63, 128), (TILE + 224, 64, 256), (TILE + 500, 65, 512))  # (first index, length, tile column it straddles)


def dense_families():
    fam = {"lane": [5 + 32 * t for t in range(24)], "rows64": [7 + 64 * t for t in range(16)]}
    for start, length, _ in DENSE_RUNS:
        fam[f"run{length}"] = list(range(start, start + length))
    fam["seam"] = list(range(1000, 1048)) + list(range(2040, 2061))
    fam["tail"] = [0] + list(range(DENSE_N - 40, DENSE_N))
    return fam


def dense(bits=256):
    def make():
        rng = np.random.default_rng(1201 + bits)
        nb = bits // 8
        h = rng.integers(0, 256, (DENSE_N, nb), dtype=np.uint8)
        for members in dense_families().values():
            base = rng.integers(0, 256, nb, dtype=np.uint8)
            for m, idx in enumerate(members):
                # every other member differs from the family hash only OUTSIDE the first half of the bits (the first 128 of a 256-bit
                # hash are the prefix the screen looks at): screen and exact completion see different distances
                h[idx] = flip(base, (m // 2) % 3, rng, lo=bits // 2 if m % 2 else 0)
        return _finish(h, bits)
    return _cached(("dense", bits), make)


# ------------------------------------------------------------------ G3: sizes around every tile, chunk and block edge
def sizes_pairs(n, bits=256):
    """(i, j, distance) planted into sizes(n): those of (0, 1), (0, n-1), (n-2, n-1), (n//2, n-1) that exist and do not contradict an
    earlier one (n < 4)"""
    dist = (0, 40, 41, 7) if bits == 256 else (0, 16, 17, 7)
    out, fixed = [], {0}
    for (a, b), d in zip(((0, 1), (0, n - 1), (n - 2, n - 1), (n // 2, n - 1)), dist):
        if a == b or (a in fixed and b in fixed):
            continue
        out.append((a, b, d))
        fixed |= {a, b}
    return out


def sizes(n, bits=256):
    def make():
        rng = np.random.default_rng(1301 + bits + 7 * n)
        h = rng.integers(0, 256, (n, bits // 8), dtype=np.uint8)
        fixed = {0}
        for a, b, d in sizes_pairs(n, bits):
            src, dst = (a, b) if b not in fixed else (b, a)
            h[dst] = flip(h[src], d, rng)
            fixed |= {a, b}
        return _finish(h, bits)
    return _cached(("sizes", bits, n), make)


# ------------------------------------------------------------------ G4: 8 variants per file
VARIANTS_N = TILE + 129
VARIANTS_PLANTED = 230


def variants_planted():
    """(i, v, j, d): variant v of file i is a flip by d bits of hash j > i; i distinct, (0, ., n - 1) first"""
    n, out = VARIANTS_N, []
    for t in range(VARIANTS_PLANTED):
        i = 0 if t == 0 else (379 * t) % 1100
        j = n - 1 if t == 0 else i + 1 + (131 * t) % (n - 1 - i)
        out.append((i, 1 + t % 7, j, t % 46))
    return out


def variants():
    """(variants uint8[n, 8, 32], hashes uint8[n, 32], low uint8[n])"""
    def make():
        rng = np.random.default_rng(1401)
        n = VARIANTS_N
        h = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        var = rng.integers(0, 256, (n, 8, 32), dtype=np.uint8)
        var[:, 0] = h
        planted = variants_planted()
        for i, v, j, d in planted:
            var[i, v] = flip(h[j], d, rng)
        low = (rng.random(n) < 0.25).astype(np.uint8)  # (~15 % once the planted files are cleared)
        for i, v, j, d in planted:  # planted pairs stay ordinary ones ...
            low[i] = low[j] = 0
        # ... but for: equal pairs with a low-confidence side (still reported), near pairs with one (suppressed)
        low[planted[46][0]] = low[planted[92][2]] = 1
        low[planted[47][0]] = low[planted[93][2]] = 1
        for a in (var, h, low):
            a.setflags(write=False)
        return var, h, low
    return _cached(("variants",), make)


# ------------------------------------------------------------------ references
def _distances256(h):
    b = np.unpackbits(np.ascontiguousarray(h, np.uint8).reshape(-1, 32), axis=1).astype(np.float32)
    pc = b.sum(1)
    return (pc[:, None] + pc[None, :] - 2.0 * (b @ b.T)).astype(np.int16)  # exact: integers <= 256 in float32


def _distances64(h):
    h = np.ascontiguousarray(h, np.uint64)
    n = len(h)
    d = np.zeros((n, n), np.uint8)
    for s in range(0, n, 256):  # strips of rows against the columns from the strip on: the upper triangle is all that is read
        x = h[s:s + 256, None] ^ h[None, s:]
        pc = np.zeros(x.shape, np.uint8)
        for k in range(64):
            pc += ((x >> np.uint64(k)) & np.uint64(1)).astype(np.uint8)
        d[s:s + 256, s:] = pc
    return d


def _edges_of(d, thr):
    i, j = np.nonzero(np.triu(d <= thr, k=1))
    return np.stack([i, j, d[i, j].astype(np.int64)], axis=1).astype(np.int64).reshape(-1, 3)


def brute256(h, thr):
    """int64[m, 3]: the (i, j, d) with i < j and d <= thr, ascending in (i, j)"""
    return _edges_of(_distances256(h), thr)


def brute64(h, thr):
    return _edges_of(_distances64(h), thr)


def _flags(x, width, nchunks, thr):
    """x: uint8[m, nbytes] XOR of the two hashes -> uint16 flags[m].  The probe key of find_groups (hamminghash.rs:206-238): chunk k is
    bytes 2k, 2k+1 little endian (u64: byte k); the first chunk (ascending) whose difference has at most `tol` bits set; slot 0 = the
    exact bucket, 1 + b = the bucket with bit b flipped."""
    tol = 1 if thr // nchunks >= 1 else 0
    m = len(x)
    bitsle = np.unpackbits(x, axis=1, bitorder="little").reshape(m, nchunks, width)  # bit b of chunk k
    pc = bitsle.sum(2)
    ok = pc <= tol
    k = ok.argmax(1)
    row = np.arange(m)
    slot = np.where(pc[row, k] == 0, 0, 1 + bitsle[row, k].argmax(1))
    return np.where(ok.any(1), RPH_EDGE_MIH_R1 | (k << 5) | slot, 0).astype(np.uint16)


def flags256(h, i, j, thr):
    h = np.ascontiguousarray(h, np.uint8).reshape(-1, 32)
    return _flags(h[np.asarray(i, np.int64)] ^ h[np.asarray(j, np.int64)], 16, 16, thr)


def flags64(h, i, j, thr):
    b = np.ascontiguousarray(h, "<u8").view(np.uint8).reshape(-1, 8)
    return _flags(b[np.asarray(i, np.int64)] ^ b[np.asarray(j, np.int64)], 8, 8, thr)


def variant_brute(var, hashes, low, thr):
    """int64[m, 4]: the (i, j, v, d) with j > i and distance(variant v of i, hash j) <= limit, the limit 0 where low[i] | low[j]"""
    n = len(hashes)
    bv = np.unpackbits(np.ascontiguousarray(var, np.uint8).reshape(-1, 32), axis=1).astype(np.float32)
    bh = np.unpackbits(np.ascontiguousarray(hashes, np.uint8), axis=1).astype(np.float32)
    dist = (bv.sum(1)[:, None] + bh.sum(1)[None, :] - 2.0 * (bv @ bh.T)).astype(np.int64).reshape(n, -1, n)
    low = np.asarray(low, np.uint8)
    limit = np.where((low[:, None] | low[None, :]) != 0, 0, thr)
    later = np.arange(n)[None, :] > np.arange(n)[:, None]
    i, v, j = np.nonzero((dist <= limit[:, None, :]) & later[:, None, :])
    return np.stack([i, j, v, dist[i, v, j]], axis=1).astype(np.int64).reshape(-1, 4)


# ------------------------------------------------------------------ comparing edge lists
def pack(i, j, d, flags):
    """sorted uint64 keys, one per (i, j, d, flags): two edge lists are the same multiset of tuples iff their keys are equal"""
    i, j, d, flags = (np.asarray(a).astype(np.uint64) for a in (i, j, d, flags))
    assert (i < 1 << 16).all() and (j < 1 << 16).all() and (d < 1 << 9).all() and (flags < 1 << 16).all()
    return np.sort((i << np.uint64(41)) | (j << np.uint64(25)) | (d << np.uint64(16)) | flags)


def unpack(keys):
    keys = np.asarray(keys, np.uint64)
    return [(int(k >> 41), int((k >> 25) & 0xFFFF), int((k >> 16) & 0x1FF), int(k & 0xFFFF)) for k in keys.tolist()]


def edge_keys(edges):
    """keys of a device edge list (EDGE_DTYPE records)"""
    return pack(edges["i"], edges["j"], edges["d"], edges["flags"])


def difference(got, want, limit=8):
    """'' when the two key arrays are equal, otherwise the first (i, j, d, flags) that are missing and that are extra (or double)"""
    if len(got) == len(want) and np.array_equal(got, want):
        return ""
    gu, gc = np.unique(got, return_counts=True)
    wu, wc = np.unique(want, return_counts=True)
    missing = np.setdiff1d(wu, gu)
    extra = np.concatenate([np.setdiff1d(gu, wu), gu[gc > 1]])
    return f"{len(got)} edges, {len(want)} expected; missing {unpack(missing[:limit])}; extra or reported twice {unpack(extra[:limit])}"


GRIDS = {"positions": positions, "dense": dense}


def grid(name, bits=256, n=None):
    return sizes(n, bits) if name == "sizes" else GRIDS[name](bits)


def distances(name, bits=256, n=None):
    """the full distance matrix of a grid, computed once"""
    return _cached(("dist", name, bits, n), lambda: (_distances256 if bits == 256 else _distances64)(grid(name, bits, n)))


def edges(name, thr, bits=256, n=None):
    """brute-force (i, j, d) of a grid at a threshold, from the cached distance matrix"""
    return _edges_of(distances(name, bits, n), thr)


def expected(name, thr, bits=256, n=None):
    """sorted keys of what a square sweep of the grid must report at `thr`: brute force plus the restated probe key"""
    def make():
        e = edges(name, thr, bits, n)
        f = (flags256 if bits == 256 else flags64)(grid(name, bits, n), e[:, 0], e[:, 1], thr)
        return pack(e[:, 0], e[:, 1], e[:, 2], f)
    return _cached(("expected", name, bits, n, thr), make)
