"""The merge-tree rule (include/rupphash.h, "Merge tree") restated in numpy, and what the merge-tree tests run on
(test_merge_tree_cpu.py needs no GPU and pins the closed forms used at grid size; test_merge_tree_gpu.py runs the kernels).

The model goes by the definition, not by Kruskal: label_s for EVERY s by library_corpus.min_labels over the edges with d <= s, then
level[x] = the first s at which label_s[x] != x and into[x] = that label.  Everything is seeded."""
import ctypes as C
import functools
from collections import namedtuple

import numpy as np

import library_corpus as lc

NEVER = 255
SIMS = (0, 1, 15, 16, 31, 32, 40, 47, 48, 63)  # the cuts compared with rph_group_files_pdq
EDGE = np.dtype([("i", np.uint32), ("j", np.uint32), ("d", np.uint16), ("flags", np.uint16)])

Tree = namedtuple("Tree", "into level edges_at labels")  # labels: (top + 1, n), label_s for every s


def edge_array(ijd):
    """(m, 3) integers -> rph_edge records (flags 0)"""
    ijd = np.asarray(ijd, np.int64).reshape(-1, 3)
    out = np.zeros(len(ijd), EDGE)
    out["i"], out["j"], out["d"] = ijd[:, 0], ijd[:, 1], ijd[:, 2]
    return out


def tree_of(n, ijd, top):
    """the rule over an edge list (i, j, d) in global numbering, d <= top"""
    ijd = np.asarray(ijd, np.int64).reshape(-1, 3)
    assert (ijd[:, 2] <= top).all() and (ijd[:, :2] < max(n, 1)).all()
    labels = np.stack([lc.min_labels(n, ijd[ijd[:, 2] <= s][:, :2]) for s in range(top + 1)]) if n else np.zeros((top + 1, 0), np.uint32)
    ids = np.arange(n, dtype=np.uint32)
    moved = labels != ids[None, :]
    level = np.where(moved.any(axis=0), moved.argmax(axis=0), NEVER).astype(np.uint8)
    into = np.where(level == NEVER, ids, labels[np.minimum(level, top), ids]).astype(np.uint32)
    edges_at = np.bincount(ijd[:, 2], minlength=top + 1).astype(np.uint64)
    return Tree(into, level, edges_at, labels)


def check_consequences(into, level, top):
    """what the header states about every tree: into[x] < x, levels rise strictly along a chain, chains of at most top + 1 links"""
    n = len(into)
    ids = np.arange(n)
    joined = level != NEVER
    assert (into[~joined] == ids[~joined]).all() and (into[joined] < ids[joined]).all() and (level[joined] <= top).all()
    assert (level[into[joined]].astype(int) > level[joined]).all()  # (NEVER is 255: above every level)
    at, links = ids.copy(), 0
    while (level[at] != NEVER).any():
        at = np.where(level[at] != NEVER, into[at], at)
        links += 1
        assert links <= top + 1
    return links


def profile_of(labels):
    """(components with more than one member, files in them) for every s, by counting"""
    groups, files = [], []
    for row in labels:
        count = np.bincount(row, minlength=len(row))
        groups.append(int((count > 1).sum()))
        files.append(int(count[count > 1].sum()))
    return np.array(groups, np.uint64), np.array(files, np.uint64)


# ---------------------------------------------------------------- hand-made edge lists
# name, n, top, edges (m, 3) = (i, j, d) as the call gets them, i_base, j_base
EdgeCase = namedtuple("EdgeCase", "name n top edges i_base j_base")


def _case(name, n, top, edges, i_base=0, j_base=0):
    return EdgeCase(name, n, top, np.asarray(edges, np.int64).reshape(-1, 3), i_base, j_base)


def edge_cases():
    import itertools

    rng = np.random.default_rng(515)
    # into[3] must be 0: the root a CAS hooks 3 under may be hooked itself later in the level
    chain = [(2, 3, 9), (1, 2, 9), (0, 1, 9)]
    for k, order in enumerate(itertools.permutations(chain)):
        yield _case(f"same-level-chain-order-{k}", 4, 20, order)
    yield _case("ladder-0-64", 65, 63, [(k, k + 1, k) for k in range(64)])  # every level non-empty, one edge per bucket
    yield _case("ladder-hub-last", 65, 63, [(63 - k, 64, k) for k in range(64)])  # the absorbing root changes at every level
    tri = [(0, 1, 3), (1, 2, 3)]
    yield _case("cycle-closed-by-equal-edge", 3, 10, tri + [(0, 2, 3)])
    yield _case("cycle-closed-by-heavier-edge", 3, 10, tri + [(0, 2, 7)])
    yield _case("cycle-closed-by-lighter-edge", 3, 10, tri + [(0, 2, 1)])
    some = np.stack([rng.integers(0, 300, 150), rng.integers(0, 300, 150)], axis=1)
    eight = np.repeat(some, 8, axis=0)
    yield _case("every-edge-8-times-differing-d", 300, 63, np.concatenate([eight, rng.integers(0, 64, (len(eight), 1))], axis=1))
    yield _case("self-edges", 50, 12, [(k, k, k % 13) for k in range(50)] + [(3, 9, 4), (9, 9, 0), (9, 30, 4), (30, 3, 2)])
    yield _case("empty-levels", 40, 254, [(0, 1, 7), (2, 3, 7), (1, 3, 100), (5, 4, 101), (4, 0, 200), (10, 11, 253)])  # both ends and the middle empty
    yield _case("largest-top-with-an-edge-at-it", 12, 254, [(0, 1, 254), (1, 2, 0), (5, 4, 254), (4, 2, 253)])  # 255 is NEVER: top stops at 254
    yield _case("top-0", 6, 0, [(0, 1, 0), (4, 3, 0), (3, 1, 0)])
    yield _case("no-edges", 70, 63, [])
    yield _case("n-1", 1, 63, [])
    yield _case("n-1-self-edge", 1, 5, [(0, 0, 5)])
    star = [(0, k, 17) for k in range(1, 600)]
    yield _case("one-bucket-all-edges", 600, 63, star)
    # the first wave of the first block: 64 lanes with 64 levels; the next: 64 lanes with one
    lanes = [(k, 64 + k, k) for k in range(64)] + [(128 + k, 200 + k, 33) for k in range(64)]
    yield _case("wave-64-levels-then-wave-one-level", 300, 63, lanes)
    # as the library's append passes them: cross edges (library, new-local), inner edges (new-local, new-local)
    k, n = 700, 1000
    cross = np.stack([rng.integers(0, k, 200), rng.integers(0, n - k, 200), rng.integers(0, 41, 200)], axis=1)
    inner = np.stack([rng.integers(0, n - k, 120), rng.integers(0, n - k, 120), rng.integers(0, 41, 120)], axis=1)
    yield _case("cross-edges-with-j-base", n, 40, cross, 0, k)
    yield _case("inner-edges-with-both-bases", n, 40, inner, k, k)
    yield _case("random-3000-over-5000", 5000, 63, np.stack([rng.integers(0, 5000, 3000), rng.integers(0, 5000, 3000), rng.integers(0, 64, 3000)], axis=1))


def global_ijd(case):
    return case.edges + np.array([case.i_base, case.j_base, 0], np.int64)[None, :]


# ---------------------------------------------------------------- beyond one grid: closed forms
# G lanes are one pass of the kernels' grid-stride loops (library_corpus.grid_sizes).  test_merge_tree_cpu.py pins these closed forms
# against tree_of at G = 1024.
def blocks_of_four_tree(n):
    """library_corpus.blocks_of_four, the edge (x, y) at level x & 63.  Every pair is listed from both ends, so the smaller level decides."""
    pairs, _ = lc.blocks_of_four(n)
    ijd = np.concatenate([pairs.astype(np.int64), (pairs[:, :1] & 63).astype(np.int64)], axis=1)
    x = np.arange(n, dtype=np.int64)
    b, r = x & ~3, x & 3
    low = b & 63  # (b, b+1) and (b, b+2) at b & 63; b+3 hangs on b+1, at (b+1) & 63 -- one level later, both ends in the component of b by then
    level = np.where(r == 0, NEVER, np.where(r == 3, low + 1, low))
    into = np.where(r == 0, x, b)
    first = n & ~3  # the ragged last block, by the definition
    if first < n:
        tail = ijd[(ijd[:, :2] >= first).all(axis=1)] - np.array([first, first, 0])
        t = tree_of(n - first, tail, 63)
        level[first:] = t.level
        into[first:] = np.where(t.level == NEVER, x[first:], t.into + first)
    return ijd, into.astype(np.uint32), level.astype(np.uint8)


def star_forest_tree(n):
    """library_corpus.star_forest, follower f joins its hub at level f & 63"""
    pairs, hub = lc.star_forest(n)
    f = np.maximum(pairs[:, 0], pairs[:, 1]).astype(np.int64)  # the hub is the smaller end
    ijd = np.concatenate([pairs.astype(np.int64), (f & 63)[:, None]], axis=1)
    x = np.arange(n, dtype=np.int64)
    level = np.where(hub == x, NEVER, x & 63).astype(np.uint8)
    return ijd, hub.astype(np.uint32), level


LARGE_TREE_CASES = [(family, size) for family in ("blocks-of-four", "star-forest", "star-forest-one-level") for size in ("G+77", "2G+1")]


def large_tree_case(G, family, size, seed=77):
    """(n, shuffled (i, j, d), into, level) of one family with more than G files and at least G + 77 or 2 G + 1 EDGES, so that the loops
    over the files and over the edges both come round again.  star-forest-one-level puts every edge at level 17: one bucket, and more than
    G roots hooked in one level."""
    target = lc.grid_sizes(G)[size == "2G+1"]
    n = target if family == "blocks-of-four" else target + target // 999 + 2  # (a hub per 1000 files has no edge of its own)
    ijd, into, level = (blocks_of_four_tree if family == "blocks-of-four" else star_forest_tree)(n)
    if family == "star-forest-one-level":
        ijd[:, 2] = 17
        level = np.where(level == NEVER, NEVER, 17).astype(np.uint8)
    assert n > G and len(ijd) >= target
    return n, ijd[np.random.default_rng(seed).permutation(len(ijd))], into, level


# ---------------------------------------------------------------- files
Files = namedtuple("Files", "hashes coeffs has_features quality family")
TOP = 63


def _flip(h, bits):
    v = h.copy()
    for b in bits:
        v[b // 8] ^= 1 << (b % 8)
    return v


def dihedral_rows(coeffs256):
    """the 8 rows of a file with features, through rph_pdq_dihedral_one"""
    from rupphash_amd import _lib

    c = np.ascontiguousarray(coeffs256, np.float32)
    out = np.zeros((8, 32), np.uint8)
    _lib.load().rph_pdq_dihedral_one(c.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return out


def to_hash(coeffs256):
    from rupphash_amd import _lib

    c = np.ascontiguousarray(coeffs256, np.float32)
    out = np.zeros(32, np.uint8)
    _lib.load().rph_pdq_to_hash(c.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return out


def is_low(quality):
    return (quality >= 0) & (quality < 50)  # is_low_pdq_quality, scanner.rs:1592-1594; < 0 is None


def file_edges(f, top=TOP, n=None):
    """every (i, j, d) the variant sweep at `top` reports among the first n files: one per row of file i (8 with features, else its
    hash) within the pair's limit -- 0 if either file is low-confidence"""
    n = len(f.hashes) if n is None else n
    bits = np.unpackbits(f.hashes[:n], axis=1).astype(np.int16)
    low = is_low(f.quality[:n])
    out = []
    for i in range(n - 1):
        rows = dihedral_rows(f.coeffs[i]) if f.has_features[i] else f.hashes[i:i + 1]
        rb = np.unpackbits(rows, axis=1).astype(np.int16)
        d = np.abs(rb[:, None, :] - bits[None, i + 1:, :]).sum(axis=2)  # (rows, n - i - 1)
        limit = np.where(low[i] | low[i + 1:], 0, top)
        v, j = np.nonzero(d <= limit[None, :])
        out += [(i, i + 1 + int(jj), int(d[vv, jj])) for vv, jj in zip(v, j)]
    return np.array(out, np.int64).reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def files():
    """~300 files.  Featureless files carry constructed hashes: random 256-bit strings with chosen bit flips, so every distance within 63 is
    built on purpose (unrelated random hashes lie about 128 +- 8 apart); files with features carry random coefficients, whose 8 rows are
    as far from everything else.  family[x] names the construction x belongs to (-1: filler); the builder asserts that no pair of
    different families, and no filler, lies within 63."""
    rng = np.random.default_rng(8088)
    hashes, coeffs, hf, quality, family = [], [], [], [], []

    def add(h=None, features=False, q=90, fam=-1):
        c = rng.normal(0, 20, 256).astype(np.float32)
        hashes.append(to_hash(c) if features else h)
        coeffs.append(c), hf.append(int(features)), quality.append(q), family.append(fam)
        return len(hashes) - 1

    def filler(count):
        for _ in range(count):
            add(rng.integers(0, 256, 32, dtype=np.uint8), features=False, q=int(rng.choice([-1, 60, 90])))
            if rng.random() < 0.3:
                add(features=True)

    def star(fam, sizes, q=90):
        """a base and copies with disjoint flip sets of the given sizes: d(base, copy) = size, d(copy a, copy b) = size a + size b"""
        base, perm, at = rng.integers(0, 256, 32, dtype=np.uint8), rng.permutation(256), 0
        add(base, fam=fam, q=q)
        for m in sizes:
            add(_flip(base, perm[at:at + m]), fam=fam, q=q)
            at += m
            filler(2)

    filler(3)
    star(0, [0, 1, 15, 16, 31, 32, 40])          # joins at 0, 1, 15, 16, 31, 32, 40
    star(1, [47, 48, 63])                         # joins at 47, 48, 63
    # a path: each file 20 or 63 bits from the one before, on fresh bits, so far ends only meet through the middle
    base, perm, at = rng.integers(0, 256, 32, dtype=np.uint8), rng.permutation(256), 0
    add(base, fam=2)
    for m in (63, 20, 63, 20):
        base = _flip(base, perm[at:at + m])
        at += m
        add(base, fam=2)
        filler(1)
    # only through variant 5 of the lower-numbered file: j's hash is i's row 5 with 20 bits flipped, and j has no features
    i = add(features=True, fam=3)
    filler(2)
    add(_flip(dihedral_rows(coeffs[i])[5], rng.permutation(256)[:20]), fam=3)
    # the other index order does not match: the featureless file comes first, and its one row is its hash
    later = rng.normal(0, 20, 256).astype(np.float32)
    add(_flip(dihedral_rows(later)[5], rng.permutation(256)[:20]), fam=4)
    filler(2)
    hashes.append(to_hash(later)), coeffs.append(later), hf.append(1), quality.append(90), family.append(4)
    # low-confidence twins: identical ones join at 0, at one bit they never do; a low-confidence copy of a good file joins it at 0 only
    twin = rng.integers(0, 256, 32, dtype=np.uint8)
    add(twin, q=10, fam=5), filler(1), add(twin, q=49, fam=5)
    near = rng.integers(0, 256, 32, dtype=np.uint8)
    add(near, q=10, fam=6), add(_flip(near, [77]), q=10, fam=6)
    good = rng.integers(0, 256, 32, dtype=np.uint8)
    add(good, q=90, fam=7), add(good, q=0, fam=7), add(_flip(good, [5]), q=90, fam=7), add(_flip(good, [5, 6]), q=3, fam=7)
    # a file with features and an exact copy of its hash, a copy at 63, a copy at 64 (out of reach)
    i = add(features=True, fam=8)
    add(hashes[i].copy(), fam=8), add(_flip(hashes[i], rng.permutation(256)[:63]), fam=8)
    add(_flip(hashes[i], rng.permutation(256)[:64]), fam=9)
    filler(270 - len(hashes))
    star(10, [7, 7])  # behind file 257: the prefix of 257 files does not hold it
    f = Files(np.stack(hashes), np.stack(coeffs), np.array(hf, np.uint8), np.array(quality, np.int32), np.array(family))
    # nothing unintended within 63: every pair a sweep at 63 could report lies inside one family, low confidence set aside
    anyq = f._replace(quality=np.full(len(f.hashes), 90, np.int32))
    e = file_edges(anyq)
    assert ((f.family[e[:, 0]] == f.family[e[:, 1]]) & (f.family[e[:, 0]] >= 0)).all(), e[f.family[e[:, 0]] != f.family[e[:, 1]]]
    return f


FILE_SIZES = (1, 2, 257, None)  # prefixes of files(); None: all of them


@functools.lru_cache(maxsize=None)
def file_tree(n=None):
    """(edges (i, j, d), Tree) of the first n files by the definition"""
    f = files()
    n = len(f.hashes) if n is None else n
    e = file_edges(f, TOP, n)
    return e, tree_of(n, e, TOP)


def file_args(n=None):
    f = files()
    n = len(f.hashes) if n is None else n
    return dict(hashes=f.hashes[:n], coeffs=f.coeffs[:n], has_features=f.has_features[:n], quality=f.quality[:n])
