"""What the device union-find, the component export and the resident library are tested on (test_library_cpu.py pins the expectations
without a GPU; test_components_gpu.py and test_library_gpu.py run them).  Everything is seeded and needs numpy and the CPU oracle only."""
import functools
from collections import namedtuple

import numpy as np

# n files; labels: the forest on entry (None = identity); calls: [(edges (m, 2) uint32, i_base, j_base)], one rph_union_find_labels_dev each
UnionCase = namedtuple("UnionCase", "name n labels calls")


def _e(pairs):
    return np.array(list(pairs), np.uint32).reshape(-1, 2)


def _path(n):
    return _e((k, k + 1) for k in range(n - 1))


def edge_lists():
    rng = np.random.default_rng(2024)
    one = lambda name, n, edges, labels=None: UnionCase(name, n, labels, [(edges, 0, 0)])  # noqa: E731
    p65 = _path(65)
    yield one("path-65-ascending", 65, p65)  # one wave's lanes all hook neighbours
    yield one("path-65-descending", 65, p65[::-1].copy())
    yield one("path-65-shuffled", 65, p65[rng.permutation(len(p65))])
    p4097 = _path(4097)
    yield one("path-4097-shuffled", 4097, p4097[rng.permutation(len(p4097))])  # many blocks
    yield one("star-hub-first", 2000, _e((0, k) for k in range(1, 2000)))
    yield one("star-hub-last", 2000, _e((k, 1999) for k in range(1999)))  # the hub's root changes under every CAS
    cliques = [(a, b) for base in (0, 40) for a in range(base, base + 40) for b in range(a + 1, base + 40)] + [(17, 63)]
    yield one("two-cliques-one-bridge", 90, _e(cliques))
    some = _e(zip(rng.integers(0, 300, 150), rng.integers(0, 300, 150)))
    yield one("every-edge-8-times", 300, np.repeat(some, 8, axis=0))  # as the variant sweeps report them
    yield one("self-edges", 50, _e([(k, k) for k in range(50)] + [(3, 9), (9, 9), (9, 30)]))
    yield one("no-edges", 70, _e([]))
    yield one("n-1", 1, _e([]))
    yield one("n-1-self-edge", 1, _e([(0, 0)]))
    yield one("random-3000-over-5000", 5000, _e(zip(rng.integers(0, 5000, 3000), rng.integers(0, 5000, 3000))))
    # three old groups kept as labels, one new file with an edge into each
    labels = np.arange(41, dtype=np.uint32)
    labels[[5, 6, 7]] = 4
    labels[[21, 30]] = 20
    labels[39] = 11
    yield UnionCase("forest-plus-one-node", 41, labels, [(_e([(6, 40), (30, 40), (39, 40)]), 0, 0)])
    # a library of k files and n - k new ones: cross edges (library, new-local) then inner edges (new-local, new-local)
    k, n = 700, 1000
    cross = _e(zip(rng.integers(0, k, 200), rng.integers(0, n - k, 200)))
    inner = _e(zip(rng.integers(0, n - k, 120), rng.integers(0, n - k, 120)))
    yield UnionCase("two-calls-with-bases", n, None, [(cross, 0, k), (inner, k, k)])


def global_edges(case):
    """the case's edges in the numbering of the whole set, the entry forest's pointers included"""
    parts = [np.stack([e[:, 0] + ib, e[:, 1] + jb], axis=1) for e, ib, jb in case.calls]
    if case.labels is not None:
        parts.append(np.stack([np.arange(case.n, dtype=np.uint32), case.labels], axis=1))
    return np.concatenate(parts).astype(np.uint32)


def min_labels(n, edges):
    """union-find that hooks the larger root under the smaller: label[x] = smallest index of x's component"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in edges.tolist():
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([find(x) for x in range(n)], np.uint32)


def groups_of(labels):
    """components with more than one member, members ascending, groups by first member"""
    by = {}
    for x, l in enumerate(np.asarray(labels).tolist()):
        by.setdefault(l, []).append(x)
    return [m for _, m in sorted(by.items()) if len(m) > 1]


def label_families(n):
    ids = np.arange(n, dtype=np.uint32)
    yield f"singletons-{n}", ids.copy()
    yield f"one-component-{n}", np.zeros(n, np.uint32)
    pairs = ids & ~np.uint32(1)
    yield f"pairs-{n}", pairs
    half = ids.copy()
    half[n // 2: 2 * (n // 2)] = ids[: n // 2]  # (k, k + n / 2): members interleave in index order
    yield f"interleaved-{n}", half


def label_cases():
    for n in (1, 2, 255, 256, 257, 4099):
        yield from label_families(n)


# ---------------------------------------------------------------- beyond one grid
# A union-find or export launch has at most 8 * compute_units blocks of 256 lanes: G = 8 * cus * 256 items are one pass of the grid-stride
# loops.  These cases are there for the second pass and the 64-bit indexing, not for depth: shallow components whose labels have a closed
# form (`want`), edges shuffled.  test_library_cpu.py pins want == min_labels at G = 1024.
LargeCase = namedtuple("LargeCase", "name n labels calls want")


def grid_sizes(G):
    return (G + 77, 2 * G + 1)  # one full pass and a ragged second; two full passes and one item


def blocks_of_four(n):
    """(x, x ^ 1) and (x, x ^ 2) for every x whose partner is inside n: label x & ~3, also in a ragged last block (its first member has an
    edge to each of the others that exist)"""
    x = np.arange(n, dtype=np.uint32)
    edges = np.concatenate([np.stack([x, x ^ k], axis=1)[(x ^ k) < n] for k in (1, 2)])
    want = x & ~np.uint32(3)
    first = n & ~3
    want[first:] = first + min_labels(n - first, edges[(edges >= first).all(axis=1)] - first)  # the ragged block, derived the same way
    return edges, want


def star_forest(n):
    """hub 1000 k to each of its followers, the hub as j in half of the edges: hub contention in every block at once"""
    x = np.arange(n, dtype=np.uint32)
    hub = x - x % 1000
    f = x[x != hub]
    edges = np.where((f % 2 == 1)[:, None], np.stack([hub[f], f], axis=1), np.stack([f, hub[f]], axis=1)).astype(np.uint32)
    return edges, hub


def split_with_bases(edges, n):
    """two calls: the edges inside the upper half local to it, with i_base = j_base = n / 2; the rest as they are"""
    h = n // 2
    upper = (edges >= h).all(axis=1)
    return [(edges[~upper], 0, 0), (edges[upper] - np.uint32(h), h, h)]


LARGE_CASES = [f"{family}-{size}{calls}" for family in ("blocks-of-four", "star-forest") for size in ("G+77", "2G+1") for calls in ("", "-two-calls")] + [
    "star-forest-G+77-every-edge-8-times", "clique-1500-in-2000", "chain-4097-as-entry-forest"]


def large_case(G, name):
    """one of LARGE_CASES at a grid of G lanes (built on request: the large ones hold millions of edges)"""
    rng = np.random.default_rng([4242, LARGE_CASES.index(name)])
    if name == "clique-1500-in-2000":  # 1 124 250 edges, all aimed at one root
        a, b = np.triu_indices(1500, 1)
        edges = (np.stack([a, b], axis=1) + 250).astype(np.uint32)
        want = np.arange(2000, dtype=np.uint32)
        want[250:1750] = 250
        return LargeCase(name, 2000, None, [(edges[rng.permutation(len(edges))], 0, 0)], want)
    if name == "chain-4097-as-entry-forest":  # legal (labels[x] <= x) but not flattened: one chain, no edges
        chain = np.maximum(np.arange(4097, dtype=np.int64) - 1, 0).astype(np.uint32)
        return LargeCase(name, 4097, chain, [(_e([]), 0, 0)], np.zeros(4097, np.uint32))
    n = grid_sizes(G)["2G+1" in name]
    edges, want = (blocks_of_four if name.startswith("blocks") else star_forest)(n)
    edges = edges[rng.permutation(len(edges))]
    if name.endswith("two-calls"):
        return LargeCase(name, n, None, split_with_bases(edges, n), want)
    if name.endswith("8-times"):
        edges = np.repeat(edges, 8, axis=0)  # as the variant sweeps report them
    return LargeCase(name, n, None, [(edges, 0, 0)], want)


def large_edge_lists(G):
    for name in LARGE_CASES:
        yield large_case(G, name)


# ---------------------------------------------------------------- dense sets
def library_first_cap(n_new):
    """the edge capacity rph_library_append starts its retry loop with, read from library.cpp (the dense cases assert that they overflow
    THIS number: when it changes they fail their premise, not their purpose)"""
    import os
    import re

    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rupphash_amd", "csrc", "library.cpp")).read()
    found = re.findall(r"uint64_t cap = std::max<uint64_t>\((\d+)u << (\d+), (\d+) \* n_new\);", src)
    assert len(found) == 1, "the initial capacity of append() is no longer written as max(a << b, c * n_new)"
    a, b, c = map(int, found[0])
    return max(a << b, c * n_new)


def dense_hashes(m, seed=99, common=None):
    """m files that share one hash, and one unrelated random hash behind every 40 of them (so that labels are not all zero):
    (hashes, is_common)"""
    rng = np.random.default_rng(seed)
    common = rng.integers(0, 256, 32, dtype=np.uint8) if common is None else common
    rows, flag = [], []
    for k in range(m):
        rows.append(common)
        flag.append(True)
        if k % 40 == 39:
            rows.append(rng.integers(0, 256, 32, dtype=np.uint8))
            flag.append(False)
    return np.stack(rows), np.array(flag)


def dense_expectation(is_common, rows_per_file=1):
    """closed form of a dense set at a similarity under the unrelated hashes' distances: (labels, groups, comparisons)"""
    ids = np.nonzero(is_common)[0]
    labels = np.arange(len(is_common), dtype=np.uint32)
    labels[ids] = ids[0] if len(ids) else 0
    m = len(ids)
    return labels, ([ids.tolist()] if m > 1 else []), rows_per_file * m * (m - 1) // 2


# ---------------------------------------------------------------- files
N_FILES = 1901
BRIDGE = dict(a=200, a2=201, b=300, b2=301, c=1900)  # C is the last file: its append merges the groups of A and of B
SPLITS = [[1901], [1, 1900], [1500, 1, 400], [0, 900, 0, 1001], [1023, 1, 1, 876], [100] * 19 + [1]]

Files = namedtuple("Files", "coeffs hashes dih quality has_features")


def _flip(rng, h, bits):
    v = h.copy()
    for b in bits:
        v[b // 8] ^= 1 << (b % 8)
    return v


def mirror(c):
    m = c.reshape(16, 16).copy()
    m[:, 0::2] *= -1
    return m.ravel()


def files(rng, oracle):
    """Near-duplicate coefficient families (small perturbations), mirrored copies, qualities with None (-1) and low values, 10 %
    featureless files; hashes and the 8 dihedral variants by the CPU oracle.  Plus five featureless files that only have hashes:
    A, A' (5 bits from A), B, B' and C with d(A, C) = d(B, C) = 30 on disjoint bits, so d(A, B) = 60."""
    n = N_FILES
    coeffs = rng.normal(0, 20, (n, 256)).astype(np.float32)
    for _ in range(60):
        src = rng.integers(0, n)
        for j in rng.choice(n, 3, replace=False):
            coeffs[j] = coeffs[src] + rng.normal(0, 0.8, 256).astype(np.float32)
    coeffs[1500] = coeffs[3] + rng.normal(0, 0.8, 256).astype(np.float32)
    coeffs[1] = coeffs[0] + rng.normal(0, 0.8, 256).astype(np.float32)
    coeffs[1400] = mirror(coeffs[10])
    coeffs[1700] = mirror(coeffs[20])
    hashes = np.stack([oracle.to_hash(c) for c in coeffs])
    dih = np.stack([oracle.dihedral_hashes(c) for c in coeffs])
    quality = rng.integers(30, 101, n).astype(np.int32)
    quality[::7] = -1
    has_features = (rng.random(n) > 0.1).astype(np.uint8)
    has_features[[0, 1, 3, 10, 20, 1500]] = 1
    quality[[0, 1, 3, 1500]] = 90
    bits = rng.permutation(256)
    c = rng.integers(0, 256, 32, dtype=np.uint8)
    a, b = _flip(rng, c, bits[:30]), _flip(rng, c, bits[30:60])
    for key, h in (("a", a), ("a2", _flip(rng, a, bits[60:65])), ("b", b), ("b2", _flip(rng, b, bits[65:70])), ("c", c)):
        i = BRIDGE[key]
        hashes[i], has_features[i], quality[i] = h, 0, 90
        dih[i] = h  # what a featureless file's rows are
    return Files(coeffs, hashes, dih, quality, has_features)


@functools.lru_cache(maxsize=None)
def corpus():
    import oracle

    oracle.lib()
    return files(np.random.default_rng(6061), oracle)


def batches(split):
    """(first, last) of every batch of a split"""
    out, at = [], 0
    for m in split:
        out.append((at, at + m))
        at += m
    assert at == N_FILES
    return out
