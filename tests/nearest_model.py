"""The rule of rph_hamming_nearest (include/rupphash.h) in numpy, and builders of libraries whose answers are known in closed form.
Shared by test_nearest_cpu.py and test_nearest_gpu.py; nothing here touches the library under test."""
import numpy as np

from rupphash_amd import EDGE_DTYPE

NO_FILE = 0xFFFFFFFF
MAX_K = 64
VARIANT_SHIFT = 9
EMPTY_D = 0xFFFF


def as_rows(rows):
    rows = np.ascontiguousarray(rows, np.uint8)
    return rows.reshape(len(rows), 1, 32) if rows.ndim == 2 else rows


def distances(rows, hashes_q):
    """d[i, v, q] = hamming256(rows[i, v], hashes_q[q]) by unpackbits"""
    r = np.unpackbits(as_rows(rows), axis=2).astype(np.float32)          # [n, nv, 256] of 0 / 1
    q = np.unpackbits(np.ascontiguousarray(hashes_q, np.uint8).reshape(-1, 32), axis=1).astype(np.float32)  # [nq, 256]
    n, nv, _ = r.shape
    # differing bits = ones(a) + ones(b) - 2 common ones; every term is an integer <= 256, exact in float32
    common = r.reshape(n * nv, 256) @ q.T
    d = r.sum(axis=2).reshape(n * nv, 1) + q.sum(axis=1)[None, :] - 2 * common
    return d.astype(np.int32).reshape(n, nv, len(q))


def file_distances(rows, hashes_q, has_features=None):
    """(dist[i, q], variant[i, q]): minimum over the rows a file owns and the smallest row attaining it"""
    d = distances(rows, hashes_q)
    if has_features is not None and d.shape[1] > 1:
        plain = np.asarray(has_features, np.uint8) == 0
        d[plain, 1:, :] = 1 << 20  # rows 1.. of a file without features are not its own
    return d.min(axis=1), d.argmin(axis=1)  # argmin: the first (smallest) index of the minimum


def nearest(rows, hashes_q, k, max_dist=256, has_features=None, skip=None):
    """(edges[n_q, k], counts[n_q]) as every form of the call must return them"""
    rows = as_rows(rows)
    hq = np.ascontiguousarray(hashes_q, np.uint8).reshape(-1, 32)
    n, nq = len(rows), len(hq)
    edges = np.zeros((nq, k), EDGE_DTYPE)
    edges["i"], edges["d"] = NO_FILE, EMPTY_D
    edges["j"] = np.arange(nq, dtype=np.uint32)[:, None]
    counts = np.zeros(nq, np.uint32)
    if n == 0 or nq == 0:
        return edges, counts
    dist, variant = file_distances(rows, hq, has_features)
    files = np.arange(n)
    for q in range(nq):
        ok = dist[:, q] <= max_dist
        if skip is not None and skip[q] is not None and int(skip[q]) != NO_FILE:
            ok &= files != int(skip[q])
        cand = files[ok]
        order = np.lexsort((cand, dist[cand, q]))[:k]  # by (d, i)
        got = cand[order]
        counts[q] = len(got)
        edges["i"][q, :len(got)] = got
        edges["d"][q, :len(got)] = dist[got, q]
        edges["flags"][q, :len(got)] = variant[got, q] << VARIANT_SHIFT
    return edges, counts


def same(got, want):
    """exact equality of all slots and counts, with the first difference in the message"""
    (ge, gc), (we, wc) = got, want
    assert ge.shape == we.shape and gc.shape == wc.shape, (ge.shape, we.shape)
    if not np.array_equal(gc, wc):
        q = int(np.flatnonzero(gc != wc)[0])
        raise AssertionError(f"counts differ at query {q}: {gc[q]} != {wc[q]}")
    if ge.tobytes() != we.tobytes():
        q, r = (int(x[0]) for x in np.nonzero(ge != we))
        raise AssertionError(f"slot ({q}, {r}): {ge[q, r]} != {we[q, r]}\n got {ge[q]}\nwant {we[q]}")


# ---- builders ----
def flip(h, bits):
    out = np.array(h, np.uint8, copy=True)
    for b in bits:
        out[int(b) // 8] ^= np.uint8(1 << (int(b) % 8))
    return out


def base_hash(seed=7):
    return np.random.default_rng(seed).integers(0, 256, 32, dtype=np.uint8)


def ladder(n, base=None):
    """file i = base with its first i mod 257 bits flipped: dist(file i, base) = i mod 257"""
    base = base_hash() if base is None else base
    steps = np.stack([flip(base, range(j)) for j in range(257)])
    return steps[np.arange(n) % 257].copy()


def ladder_descending(n, base=None):
    return ladder(n, base)[::-1].copy()


def ladder_shuffled(n, seed, base=None):
    return ladder(n, base)[np.random.default_rng(seed).permutation(n)].copy()


def identical(n, h=None):
    """a degenerate block: n copies of one hash"""
    return np.tile(base_hash(11) if h is None else h, (n, 1))


def complement(h):
    return np.bitwise_not(np.asarray(h, np.uint8))


def at_distance(h, d, rng):
    """a hash exactly d bits from h, the bits chosen by rng"""
    return flip(h, rng.choice(256, d, replace=False))


def with_variants(hashes, rng=None, far=None):
    """[n, 8, 32]: row 0 = the hash, rows 1-7 random (rng) or copies of `far`"""
    hashes = np.asarray(hashes, np.uint8)
    rows = np.empty((len(hashes), 8, 32), np.uint8)
    rows[:, 0] = hashes
    rows[:, 1:] = rng.integers(0, 256, (len(hashes), 7, 32), dtype=np.uint8) if far is None else far
    return rows


def decoys(hashes, query, rng, near=3):
    """(rows, has_features) where every file has features 0 and its rows 1-7 lie within `near` bits of the query: a form that reads
    them reports the file at that distance instead of its own"""
    rows = with_variants(hashes, rng)
    for i in range(len(rows)):
        for v in range(1, 8):
            rows[i, v] = at_distance(query, int(rng.integers(0, near + 1)), rng)
    return rows, np.zeros(len(rows), np.uint8)


def random_library(n, nv, seed):
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, 256, (n, nv, 32), dtype=np.uint8)
    return rows, rng
