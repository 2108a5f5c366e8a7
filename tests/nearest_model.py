"""The rule of rph_hamming_nearest (include/rupphash.h) in numpy, and builders of libraries whose answers are known in closed form.
Shared by test_nearest_cpu.py, test_nearest_gpu.py and test_nearest_grid_gpu.py; nothing here touches the library under test."""
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


_BYTE_ONES = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(axis=1).astype(np.uint8)
POPCOUNT_TEMP_WORDS = 1 << 23  # uint64 words of XOR that distances_popcount holds at a time (64 MiB)


def _ones64(x):
    """set bits of every uint64, as uint8"""
    if hasattr(np, "bitwise_count"):
        return np.bitwise_count(x)
    return _BYTE_ONES[x.view(np.uint8).reshape(x.shape + (8,))].sum(axis=-1, dtype=np.uint8)


def distances_popcount(rows, hashes_q):
    """distances() by XOR on uint64 views and a population count, in blocks of rows and queries (one query at a time against a large
    library) so that the temporaries stay at POPCOUNT_TEMP_WORDS whatever the sizes: what the large libraries and the long query lists
    are checked with"""
    rows = as_rows(rows)
    n, nv, _ = rows.shape
    r = rows.reshape(n * nv, 32).view(np.uint64)                                     # [n nv, 4]
    q = np.ascontiguousarray(hashes_q, np.uint8).reshape(-1, 32).view(np.uint64)     # [nq, 4]
    d = np.empty((n * nv, len(q)), np.int32)
    r_step = max(1, POPCOUNT_TEMP_WORDS // 4)
    q_step = max(1, POPCOUNT_TEMP_WORDS // (4 * max(min(n * nv, r_step), 1)))
    for r0 in range(0, n * nv, r_step):
        for q0 in range(0, len(q), q_step):
            x = r[r0:r0 + r_step, None, :] ^ q[None, q0:q0 + q_step, :]
            d[r0:r0 + r_step, q0:q0 + q_step] = _ones64(x).sum(axis=2, dtype=np.int32)
    return d.reshape(n, nv, len(q))


def file_distances(rows, hashes_q, has_features=None, distances=distances):
    """(dist[i, q], variant[i, q]): minimum over the rows a file owns and the smallest row attaining it"""
    d = distances(rows, hashes_q)
    if has_features is not None and d.shape[1] > 1:
        plain = np.asarray(has_features, np.uint8) == 0
        d[plain, 1:, :] = 1 << 20  # rows 1.. of a file without features are not its own
    return d.min(axis=1), d.argmin(axis=1)  # argmin: the first (smallest) index of the minimum


def _empty_result(nq, k):
    edges = np.zeros((nq, k), EDGE_DTYPE)
    edges["i"], edges["d"] = NO_FILE, EMPTY_D
    edges["j"] = np.arange(nq, dtype=np.uint32)[:, None]
    return edges, np.zeros(nq, np.uint32)


def nearest_vectorised(rows, hashes_q, k, max_dist=256, has_features=None, skip=None, distances=distances_popcount):
    """nearest() without a Python loop over the queries, for thousands to a million of them: one sort along the file axis of the key
    (dist, file), files that the cutoff or skip excludes pushed behind every real key"""
    rows = as_rows(rows)
    hq = np.ascontiguousarray(hashes_q, np.uint8).reshape(-1, 32)
    n, nq = len(rows), len(hq)
    edges, counts = _empty_result(nq, k)
    if n == 0 or nq == 0:
        return edges, counts
    dist, variant = file_distances(rows, hq, has_features, distances)
    out = dist > max_dist
    if skip is not None:
        sk = np.array([NO_FILE if x is None else int(x) for x in skip], np.int64)
        has = np.flatnonzero(sk < n)
        out[sk[has], has] = True
    key = dist.astype(np.int64) << 32 | np.arange(n, dtype=np.int64)[:, None]
    key[out] = np.iinfo(np.int64).max
    m = min(k, n)
    key = np.sort(key, axis=0)[:m].T                      # [nq, m]
    filled = key != np.iinfo(np.int64).max
    got = np.where(filled, key & 0xFFFFFFFF, 0)
    at = np.arange(nq)[:, None]
    edges["i"][:, :m] = np.where(filled, got, NO_FILE)
    edges["d"][:, :m] = np.where(filled, key >> 32, EMPTY_D)
    edges["flags"][:, :m] = np.where(filled, variant[got, at] << VARIANT_SHIFT, 0)
    counts[:] = filled.sum(axis=1)
    return edges, counts


def nearest(rows, hashes_q, k, max_dist=256, has_features=None, skip=None, distances=distances):
    """(edges[n_q, k], counts[n_q]) as every form of the call must return them"""
    rows = as_rows(rows)
    hq = np.ascontiguousarray(hashes_q, np.uint8).reshape(-1, 32)
    n, nq = len(rows), len(hq)
    edges, counts = _empty_result(nq, k)
    if n == 0 or nq == 0:
        return edges, counts
    dist, variant = file_distances(rows, hq, has_features, distances)
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
