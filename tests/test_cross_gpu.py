"""Cross-set Hamming sweeps and the incremental grouping on the GPU (-m gpu): rph_hamming_cross_pairs, rph_hamming_variant_cross_pairs,
their _dev forms and rph_group_files_pdq_append.  Every edge-set test runs under the three formulations of the fast path (fp4 MFMA,
int8 MFMA, VALU), which must agree edge for edge, flags included, and is compared with a brute force or a set known by construction."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KERNELS = (2, 1, 0)


@pytest.fixture(scope="module")
def eng():
    from rupphash_amd import Engine

    e = Engine(0)
    yield e
    e.set_hamming_kernel(2)
    e.close()


def canon(edges):
    """the edge list ordered by (i, j, flags, d)"""
    pair = (edges["i"].astype(np.uint64) << np.uint64(32)) | edges["j"].astype(np.uint64)
    rest = (edges["flags"].astype(np.uint32) << np.uint32(16)) | edges["d"].astype(np.uint32)
    return edges[np.lexsort((rest, pair))]


def ijd(edges):
    return sorted((int(e["i"]), int(e["j"]), int(e["d"])) for e in edges)


def under_every_kernel(eng, run):
    """run() under kernel settings 2, 1 and 0: the three edge lists are identical as sets of (i, j, d, flags); returns the list
    in canonical order.  Kernel 2 is restored."""
    got = None
    try:
        for k in KERNELS:
            eng.set_hamming_kernel(k)
            e = canon(run())
            if got is None:
                got = e
            assert np.array_equal(e, got), f"kernel {k} differs from kernel {KERNELS[0]}"
    finally:
        eng.set_hamming_kernel(2)
    return got


def flip_bits(rng, h, d):
    v = h.copy()
    for b in rng.choice(256, d, replace=False):
        v[b // 8] ^= 1 << (b % 8)
    return v


def cross_data(rng, n_a, n_b):
    """Two sets with clusters that span them, and exact duplicates shared at the SAME index on both sides (a[k] == b[k])."""
    a = rng.integers(0, 256, (n_a, 32), dtype=np.uint8)
    b = rng.integers(0, 256, (n_b, 32), dtype=np.uint8)
    for _ in range(30):
        base = rng.integers(0, 256, 32, dtype=np.uint8)
        for i in rng.integers(0, n_a, 3):
            a[i] = flip_bits(rng, base, int(rng.integers(0, 36)))
        for j in rng.integers(0, n_b, 3):
            b[j] = flip_bits(rng, base, int(rng.integers(0, 36)))
    m = min(n_a, n_b)
    same = sorted({0, m - 1, m // 2, m // 3, min(31, m - 1), min(32, m - 1)})
    for k in same:
        b[k] = a[k]
    return a, b, same


def expected_cross(oracle, a, b, thr):
    n_a = len(a)
    both = oracle.all_pairs256(np.concatenate([a, b]), thr)
    return sorted((int(i), int(j) - n_a, int(d)) for i, j, d in both if i < n_a <= j)


SHAPES = [(1, 1), (1, 2500), (2500, 1), (33, 31), (1025, 129), (1023, 2049)]


# ------------------------------------------------------------------ 1. brute force at the smallest shapes that can go wrong
@pytest.mark.parametrize("n_a,n_b", SHAPES)
def test_cross_pairs_match_brute_force(eng, oracle, n_a, n_b):
    rng = np.random.default_rng(1000 * n_a + n_b)
    a, b, same = cross_data(rng, n_a, n_b)
    for thr in (0, 31, 40, 63, 70):
        want = expected_cross(oracle, a, b, thr)
        got = under_every_kernel(eng, lambda: eng.hamming_cross_pairs(a, b, thr))
        assert ijd(got) == want, (n_a, n_b, thr)
        assert all(i < n_a and j < n_b for i, j, _ in ijd(got))
        pairs = {(i, j) for i, j, _ in want}
        for k in same:  # what the square kernel's `col <= owner` rule would drop
            assert (k, k) in pairs
        assert thr < 40 or len(want) > len(same) or min(n_a, n_b) == 1  # the clusters span the two sets


# ------------------------------------------------------------------ 2. symmetry
@pytest.mark.parametrize("n_a,n_b", [(33, 31), (1025, 129), (2500, 1)])
def test_cross_pairs_are_symmetric(eng, n_a, n_b):
    rng = np.random.default_rng(77 + n_a)
    a, b, _ = cross_data(rng, n_a, n_b)
    ab = under_every_kernel(eng, lambda: eng.hamming_cross_pairs(a, b, 40))
    ba = under_every_kernel(eng, lambda: eng.hamming_cross_pairs(b, a, 40))
    swapped = ba.copy()
    swapped["i"], swapped["j"] = ba["j"], ba["i"]
    assert len(ab) > 0 and np.array_equal(canon(swapped), ab)


# ------------------------------------------------------------------ 3. heavily duplicated data: the queue-overflow fallback
@pytest.mark.parametrize("thr", [0, 40])
def test_identical_hashes_every_pair_once(eng, thr):
    from rupphash_amd import EDGE_DTYPE, _lib

    h = np.random.default_rng(3).integers(0, 256, 32, dtype=np.uint8)
    a, b = np.tile(h, (1100, 1)), np.tile(h, (600, 1))
    got = under_every_kernel(eng, lambda: eng.hamming_cross_pairs(a, b, thr))
    assert len(got) == 660_000
    key = got["i"].astype(np.int64) * 600 + got["j"]
    assert got["i"].max() == 1099 and got["j"].max() == 599 and len(np.unique(key)) == 660_000
    assert (got["d"] == 0).all()
    # capacity protocol: the total is reported even when it does not fit
    edges = np.zeros(10, EDGE_DTYPE)
    found = C.c_uint64()
    rc = eng.L.rph_hamming_cross_pairs(eng.ctx, a.ctypes.data_as(C.c_void_p), 1100, b.ctypes.data_as(C.c_void_p), 600, thr, 0, 1,
                                       edges.ctypes.data_as(C.c_void_p), 10, C.byref(found))
    assert rc == _lib.RPH_ERR_CAPACITY and found.value == 660_000
    assert (edges["i"] < 1100).all() and (edges["j"] < 600).all() and (edges["d"] == 0).all()


def test_empty_sides_and_oversized_counts(eng):
    from rupphash_amd import RphError, _lib

    h = np.zeros((5, 32), np.uint8)
    none = np.zeros((0, 32), np.uint8)
    assert len(eng.hamming_cross_pairs(h, none, 40)) == 0 and len(eng.hamming_cross_pairs(none, h, 40)) == 0
    found = C.c_uint64(9)
    for n_a, n_b in ((2**32, 5), (5, 2**32)):  # refused before anything is read
        rc = eng.L.rph_hamming_cross_pairs(eng.ctx, h.ctypes.data_as(C.c_void_p), n_a, h.ctypes.data_as(C.c_void_p), n_b, 40, 0, 1, None, 0,
                                           C.byref(found))
        assert rc == _lib.RPH_ERR_INVALID_ARG
    with pytest.raises(RphError):
        eng.group_files_pdq_append(h, [], h, 64)


# ------------------------------------------------------------------ 4. segments longer than one tile; tile, chunk and segment edges
def edge_indices(n):
    out = [0, 127, 128, 255, 256, 1023, 1024, n - 1]
    for k in list(range(1, 17)) + [n // 1024]:
        out += [1024 * k - 1, 1024 * k]
    return sorted({x for x in out if 0 <= x < n})


@pytest.fixture(scope="module")
def planted():
    """Uniform random hashes with planted pairs at distances 0 .. 46.  No unplanted pair of uniform 256-bit hashes lies within 46 bits
    (46 is more than 10 sigma below the mean of 128: over 8.6e9 pairs the expected count is far below 1e-10), so the edge set at
    threshold 40 is exactly the planted pairs of distance <= 40.  Every column is derived from one row; rows are unrelated.
    Returns (a, b, the planted pairs within 40, those at 41 .. 46)."""
    n_a, n_b = 65_536 + 5, 131_072 + 37
    rng = np.random.default_rng(4040)
    a = rng.integers(0, 256, (n_a, 32), dtype=np.uint8)
    b = rng.integers(0, 256, (n_b, 32), dtype=np.uint8)
    rows = edge_indices(n_a) + sorted(set(rng.integers(0, n_a, 50).tolist()))
    cols = sorted(set(edge_indices(n_b) + rng.integers(0, n_b, 70).tolist()))
    order = rng.permutation(len(cols))
    want, absent = [], []
    for t, ci in enumerate(order):
        c, r, d = cols[ci], rows[t % len(rows)], t % 47
        b[c] = flip_bits(rng, a[r], d)
        (want if d <= 40 else absent).append((r, c, d))
    assert len(cols) >= 2 * 47 and len(cols) >= len(rows)  # every distance twice, every planted row used
    assert {d for _, _, d in want} == set(range(41)) and {d for _, _, d in absent} == set(range(41, 47))
    return a, b, sorted(want), sorted(absent)


def test_planted_pairs_across_tiles_chunks_and_segments(eng, planted):
    """At thresholds 50 and 60 the edge set is every planted pair: the binomial tail puts the expected number of unplanted pairs among
    the 8.6e9 at 4.9e-14 (threshold 50) and 2.2e-8 (threshold 60); at 75 it would be 0.12.  The prefix widths are 4 at threshold 40,
    5 (int8 MFMA, VALU) and 6 (fp4 MFMA) at 50, 6 at 60: the wider prefixes under segments of two column tiles and more."""
    a, b, want, absent = planted
    # the launcher's own rule: this rectangle is swept in segments of at least two column tiles by the MFMA kernels
    for k in (2, 1):
        assert eng.hamming_cross_layout(len(a), len(b), kernel=k)[1] >= 2
    assert [[eng.L.rph_hamming_prefix_dwords(thr, k) for k in KERNELS] for thr in (40, 50, 60)] == [[4, 4, 4], [6, 5, 5], [6, 6, 6]]
    for thr in (40, 50, 60):
        got = under_every_kernel(eng, lambda: eng.hamming_cross_pairs(a, b, thr))
        assert ijd(got) == (want if thr == 40 else sorted(want + absent)), thr


def test_planted_pairs_in_three_parts(eng, planted):
    a, b, want, _ = planted
    parts = [under_every_kernel(eng, lambda p=p: eng.hamming_cross_pairs(a, b, 40, part=p, nparts=3)) for p in range(3)]
    assert all(len(p) > 0 for p in parts)
    union = sorted(x for p in parts for x in ijd(p))
    assert union == want  # sorted lists: a pair reported by two parts would appear twice


# ------------------------------------------------------------------ 5. variant cross sweep
def coefficient_pool(rng, n):
    """near-duplicate coefficient sets (small perturbations) and a mirrored copy (sign flip on odd-frequency columns)"""
    coeffs = rng.normal(0, 20, (n, 256)).astype(np.float32)
    for _ in range(60):
        src = rng.integers(0, n)
        for j in rng.choice(n, 3, replace=False):
            coeffs[j] = coeffs[src] + rng.normal(0, 0.8, 256).astype(np.float32)
    return coeffs


def mirror(c):
    m = c.reshape(16, 16).copy()
    m[:, 0::2] *= -1
    return m.ravel()


def test_variant_cross_pairs_match_numpy(eng):
    rng = np.random.default_rng(5150)
    n_a, n_b = 1300, 700
    coeffs = coefficient_pool(rng, n_a + n_b)
    coeffs[n_a + 100] = mirror(coeffs[10])
    coeffs[n_a + 5] = coeffs[1299] + rng.normal(0, 0.8, 256).astype(np.float32)
    hashes, dih = eng.pdq_hashes_from_coeffs(coeffs)
    va, hb = dih[:n_a], hashes[n_a:]
    low_a, low_b = (rng.random(n_a) < 0.15).astype(np.uint8), (rng.random(n_b) < 0.15).astype(np.uint8)
    low_a[10] = low_b[100] = 0  # the mirrored pair stays an ordinary one
    ba = np.unpackbits(va.reshape(-1, 32), axis=1).astype(np.float32)  # (n_a * 8, 256)
    bb = np.unpackbits(hb, axis=1).astype(np.float32)
    dist = (ba.sum(1)[:, None] + bb.sum(1)[None, :] - 2.0 * (ba @ bb.T)).astype(np.int64).reshape(n_a, 8, n_b)  # exact: integers <= 256
    for sim in (0, 31, 40, 63):
        limit = np.where((low_a[:, None] | low_b[None, :]) != 0, 0, sim)
        i, v, j = np.nonzero(dist <= limit[:, None, :])
        want = sorted(zip(i.tolist(), j.tolist(), v.tolist(), dist[i, v, j].tolist()))
        got = under_every_kernel(eng, lambda: eng.hamming_variant_cross_pairs(va, hb, sim, low_conf_a=low_a, low_conf_b=low_b))
        have = sorted(zip(got["i"].tolist(), got["j"].tolist(), ((got["flags"] >> 9) & 7).tolist(), got["d"].tolist()))
        assert have == want, sim
        if sim >= 31:
            assert any(x[2] != 0 for x in want) and len(want) > 100


# ------------------------------------------------------------------ 6. append equals regroup
@pytest.fixture(scope="module")
def files(eng):
    rng = np.random.default_rng(6060)
    n = 1901
    coeffs = coefficient_pool(rng, n)
    coeffs[1500] = coeffs[3] + rng.normal(0, 0.8, 256).astype(np.float32)   # the one new file of (1500, 1) joins the library
    coeffs[1] = coeffs[0] + rng.normal(0, 0.8, 256).astype(np.float32)      # the one library file of (1, 1500) is joined
    coeffs[1400] = mirror(coeffs[10])
    coeffs[1700] = mirror(coeffs[20])
    hashes, dih = eng.pdq_hashes_from_coeffs(coeffs)
    quality = rng.integers(30, 101, n).astype(np.int32)
    quality[::7] = -1
    has_features = (rng.random(n) > 0.1).astype(np.uint8)
    has_features[[0, 1, 3, 10, 20, 1500]] = 1
    quality[[0, 1, 3, 1500]] = 90
    return coeffs, hashes, dih, quality, has_features


@pytest.mark.parametrize("sim", [0, 16, 40, 63])
@pytest.mark.parametrize("n_old,n_new", [(1500, 1), (1500, 400), (1, 1500), (0, 900), (900, 0)])
def test_append_equals_regroup(eng, oracle, files, n_old, n_new, sim):
    coeffs, hashes, dih, quality, hf = (x[: n_old + n_new] for x in files)
    o, w = slice(0, n_old), slice(n_old, n_old + n_new)
    hf_lib_only = hf.copy()
    hf_lib_only[w] = 0
    # (library side, new side, the same call on the concatenation, the oracle's arguments)
    cases = {
        "coefficients on both sides": (dict(coeffs=coeffs[o], has_features=hf[o], quality=quality[o]),
                                       dict(coeffs=coeffs[w], has_features=hf[w], quality=quality[w]),
                                       dict(coeffs=coeffs, has_features=hf, quality=quality),
                                       dict(variants=dih, has_features=hf, quality=quality)),
        "no coefficients": (dict(quality=quality[o]), dict(quality=quality[w]), dict(quality=quality), dict(quality=quality)),
        # the new files have one variant each: on the concatenation that is has_features = 0 for them
        "coefficients on the library only": (dict(coeffs=coeffs[o], has_features=hf[o], quality=quality[o]), dict(quality=quality[w]),
                                             dict(coeffs=coeffs, has_features=hf_lib_only, quality=quality),
                                             dict(variants=dih, has_features=hf_lib_only, quality=quality)),
    }
    for name, (lib_kw, new_kw, all_kw, oracle_kw) in cases.items():
        old_groups, old_cmp = eng.group_files_pdq(hashes[o], sim, **lib_kw)
        want_groups, want_cmp = eng.group_files_pdq(hashes, sim, **all_kw)
        got_groups, new_cmp = eng.group_files_pdq_append(hashes[o], old_groups, hashes[w], sim,
                                                         **{"old_" + k: v for k, v in lib_kw.items()},
                                                         **{"new_" + k: v for k, v in new_kw.items()})
        assert got_groups == want_groups, name
        assert old_cmp + new_cmp == want_cmp, name
        ref_edges, ref_groups = oracle.group_pdq(hashes, sim, **oracle_kw)
        assert got_groups == ref_groups and want_cmp == len(ref_edges), name
        if n_old and n_new and sim >= 16:  # the new files do join the library
            assert new_cmp > 0 and any(g[0] < n_old <= g[-1] for g in got_groups), name


def test_scanner_helper_appends(eng, files):
    from rupphash_amd import scanner

    coeffs, hashes, _, quality, hf = (x[:800] for x in files)
    q = [None if x < 0 else int(x) for x in quality]
    old_groups, old_cmp = scanner.group_with_pdqhash(hashes[:600], 40, coeffs[:600], hf[:600], q[:600], engine=eng)
    want, want_cmp = scanner.group_with_pdqhash(hashes, 40, coeffs, hf, q, engine=eng)
    got, new_cmp = scanner.group_with_pdqhash_append(hashes[:600], old_groups, hashes[600:], 40, coeffs[:600], hf[:600], q[:600], coeffs[600:],
                                                     hf[600:], q[600:], engine=eng)
    assert got == want and old_cmp + new_cmp == want_cmp


# ------------------------------------------------------------------ 7. _dev forms on a caller's stream
def test_dev_forms_on_a_callers_stream(eng, oracle):
    from rupphash_amd import EDGE_DTYPE

    n_a, n_b, thr = 1025, 129, 40
    rng = np.random.default_rng(707)
    a, b, _ = cross_data(rng, n_a, n_b)
    want = expected_cross(oracle, a, b, thr)
    low_a = np.zeros(n_a, np.uint8)
    low_a[::2] = 1
    want_low = [(i, j, d) for i, j, d in want if d == 0 or i % 2 == 1]
    cap = 1 << 14
    d_a, d_b, d_l = eng.dev_alloc(a.nbytes), eng.dev_alloc(b.nbytes), eng.dev_alloc(n_a)
    d_e, d_c = eng.dev_alloc(cap * 12), eng.dev_alloc(8)
    st = eng.stream_create()

    def fetch():
        eng.stream_synchronize(st)
        cnt = np.zeros(1, np.uint64)
        eng.dev_download(cnt, d_c)
        edges = np.zeros(int(cnt[0]), EDGE_DTYPE)
        eng.dev_download(edges, d_e)
        return edges

    def plain():
        eng.dev_memset(d_c, 0, 8, stream=st)
        eng.hamming_cross_pairs_dev(d_a, n_a, d_b, n_b, thr, d_e, cap, d_c, stream=st)
        return fetch()

    def with_flags():
        eng.dev_memset(d_c, 0, 8, stream=st)
        eng.hamming_variant_cross_pairs_dev(d_a, 1, n_a, d_b, n_b, thr, d_e, cap, d_c, d_low_conf_a=d_l, stream=st)
        return fetch()

    try:
        eng.dev_upload(d_a, a)
        eng.dev_upload(d_b, b)
        eng.dev_upload(d_l, low_a)
        eng.synchronize()
        assert ijd(under_every_kernel(eng, plain)) == want
        assert ijd(under_every_kernel(eng, with_flags)) == want_low and 0 < len(want_low) < len(want)
    finally:
        eng.stream_destroy(st)
        for p in (d_a, d_b, d_l, d_e, d_c):
            eng.dev_free(p)
