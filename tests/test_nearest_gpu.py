"""The nearest files of a query on the GPU (-m gpu): the two kernels of nearest_kernels.hip at their block, segment and tile seams, in
every arrival order, with ties, extremes, decoy rows, cutoffs and padding, and the context, device and library forms against the numpy
model of the rule (nearest_model.py) and against the threshold sweep.  Every comparison is exact equality of all n_q x k slots and
counts.  The sizes come from rph_debug_nearest_layout; refused calls are only ever refused: no test makes a kernel read out of range."""
import ctypes as C

import numpy as np
import pytest

import library_corpus as lc
import nearest_model as nm

pytestmark = pytest.mark.gpu

FORCED_SEGMENT = 40  # files: 10 blocks of 4 files (8 rows each), or, rounded up to 64, 2 blocks of 32 files (1 row each)
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def eng():
    from rupphash_amd import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.fixture
def short_segments(request):
    from rupphash_amd import Engine

    Engine.nearest_set_segment(FORCED_SEGMENT)
    request.addfinalizer(lambda: Engine.nearest_set_segment(0))


def layout(nv, n_lib=10000, n_q=1, k=1):
    """FB, SEG, QT as the library reports them under the knob in force"""
    from rupphash_amd import Engine

    fb, seg, qt, _ = Engine.nearest_layout(n_lib, nv, n_q, k)
    return fb, seg, qt


def rows_of(hashes, nv, rng):
    """a library of these hashes: as they are, or as row 0 of 8 with random rows behind"""
    return np.array(hashes, np.uint8).reshape(-1, 1, 32) if nv == 1 else nm.with_variants(hashes, rng)


def check(eng, rows, hq, k, **kw):
    got = eng.hamming_nearest(rows, hq, k, **kw)
    nm.same(got, nm.nearest(rows, hq, k, **kw))
    return got


def dev_form(eng, rows, hq, k, max_dist=256, has_features=None, skip=None, nv=None, misalign=0, with_counts=True):
    """rph_hamming_nearest_dev on uploaded arrays, outputs prefilled with a sentinel: (status, edges, counts).  with_counts False: the
    call gets no counts pointer, and the prefilled buffer, allocated next to the slots all the same, comes back as it is"""
    from rupphash_amd import EDGE_DTYPE, RphError

    rows, hq = nm.as_rows(rows), np.ascontiguousarray(hq, np.uint8).reshape(-1, 32)
    slots = min(max(k, 1), nm.MAX_K)
    edges, counts = np.full(len(hq) * slots * EDGE_DTYPE.itemsize, SENTINEL, np.uint8), np.full(len(hq) * 4, SENTINEL, np.uint8)
    held = []

    def up(a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        held.append(eng.dev_alloc(max(a.nbytes, 16) + 16))
        if a.nbytes:
            eng.dev_upload(held[-1], a)
        return held[-1]

    status = 0
    try:
        d_out, d_counts = up(edges), up(counts)
        d_rows = up(rows)
        try:
            eng.hamming_nearest_dev((d_rows or 0) + misalign if misalign else d_rows, rows.shape[1] if nv is None else nv, len(rows), up(hq), len(hq), k, d_out,
                                    max_dist=max_dist, d_has_features=up(None if has_features is None else np.asarray(has_features, np.uint8)),
                                    d_skip=up(None if skip is None else np.asarray(skip, np.uint32)), d_counts=d_counts if with_counts else None)
        except RphError as e:
            status = e.status
        eng.synchronize()
        eng.dev_download(edges, d_out, edges.nbytes)
        eng.dev_download(counts, d_counts, counts.nbytes)
    finally:
        for p in held:
            eng.dev_free(p)
    return status, edges.view(EDGE_DTYPE).reshape(len(hq), slots), counts.view(np.uint32)


# ---- seams ----
@pytest.mark.parametrize("nv", [1, 8])
def test_seams_of_block_segment_and_tile(eng, short_segments, nv):
    fb, seg, qt = layout(nv)
    assert seg % fb == 0 and seg >= FORCED_SEGMENT and qt >= 2
    n_libs = [1, fb - 1, fb, fb + 1, seg - 1, seg, seg + 1, 2 * seg + fb + 1]
    n_qs = [1, qt - 1, qt, qt + 1, 2 * qt + 3]
    ks = [1, 2, 7, 64]
    rng = np.random.default_rng(40 + nv)
    pool = rng.integers(0, 256, (max(n_libs), nv, 32), dtype=np.uint8)
    queries = rng.integers(0, 256, (max(n_qs), 32), dtype=np.uint8)
    flags = (rng.random(max(n_libs)) < 0.7).astype(np.uint8)
    seen = set()
    for t, n_lib in enumerate(n_libs):
        for n_q, k in ((n_qs[t % 5], ks[t % 4]), (n_qs[(t + 2) % 5], ks[(t + 1) % 4]), (n_qs[(t + 3) % 5], ks[(t + 2) % 4])):
            skip = [int(rng.integers(0, n_lib)) if q % 3 == 0 else None for q in range(n_q)]
            check(eng, pool[:n_lib], queries[:n_q], k, has_features=flags[:n_lib] if nv == 8 else None, skip=skip)
            seen.add((n_lib, n_q, k))
    for axis, values in enumerate((n_libs, n_qs, ks)):  # every value of an axis against at least two values of each other axis
        for v in values:
            met = [s for s in seen if s[axis] == v]
            for other in {0, 1, 2} - {axis}:
                assert len({s[other] for s in met}) >= 2, (axis, v, other)


@pytest.mark.parametrize("nv", [1, 8])
def test_where_the_winner_sits(eng, short_segments, nv):
    fb, seg, _ = layout(nv)
    rng = np.random.default_rng(50 + nv)
    n = 2 * seg + fb + 1
    q = nm.base_hash(31)
    hashes = np.stack([nm.at_distance(q, 90 + int(rng.integers(0, 60)), rng) for _ in range(n)])
    for at in (0, n - 1, seg - 1, seg):
        lib = rows_of(hashes, nv, rng)
        lib[at, 0] = nm.at_distance(q, 2, rng)
        e, _ = check(eng, lib, q[None], 3)
        assert (e["i"][0, 0], e["d"][0, 0], e["flags"][0, 0]) == (at, 2, 0)
    if nv == 8:  # its best row as variant 7 of the library's last file
        lib = rows_of(hashes, nv, rng)
        lib[n - 1, 7] = nm.at_distance(q, 1, rng)
        e, _ = check(eng, lib, q[None], 3)
        assert (e["i"][0, 0], e["d"][0, 0], e["flags"][0, 0] >> nm.VARIANT_SHIFT) == (n - 1, 1, 7)


# ---- arrival order ----
@pytest.mark.parametrize("nv", [1, 8])
@pytest.mark.parametrize("k", [7, 64])
def test_arrival_order(eng, short_segments, nv, k):
    base = nm.base_hash()
    rng = np.random.default_rng(60 + nv + k)
    far = nm.complement(base)  # rows 1-7 at 256 from the base: the ladder alone decides
    for hashes in (nm.ladder_descending(600, base), nm.ladder(600, base), nm.ladder_shuffled(600, 5, base)):
        lib = hashes.reshape(-1, 1, 32) if nv == 1 else nm.with_variants(hashes, far=far)
        e, c = check(eng, lib, np.stack([base, hashes[77], nm.at_distance(base, 40, rng)]), k)
        assert e["d"][0, :7].tolist() == [0, 0, 0, 1, 1, 1, 2] and c[0] == k
    # more than k eligible files inside one block: a block of near files among far ones
    fb, _, _ = layout(nv)
    hashes = np.stack([nm.at_distance(base, 100 + int(rng.integers(0, 50)), rng) for _ in range(3 * fb + 1)])
    for j in range(fb):
        hashes[fb + j] = nm.at_distance(base, 1 + (j * 7) % 5, rng)
    check(eng, rows_of(hashes, nv, rng), base[None], 2)


# ---- ties ----
@pytest.mark.parametrize("nv", [1, 8])
def test_ties(eng, short_segments, nv):
    fb, seg, _ = layout(nv)
    rng = np.random.default_rng(70 + nv)
    h = nm.base_hash(11)
    n = 2 * seg + 5
    lib = rows_of(nm.identical(n, h), nv, rng)
    for k in (1, 7, 64):
        e, c = check(eng, lib, h[None], k)
        assert e["i"][0].tolist() == list(range(k)) and (e["d"] == 0).all()
    e, _ = check(eng, lib, np.stack([h, h]), 7, skip=[3, 0])
    assert e["i"][0].tolist() == [0, 1, 2, 4, 5, 6, 7] and e["i"][1].tolist() == [1, 2, 3, 4, 5, 6, 7]
    # twins on the last file of a segment and the first of the next, and on files that the two lane halves of a wave own
    half = (1, 2) if nv == 8 else (3, 4)
    for pair in ((seg - 1, seg), half, (half[0] + fb, half[1] + fb)):
        hashes = np.stack([nm.at_distance(h, 60 + int(rng.integers(0, 90)), rng) for _ in range(n)])
        hashes[pair[0]] = hashes[pair[1]] = nm.at_distance(h, 9, rng)
        e, _ = check(eng, rows_of(hashes, nv, rng), h[None], 2)
        assert e["i"][0].tolist() == list(pair) and e["d"][0].tolist() == [9, 9]


# ---- extremes ----
@pytest.mark.parametrize("nv", [1, 8])
def test_extremes_and_no_phantom_neighbour_at_128(eng, short_segments, nv):
    fb, seg, qt = layout(nv)
    rng = np.random.default_rng(80 + nv)
    base = nm.base_hash()
    far = nm.complement(base)
    # 0 and 256 in one library, next to files at exactly 128; every row 1-7 at 128 from both queries
    hashes = np.stack([nm.at_distance(base, 128, rng) for _ in range(seg + 3)])
    hashes[5], hashes[seg + 1] = far, base
    lib = hashes.reshape(-1, 1, 32) if nv == 1 else nm.with_variants(hashes, far=nm.at_distance(base, 128, rng))
    lib[5, :] = far  # all of its rows: the file is at 256 from the base
    e, c = check(eng, lib, np.stack([base, far]), 64)
    assert (e["i"][0, 0], e["d"][0, 0]) == (seg + 1, 0) and (e["i"][1, 0], e["d"][1, 0]) == (5, 0) and c.tolist() == [min(64, seg + 3)] * 2
    if seg + 3 <= 64:  # the whole library fits the list: the complement comes last, at 256
        assert (e["i"][0, seg + 2], e["d"][0, seg + 2]) == (5, 256) and (e["d"][0, 1:seg + 2] == 128).all()
    # a library shorter than one block, every file at 200: a dead row, file or column that leaks in is a neighbour at 128
    for n in (1, fb - 1) if fb > 2 else (1,):
        hashes = np.stack([nm.at_distance(base, 200, rng) for _ in range(n)])
        lib = hashes.reshape(-1, 1, 32) if nv == 1 else nm.with_variants(hashes, far=far)
        for n_q in (1, qt + 1):
            e, c = check(eng, lib, np.tile(base, (n_q, 1)), 64)
            assert (c == n).all() and (e["d"][:, :n] == 200).all() and (e["i"][:, n:] == nm.NO_FILE).all()


def test_has_features_mixes_with_decoy_rows(eng, short_segments):
    fb, seg, _ = layout(8)
    rng = np.random.default_rng(90)
    q = nm.base_hash(22)
    n = seg + fb + 3
    hashes = np.stack([nm.at_distance(q, 70 + (i * 13) % 90, rng) for i in range(n)])
    rows, hf = nm.decoys(hashes, q, rng)
    e, c = check(eng, rows, q[None], 64, has_features=hf)
    assert e["d"][0].min() >= 70 and (e["flags"] == 0).all()
    hf[rng.random(n) < 0.5] = 1
    hf[[0, 1, n - 1]] = 1, 0, 1
    e, _ = check(eng, rows, np.stack([q, hashes[1]]), 64, has_features=hf)
    assert (e["i"][0, 0], e["i"][1, 0], e["d"][1, 0]) == (0, 1, 0)  # file 0 through a decoy it owns, file 1 as its own hash
    check(eng, rows, q[None], 64)  # without the flags every file owns its decoys


@pytest.mark.parametrize("max_dist", [0, 31, 255, 256, 1000])
def test_cutoffs(eng, short_segments, max_dist):
    base = nm.base_hash()
    hashes = np.concatenate([nm.ladder_shuffled(300, 4, base), nm.complement(base)[None], base[None]])
    q = np.stack([base, nm.complement(base)])
    for nv in (1, 8):
        lib = hashes.reshape(-1, 1, 32) if nv == 1 else nm.with_variants(hashes, far=nm.at_distance(base, 128, np.random.default_rng(3)))
        e, c = check(eng, lib, q, 64, max_dist=max_dist)
        if max_dist == 0:
            assert c.tolist() == [3, 2]


def test_k_above_the_library(eng, short_segments):
    rng = np.random.default_rng(100)
    for nv in (1, 8):
        rows, _ = nm.random_library(5, nv, 101 + nv)
        q = rng.integers(0, 256, (3, 32), dtype=np.uint8)
        e, c = check(eng, rows, q, 64, skip=[None, 2, None])
        assert c.tolist() == [5, 4, 5] and (e["d"][1, 4:] == 0xFFFF).all() and (e["j"][1] == 1).all()
    e, c = check(eng, np.zeros((0, 8, 32), np.uint8), q, 3)  # an empty library
    assert (c == 0).all() and (e["i"] == nm.NO_FILE).all()
    e, c = eng.hamming_nearest(rows, np.zeros((0, 32), np.uint8), 3)  # no queries
    assert e.shape == (0, 3) and c.shape == (0,)


@pytest.mark.parametrize("nv", [1, 8])
def test_many_segments_and_the_default_layout_give_the_same_bytes(eng, nv):
    from rupphash_amd import Engine

    rows, rng = nm.random_library(5000, nv, 110 + nv)
    q = np.concatenate([rng.integers(0, 256, (90, 32), dtype=np.uint8), rows[rng.integers(0, 5000, 10), 0]])
    hf = (rng.random(5000) < 0.8).astype(np.uint8) if nv == 8 else None
    want = nm.nearest(rows, q, 10, has_features=hf)
    try:
        Engine.nearest_set_segment(8)  # two blocks of 4 files, or one of 32
        n_forced = Engine.nearest_layout(5000, nv, 100, 10)[3]
        forced = eng.hamming_nearest(rows, q, 10, has_features=hf)
    finally:
        Engine.nearest_set_segment(0)
    assert n_forced >= 5000 // 32 and Engine.nearest_layout(5000, nv, 100, 10)[3] * 2 <= n_forced
    default = eng.hamming_nearest(rows, q, 10, has_features=hf)
    nm.same(forced, want)
    nm.same(default, want)
    assert forced[0].tobytes() == default[0].tobytes() and forced[1].tobytes() == default[1].tobytes()
    status, e, c = dev_form(eng, rows, q, 10, has_features=hf)
    assert status == 0
    nm.same((e, c), want)


def test_layout_keeps_its_bounds():
    from rupphash_amd import Engine

    for n_lib, nv, n_q, k in ((1, 8, 1, 1), (10**6, 8, 1, 10), (10**6, 8, 10**4, 64), (2**32 - 2, 1, 1, 64), (2**32 - 2, 8, 10**6, 64), (10**7, 1, 32, 1)):
        fb, seg, qt, n_segs = Engine.nearest_layout(n_lib, nv, n_q, k)
        assert fb == (4 if nv == 8 else 32) and seg % fb == 0 and seg <= 1 << 20 and n_segs == -(-n_lib // seg)
        assert n_segs * qt * k * 4 <= 256 << 20            # one tile of queries always fits the workspace
        if n_lib >= 10**6 and n_q <= 32:
            assert n_segs >= 1024                          # one query against a large library spreads over the device


# ---- the library forms ----
N_LIB_FILES = 600


def host_copy(f, keep):
    """rows, flags and hashes of the corpus files `keep` as the library holds them"""
    rows = f.dih[keep].copy()
    rows[:, 0] = f.hashes[keep]
    return rows, f.has_features[keep].copy(), f.hashes[keep].copy()


@pytest.fixture(scope="module")
def files(oracle):
    return lc.corpus()


def state(lib):
    return lib.groups(), lib.labels().tolist(), lib.comparisons, len(lib)


def test_library_forms(eng, files, short_segments):
    from rupphash_amd import EDGE_DTYPE, _lib

    f = files
    rng = np.random.default_rng(120)
    keep = np.arange(N_LIB_FILES)
    queries = np.concatenate([f.hashes[rng.integers(0, lc.N_FILES, 40)], rng.integers(0, 256, (5, 32), dtype=np.uint8)])
    with eng.library(40) as lib:
        for first, last in ((0, 250), (250, N_LIB_FILES)):  # an append in two pieces
            lib.append(f.hashes[first:last], f.coeffs[first:last], f.has_features[first:last], f.quality[first:last])
        for round_ in range(2):
            rows, hf, hashes = host_copy(f, keep)
            before = state(lib)
            want = eng.hamming_nearest(rows, queries, 10, has_features=hf)
            nm.same(want, nm.nearest(rows, queries, 10, has_features=hf))
            nm.same(lib.nearest(queries, 10), want)
            nm.same(lib.nearest(queries, 64, max_dist=40), eng.hamming_nearest(rows, queries, 64, max_dist=40, has_features=hf))
            # resident files as queries (one of them twice)
            idx = np.array([0, 5, len(keep) - 1, 17, 5], np.uint32)
            nm.same(lib.nearest_files(idx, 7), eng.hamming_nearest(rows, hashes[idx], 7, has_features=hf, skip=idx))
            # an index at the size: refused, outputs untouched
            out = np.full(2 * 7 * EDGE_DTYPE.itemsize, SENTINEL, np.uint8)
            cnt = np.full(8, SENTINEL, np.uint8)
            bad = np.array([3, len(keep)], np.uint32)
            rc = lib.L.rph_library_nearest_files(lib.handle, bad.ctypes.data_as(C.c_void_p), 2, 7, 256, out.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p))
            assert rc == _lib.RPH_ERR_INVALID_ARG and (out == SENTINEL).all() and (cnt == SENTINEL).all()
            rc = lib.L.rph_library_nearest(lib.handle, queries.ctypes.data_as(C.c_void_p), 2, 65, 256, out.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p))
            assert rc == _lib.RPH_ERR_INVALID_ARG and (out == SENTINEL).all() and (cnt == SENTINEL).all()
            assert state(lib) == before  # groups, labels, comparison count and size
            if round_ == 0:  # after a removal, in the renumbered indices
                gone = np.unique(rng.integers(0, N_LIB_FILES, 50)).astype(np.uint32)
                lib.remove(gone)
                keep = np.setdiff1d(keep, gone)
    with eng.library(40) as lib:  # a true twin: the same file appended twice
        twice = np.concatenate([np.arange(30), [7]])
        lib.append(f.hashes[twice], f.coeffs[twice], f.has_features[twice], f.quality[twice])
        rows, hf, hashes = host_copy(f, twice)
        e, c = lib.nearest_files([7, 30], 3)
        nm.same((e, c), nm.nearest(rows, hashes[[7, 30]], 3, has_features=hf, skip=[7, 30]))
        assert (e["i"][0, 0], e["d"][0, 0], e["i"][1, 0], e["d"][1, 0]) == (30, 0, 7, 0)
        e, c = lib.nearest(np.zeros((0, 32), np.uint8), 3)
        assert e.shape == (0, 3)
    with eng.library(40) as lib:  # an empty library
        e, c = lib.nearest(queries[:3], 4)
        assert (e["i"] == nm.NO_FILE).all() and (c == 0).all()


@pytest.mark.parametrize("s", [0, 31, 63])
def test_nearest_with_a_cutoff_equals_the_threshold_sweep(eng, files, s):
    f = files
    rng = np.random.default_rng(130 + s)
    keep = np.arange(N_LIB_FILES)
    rows, hf, hashes = host_copy(f, keep)
    queries = np.concatenate([f.hashes[rng.integers(0, N_LIB_FILES, 60)], rng.integers(0, 256, (4, 32), dtype=np.uint8)])
    dist, variant = nm.file_distances(rows, queries, hf)
    assert ((dist <= s).sum(axis=0) <= 64).all()  # the premise: no query has more than 64 files within s
    assert (dist <= s).sum() >= 20
    with eng.library(s) as lib:
        lib.append(f.hashes[:N_LIB_FILES], f.coeffs[:N_LIB_FILES], f.has_features[:N_LIB_FILES])  # no qualities: nobody is low-confidence
        e, c = lib.nearest(queries, 64, max_dist=s)
        swept = lib.query(queries)
    best = {}
    for i, j, d, flags in swept.tolist():
        key = (d, (flags & 0x0E00) >> nm.VARIANT_SHIFT)
        best[(i, j)] = min(best.get((i, j), key), key)
    got = {(int(x["i"]), int(x["j"])): (int(x["d"]), int(x["flags"]) >> nm.VARIANT_SHIFT) for q in range(len(queries)) for x in e[q, :c[q]]}
    assert got == best
    assert sum(c.tolist()) == len(best) == int((dist <= s).sum())


# ---- refused calls ----
def test_refused_device_calls_write_nothing_and_the_next_call_is_right(eng):
    from rupphash_amd import _lib

    rows, rng = nm.random_library(50, 8, 140)
    q = rng.integers(0, 256, (3, 32), dtype=np.uint8)
    for bad in (dict(k=0), dict(k=65), dict(nv=3), dict(nv=0), dict(misalign=8)):
        k = bad.pop("k", 5)
        status, e, c = dev_form(eng, rows, q, k, **bad)
        assert status == _lib.RPH_ERR_INVALID_ARG, bad
        assert (e.view(np.uint8) == SENTINEL).all() and (c.view(np.uint8) == SENTINEL).all(), bad
    from rupphash_amd import RphError
    with pytest.raises(RphError) as err:
        eng.hamming_nearest(rows, q, 65)
    assert err.value.status == _lib.RPH_ERR_INVALID_ARG
    status, e, c = dev_form(eng, rows, q, 5, skip=[1, nm.NO_FILE, 2])
    assert status == 0
    nm.same((e, c), nm.nearest(rows, q, 5, skip=[1, None, 2]))
    status, e, c = dev_form(eng, rows, q, 5)  # counts are optional: checked through the library's and context's forms, here present
    nm.same((e, c), nm.nearest(rows, q, 5))
