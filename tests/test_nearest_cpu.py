"""The nearest files of a query on the host (no device): rph_hamming_nearest_host against the numpy model of the rule
(nearest_model.py), the model's distances against rph_hamming_distance256, every refused call with its outputs untouched, and the
Python wrappers' shapes and dtypes."""
import ctypes as C

import numpy as np
import pytest

import nearest_model as nm
from rupphash_amd import EDGE_DTYPE, _lib
from rupphash_amd import engine as engine_module
from rupphash_amd.engine import Engine

host = Engine.hamming_nearest_host


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def test_module_level_export_and_constants():
    assert engine_module.hamming_nearest_host is Engine.hamming_nearest_host
    assert _lib.RPH_NO_FILE == nm.NO_FILE == 0xFFFFFFFF and _lib.RPH_NEAREST_MAX_K == nm.MAX_K == 64
    assert _lib.RPH_EDGE_VARIANT_SHIFT == nm.VARIANT_SHIFT


def test_model_distances_match_the_scalar_function():
    L = _lib.load()
    rows, rng = nm.random_library(9, 8, 1)
    rows[3, 2] = nm.complement(rows[0, 0])
    hq = np.concatenate([rng.integers(0, 256, (4, 32), dtype=np.uint8), rows[0, 0][None]])
    d = nm.distances(rows, hq)
    for i in range(9):
        for v in range(8):
            for q in range(5):
                assert d[i, v, q] == L.rph_hamming_distance256(ptr(rows[i, v]), ptr(hq[q]))
    assert d[0, 0, 4] == 0 and d[3, 2, 4] == 256


def test_ladder_distances_are_closed_form():
    base = nm.base_hash()
    lib = nm.ladder(600, base)
    dist, _ = nm.file_distances(lib, base[None])
    assert np.array_equal(dist[:, 0], np.arange(600) % 257)


@pytest.mark.parametrize("nv", [1, 8])
@pytest.mark.parametrize("k", [1, 7, 64])
def test_random_libraries(nv, k):
    rows, rng = nm.random_library(300, nv, 100 + nv + k)
    hq = rng.integers(0, 256, (11, 32), dtype=np.uint8)
    hf = None if nv == 1 else (rng.random(300) < 0.6).astype(np.uint8)
    nm.same(host(rows, hq, k, has_features=hf), nm.nearest(rows, hq, k, has_features=hf))


def test_ties_go_to_the_smaller_file_number():
    base = nm.base_hash()
    for lib in (nm.ladder(800, base), nm.ladder_descending(800, base), nm.ladder_shuffled(800, 3, base), nm.identical(200)):
        q = np.stack([base, lib[5]])
        got = host(lib, q, 10)
        nm.same(got, nm.nearest(lib, q, 10))
    e, c = host(nm.identical(200), nm.base_hash(11)[None], 10)
    assert e["i"][0].tolist() == list(range(10)) and (e["d"] == 0).all() and c[0] == 10
    # the ladder holds distance j at files j, j + 257, j + 514: three files per distance, the smaller number first
    e, _ = host(nm.ladder(600, base), base[None], 7)
    assert e["i"][0].tolist() == [0, 257, 514, 1, 258, 515, 2] and e["d"][0].tolist() == [0, 0, 0, 1, 1, 1, 2]


def test_smallest_attaining_variant_is_reported():
    rng = np.random.default_rng(5)
    q = nm.base_hash(21)
    rows = nm.with_variants(rng.integers(0, 256, (6, 32), dtype=np.uint8), rng)
    near = nm.at_distance(q, 9, rng)
    rows[2, 3] = rows[2, 6] = near          # two rows attain the minimum: variant 3
    rows[4, 7] = nm.at_distance(q, 4, rng)  # only the last row
    rows[5, 0] = rows[5, 1] = q             # row 0 wins a tie with row 1
    e, c = host(rows, q[None], 3)
    assert e["i"][0].tolist() == [5, 4, 2] and e["d"][0].tolist() == [0, 4, 9]
    assert (e["flags"][0] >> nm.VARIANT_SHIFT).tolist() == [0, 7, 3] and c[0] == 3
    nm.same((e, c), nm.nearest(rows, q[None], 3))


def test_decoy_rows_of_files_without_features_are_ignored():
    rng = np.random.default_rng(6)
    q = nm.base_hash(22)
    hashes = np.stack([nm.at_distance(q, 100 + i, rng) for i in range(12)])
    rows, hf = nm.decoys(hashes, q, rng)
    e, c = host(rows, q[None], 12, has_features=hf)
    assert e["d"][0].tolist() == [100 + i for i in range(12)] and (e["flags"] == 0).all()
    hf[7] = 1  # ... and a file that has features does own them
    e, c = host(rows, q[None], 12, has_features=hf)
    assert e["i"][0, 0] == 7 and e["d"][0, 0] <= 3
    nm.same((e, c), nm.nearest(rows, q[None], 12, has_features=hf))
    # without the flags every file owns all its rows
    nm.same(host(rows, q[None], 12), nm.nearest(rows, q[None], 12))
    assert host(rows, q[None], 12)[0]["d"].max() <= 3


def test_skip_and_the_twin_of_a_skipped_file():
    rng = np.random.default_rng(7)
    lib = rng.integers(0, 256, (50, 32), dtype=np.uint8)
    lib[31] = lib[17]  # a bit-identical twin
    q = lib[[17, 3, 31]]
    skip = [17, None, nm.NO_FILE]
    got = host(lib, q, 5, skip=skip)
    nm.same(got, nm.nearest(lib, q, 5, skip=skip))
    e, _ = got
    assert (e["i"][0, 0], e["d"][0, 0]) == (31, 0) and 17 not in e["i"][0]
    assert e["i"][1, 0] == 3 and e["i"][2, :2].tolist() == [17, 31]


def test_k_above_the_eligible_files_pads():
    rng = np.random.default_rng(8)
    lib = rng.integers(0, 256, (5, 32), dtype=np.uint8)
    q = rng.integers(0, 256, (3, 32), dtype=np.uint8)
    e, c = host(lib, q, 64, skip=[None, 2, None])
    nm.same((e, c), nm.nearest(lib, q, 64, skip=[None, 2, None]))
    assert c.tolist() == [5, 4, 5]
    pad = e[1, 4:]
    assert (pad["i"] == nm.NO_FILE).all() and (pad["j"] == 1).all() and (pad["d"] == 0xFFFF).all() and (pad["flags"] == 0).all()


@pytest.mark.parametrize("max_dist", [0, 31, 255, 256, 1000])
def test_cutoffs(max_dist):
    base = nm.base_hash()
    lib = np.concatenate([nm.ladder_shuffled(300, 4, base), nm.complement(base)[None], base[None]])
    q = np.stack([base, nm.complement(base)])
    got = host(lib, q, 64, max_dist=max_dist)
    nm.same(got, nm.nearest(lib, q, 64, max_dist=max_dist))
    assert got[0]["d"][0, :got[1][0]].max() <= min(max_dist, 256)
    if max_dist == 0:  # the base query: ladder steps 0 and 257 and the base itself; its complement: ladder step 256 and the complement
        assert got[1].tolist() == [3, 2]
    if max_dist == 255:
        assert 256 not in got[0]["d"][1, :got[1][1]]


def test_empty_library_and_no_queries():
    q = np.random.default_rng(9).integers(0, 256, (4, 32), dtype=np.uint8)
    for nv in (1, 8):
        e, c = host(np.zeros((0, nv, 32), np.uint8), q, 3)
        nm.same((e, c), nm.nearest(np.zeros((0, nv, 32), np.uint8), q, 3))
        assert (e["i"] == nm.NO_FILE).all() and (c == 0).all() and e["j"][:, 0].tolist() == [0, 1, 2, 3]
    e, c = host(q, np.zeros((0, 32), np.uint8), 3)
    assert e.shape == (0, 3) and c.shape == (0,)
    # n_q == 0 is RPH_OK even with null pointers all round
    assert _lib.load().rph_hamming_nearest_host(None, 1, None, 0, None, None, 0, 1, 256, None, None) == _lib.RPH_OK


def test_refused_calls_write_nothing():
    L = _lib.load()
    rng = np.random.default_rng(10)
    rows = rng.integers(0, 256, (6, 8, 32), dtype=np.uint8)
    hq = rng.integers(0, 256, (2, 32), dtype=np.uint8)

    def call(rows_p=ptr(rows), nv=8, n_lib=6, hq_p=ptr(hq), n_q=2, k=3, out_null=False):
        edges = np.frombuffer(bytes([0xA5]) * (2 * 64 * EDGE_DTYPE.itemsize), np.uint8).copy()
        counts = np.full(2, 0xA5A5A5A5, np.uint32)
        before = edges.tobytes(), counts.tobytes()
        rc = L.rph_hamming_nearest_host(rows_p, nv, None, n_lib, hq_p, None, n_q, k, 256, None if out_null else ptr(edges), ptr(counts))
        assert (edges.tobytes(), counts.tobytes()) == before
        return rc

    for bad in (dict(k=0), dict(k=65), dict(k=0xFFFFFFFF), dict(nv=0), dict(nv=2), dict(nv=7), dict(nv=9), dict(n_lib=0xFFFFFFFF), dict(n_lib=1 << 40),
                dict(rows_p=None), dict(hq_p=None), dict(out_null=True)):
        assert call(**bad) == _lib.RPH_ERR_INVALID_ARG, bad
    assert b"rph_hamming_nearest_host" in L.rph_last_error()


def test_wrapper_shapes_and_dtypes():
    rng = np.random.default_rng(11)
    lib = rng.integers(0, 256, (20, 32), dtype=np.uint8)
    e, c = host(lib, lib[:3], 4)
    assert e.shape == (3, 4) and e.dtype == EDGE_DTYPE and c.shape == (3,) and c.dtype == np.uint32
    assert np.array_equal(e["j"], np.arange(3, dtype=np.uint32)[:, None].repeat(4, axis=1))
    e8, _ = host(lib.reshape(20, 1, 32).repeat(8, axis=1), lib[:3], 4)
    assert np.array_equal(e8["i"], e["i"]) and (e8["flags"] == 0).all()
    one, _ = host(lib, lib[5], 1)  # a single hash is one query
    assert one.shape == (1, 1) and one["i"][0, 0] == 5
    with pytest.raises(ValueError):
        host(lib.reshape(20, 2, 16), lib[:3], 4)
    with pytest.raises(ValueError):
        host(lib, lib[:3], 4, skip=[1])
    with pytest.raises(ValueError):
        host(lib, lib[:3], 4, has_features=[1])
    from rupphash_amd import RphError
    with pytest.raises(RphError):
        host(lib, lib[:3], 65)
    assert Engine.nearest_layout(1000, 8, 5, 10)[0] == 4 and Engine.nearest_layout(1000, 1, 5, 10)[0] == 32


# ---- the two faster models against the plain one ----
@pytest.mark.parametrize("nv", [1, 8])
def test_popcount_distances_equal_the_unpackbits_ones(nv, monkeypatch):
    rows, rng = nm.random_library(37, nv, 200 + nv)
    rows[3, nv - 1] = nm.complement(rows[0, 0])
    hq = np.concatenate([rng.integers(0, 256, (13, 32), dtype=np.uint8), rows[0, 0][None]])
    want = nm.distances(rows, hq)
    assert want[0, 0, 13] == 0 and want[3, nv - 1, 13] == 256
    got = nm.distances_popcount(rows, hq)
    assert got.dtype == want.dtype and np.array_equal(got, want)
    monkeypatch.setattr(nm, "POPCOUNT_TEMP_WORDS", 4 * 37 * nv * 3)  # three queries at a time: 14 is four full steps and a ragged one
    assert np.array_equal(nm.distances_popcount(rows, hq), want)
    monkeypatch.setattr(nm, "POPCOUNT_TEMP_WORDS", 4 * 5)            # five rows of one query at a time, as against a large library
    assert np.array_equal(nm.distances_popcount(rows, hq), want)
    x = rng.integers(0, 1 << 63, (5, 4), dtype=np.uint64) | np.uint64(1 << 63)
    assert nm._BYTE_ONES[x.view(np.uint8).reshape(5, 4, 8)].sum(axis=-1).tolist() == [[bin(v).count("1") for v in row] for row in x.tolist()]
    monkeypatch.delattr(np, "bitwise_count", raising=False)  # the byte table, for a numpy without it
    assert np.array_equal(nm.distances_popcount(rows, hq), want)


@pytest.mark.parametrize("nv", [1, 8])
@pytest.mark.parametrize("k", [1, 7, 64])
def test_vectorised_model_equals_the_loop(nv, k):
    rows, rng = nm.random_library(50, nv, 300 + nv + k)
    rows[31, 0] = rows[17, 0]  # a twin: ties by file number
    hq = np.concatenate([rng.integers(0, 256, (9, 32), dtype=np.uint8), rows[[17, 31, 4], 0]])
    hf = None if nv == 1 else (rng.random(50) < 0.6).astype(np.uint8)
    skip = [None, 3, nm.NO_FILE, 49, 0, None, None, None, None, 17, None, 4]
    for kw in (dict(), dict(has_features=hf), dict(skip=skip), dict(has_features=hf, skip=skip, max_dist=120), dict(max_dist=0), dict(max_dist=1000)):
        for dist in (nm.distances, nm.distances_popcount):
            nm.same(nm.nearest_vectorised(rows, hq, k, distances=dist, **kw), nm.nearest(rows, hq, k, **kw))
        nm.same(nm.nearest(rows, hq, k, distances=nm.distances_popcount, **kw), nm.nearest(rows, hq, k, **kw))
    few = rows[:5]  # k above the library, and above what skip and the cutoff leave
    nm.same(nm.nearest_vectorised(few, hq, k, has_features=None if hf is None else hf[:5], skip=[2] * 12), nm.nearest(few, hq, k, has_features=None if hf is None else hf[:5], skip=[2] * 12))
    nm.same(nm.nearest_vectorised(few, hq, k, max_dist=110), nm.nearest(few, hq, k, max_dist=110))
    nm.same(nm.nearest_vectorised(few[:0], hq, k), nm.nearest(few[:0], hq, k))
    nm.same(nm.nearest_vectorised(few, hq[:0], k), nm.nearest(few, hq[:0], k))


# ---- how a call is cut, under the two knobs ----
MIB = 1 << 20
DEFAULT_WORKSPACE = 256 * MIB
MAX_SEG = 1 << 20


@pytest.fixture
def knobs(request):
    """sets the workspace limit and the forced segment; both are back at their defaults when the test is through"""
    def restore():
        Engine.nearest_set_workspace(0)
        Engine.nearest_set_segment(0)

    def set_(workspace=0, segment=0):
        Engine.nearest_set_workspace(workspace)
        Engine.nearest_set_segment(segment)

    request.addfinalizer(restore)
    return set_


def test_default_layout_is_the_parents():
    # with both knobs at 0: the tuples of the commit before the workspace knob, for the arguments of test_layout_keeps_its_bounds
    want = {(1, 8, 1, 1): (4, 64, 32, 1), (10**6, 8, 1, 10): (4, 492, 32, 2033), (10**6, 8, 10**4, 64): (4, 142860, 32, 7),
            (2**32 - 2, 1, 1, 64): (32, 1 << 20, 32, 4096), (2**32 - 2, 8, 10**6, 64): (4, 1 << 20, 32, 4096), (10**7, 1, 32, 1): (32, 4896, 32, 2043)}
    for args, layout in want.items():
        assert Engine.nearest_layout(*args) == layout, args
    # ... and the chunk: what 256 MiB holds of that many segments' lists, in whole tiles, 2^20 queries at most
    assert [Engine.nearest_chunk_queries(*a) for a in want] == [1 << 20, 3296, 149792, 256, 256, 32832]


def test_layout_keeps_its_bounds_under_the_knobs(knobs):
    whole = lambda files, fb: -(-files // fb) * fb  # noqa: E731  (in whole MFMA blocks)
    seen = 0
    for workspace in (0, 8192, 64 << 10, MIB):
        limit = workspace or DEFAULT_WORKSPACE
        for forced in (0, 8, 40, MAX_SEG, MAX_SEG + 4):
            knobs(workspace, forced)
            for k in (1, 7, 32, 33, 64):
                most_segs = limit // (32 * k * 4)
                for n_lib in (0, 1, 300, 1000, 10**6, 2**32 - 2):
                    if n_lib > most_segs * MAX_SEG:
                        continue  # more files than the key's 20 bits and this workspace can hold between them
                    for nv in (1, 8):
                        for n_q in (1, 31, 33, 70, 10**4, 2**20 + 33):
                            fb, seg, qt, n_segs = Engine.nearest_layout(n_lib, nv, n_q, k)
                            chunk = Engine.nearest_chunk_queries(n_lib, nv, n_q, k)
                            where = (workspace, forced, k, n_lib, nv, n_q, seg, n_segs, chunk)
                            assert fb == (4 if nv == 8 else 32) and qt == 32, where
                            assert seg % fb == 0 and 0 < seg <= MAX_SEG and n_segs == -(-n_lib // seg), where
                            assert chunk % 32 == 0 and 32 <= chunk <= 1 << 20, where
                            assert n_segs * min(chunk, max(n_q, 32)) * k * 4 <= limit, where
                            if forced and n_segs:  # the forced length holds unless the workspace or the key asks for another
                                assert seg == min(max(whole(forced, fb), whole(-(-n_lib // most_segs), fb)), MAX_SEG), where
                            seen += 1
    assert seen == 7200 - 14 * 5 * 12  # 2^32 - 2 files need 4096 segments: of the small workspaces only 1 MiB at k = 1 holds them


def test_workspace_knob_floor_and_reset(knobs):
    args = (1000, 1, 70, 64)
    default = Engine.nearest_layout(*args), Engine.nearest_chunk_queries(*args)
    floor = (32, 1024, 32, 1), 32  # 8192 bytes: one segment of 64-key lists for one tile
    for workspace in (1, 100, 8191, 8192):
        knobs(workspace)
        assert (Engine.nearest_layout(*args), Engine.nearest_chunk_queries(*args)) == floor, workspace
    knobs(8192 + 8192)
    assert (Engine.nearest_layout(*args), Engine.nearest_chunk_queries(*args)) == ((32, 512, 32, 2), 32)
    knobs(0)
    assert (Engine.nearest_layout(*args), Engine.nearest_chunk_queries(*args)) == default == ((32, 512, 32, 2), (256 * MIB) // (2 * 64 * 4))


def test_shapes_the_gpu_tests_rely_on(knobs):
    """What test_nearest_grid_gpu.py takes for granted, worked out from nearest_layout() by hand: it asserts the same on the device, but a
    premise that drifts fails here first."""
    knobs(64 << 10, 8)
    # 65536 / (32 x 7 x 4) = 73 segments at most, so 8-file segments stay: 38 of them; 65536 / (38 x 7 x 4) = 61 queries, whole tiles: 32
    assert Engine.nearest_layout(300, 8, 69, 7) == (4, 8, 32, 38) and Engine.nearest_chunk_queries(300, 8, 69, 7) == 32
    for nv, fb in ((1, 32), (8, 4)):
        # 65536 / (32 x 64 x 4) = 8 segments at most: 125 files each, in whole blocks 128; 8 segments x 32 queries x 64 x 4 = 65536 exactly
        for n_q in (31, 32, 33, 69):
            assert Engine.nearest_layout(1000, nv, n_q, 64) == (fb, 128, 32, 8) and Engine.nearest_chunk_queries(1000, nv, n_q, 64) == 32
        assert 8 * 32 * 64 * 4 == 64 << 10
    knobs(MIB, 8)
    # 128 segments at most: 17 files each, in whole blocks 20 (105 segments) or 32 (66); 1 MiB / (105 x 256) = 39, / (66 x 256) = 62: one tile
    assert Engine.nearest_layout(2100, 8, 69, 64) == (4, 20, 32, 105) and Engine.nearest_chunk_queries(2100, 8, 69, 64) == 32
    assert Engine.nearest_layout(2100, 1, 69, 64) == (32, 32, 32, 66) and Engine.nearest_chunk_queries(2100, 1, 69, 64) == 32
    knobs(0, MAX_SEG + 4)
    for n_lib, nv, n_q, k in ((2 * MAX_SEG + 40, 1, 3, 7), (MAX_SEG + 6, 8, 3, 7), (5, 8, 1, 1), (2**32 - 2, 1, 10**4, 64)):
        assert Engine.nearest_layout(n_lib, nv, n_q, k)[1:] == (MAX_SEG, 32, -(-n_lib // MAX_SEG)), (n_lib, nv)
    knobs(0, MAX_SEG)
    assert Engine.nearest_layout(2 * MAX_SEG + 40, 1, 3, 7) == (32, MAX_SEG, 32, 3) and Engine.nearest_layout(MAX_SEG + 6, 8, 3, 7) == (4, MAX_SEG, 32, 2)
    knobs(0, 0)
    # the chunk limit that needs no knob: five files are one segment, whose lists of 2 would let 2^25 queries in; MAX_CHUNK_QUERIES cuts first
    assert Engine.nearest_layout(5, 8, 2**20 + 33, 2) == (4, 64, 32, 1) and Engine.nearest_chunk_queries(5, 8, 2**20 + 33, 2) == 1 << 20
    knobs(0, 8)
    assert Engine.nearest_layout(73, 8, 10**4, 2) == (4, 8, 32, 10) and Engine.nearest_layout(9 * 32 + 1, 1, 10**4, 2) == (32, 32, 32, 10)
