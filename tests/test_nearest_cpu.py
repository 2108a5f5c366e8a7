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
