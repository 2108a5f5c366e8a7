"""The resident library on the GPU (-m gpu): after every append its groups, labels and comparison count are those of
rph_group_files_pdq on the files appended so far, whatever the batches were; restore + append equals the one-shot call; a query reports
the pairs a numpy brute force finds and changes nothing."""
import ctypes as C

import numpy as np
import pytest

import library_corpus as lc

pytestmark = pytest.mark.gpu

SIMS = (0, 16, 40, 63)
MODES = ("coefficients-everywhere", "no-coefficients", "alternating")


@pytest.fixture(scope="module")
def eng():
    from rupphash_amd import Engine

    e = Engine(0)
    yield e
    e.set_hamming_kernel(2)
    e.close()


@pytest.fixture(scope="module")
def files():
    return lc.corpus()


def with_coefficients(split, mode):
    """per batch: does it come with coefficients (alternating: every second batch that has files)"""
    out, k = [], 0
    for m in split:
        out.append(mode == MODES[0] or (mode == MODES[2] and k % 2 == 0))
        k += m > 0
    return out


def effective_features(f, split, mode):
    """has_features of the concatenation: 0 for the files of batches that came without coefficients"""
    hf = f.has_features.copy()
    for (first, last), has in zip(lc.batches(split), with_coefficients(split, mode)):
        if not has:
            hf[first:last] = 0
    return hf


def batch(f, first, last, has):
    kw = dict(quality=f.quality[first:last])
    if has:
        kw.update(coeffs=f.coeffs[first:last], has_features=f.has_features[first:last])
    return kw


_expected = {}


def expected(eng, f, sim, stop, hf):
    """(groups, comparisons) of rph_group_files_pdq on the first `stop` files; computed once per distinct request"""
    key = (sim, stop, hf[:stop].tobytes())
    if key not in _expected:
        if hf[:stop].any():
            _expected[key] = eng.group_files_pdq(f.hashes[:stop], sim, f.coeffs[:stop], hf[:stop], f.quality[:stop])
        else:
            _expected[key] = eng.group_files_pdq(f.hashes[:stop], sim, quality=f.quality[:stop])
    return _expected[key]


_oracle = {}


def oracle_groups(oracle, f, sim, hf):
    key = (sim, hf.tobytes())
    if key not in _oracle:
        edges, groups = oracle.group_pdq(f.hashes, sim, variants=f.dih if hf.any() else None, has_features=hf if hf.any() else None, quality=f.quality)
        _oracle[key] = (groups, len(edges))
    return _oracle[key]


def first_members(groups, first, last):
    want = np.arange(first, last, dtype=np.uint32)
    for g in groups:
        for m in g:
            if first <= m < last:
                want[m - first] = g[0]
    return want


def run_split(eng, oracle, f, split, sim, mode):
    hf = effective_features(f, split, mode)
    joined = False
    with eng.library(sim) as lib:
        assert len(lib) == 0 and lib.comparisons == 0 and lib.groups() == []
        for (first, last), has in zip(lc.batches(split), with_coefficients(split, mode)):
            before = lib.comparisons
            labels, new_cmp = lib.append(f.hashes[first:last], **batch(f, first, last, has))
            want_groups, want_cmp = expected(eng, f, sim, last, hf)
            assert len(lib) == last
            assert lib.groups() == want_groups, (split, sim, mode, last)
            assert before + new_cmp == lib.comparisons == want_cmp, (split, sim, mode, last)
            assert np.array_equal(labels, first_members(want_groups, first, last)), (split, sim, mode, last)
            assert np.array_equal(lib.labels(), first_members(want_groups, 0, last))
            joined |= 0 < first < last and any(g[0] < first <= g[-1] for g in want_groups)
        ref_groups, ref_cmp = oracle_groups(oracle, f, sim, hf)
        assert lib.groups() == ref_groups and lib.comparisons == ref_cmp
    return joined


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sim", SIMS)
@pytest.mark.parametrize("split", lc.SPLITS, ids=lambda s: "-".join(map(str, s)) if len(s) < 6 else "19x100-1")
def test_every_append_equals_regrouping_the_prefix(eng, oracle, files, split, sim, mode):
    joined = run_split(eng, oracle, files, split, sim, mode)
    if len(split) > 1 and sim >= 40:
        assert joined  # some append did join new files to old groups


@pytest.mark.parametrize("kernel", [0, 1, 2, 3, 4])
def test_one_split_under_every_hamming_kernel(eng, oracle, files, kernel):
    eng.set_hamming_kernel(2)
    hf = effective_features(files, [1023, 1, 1, 876], MODES[0])
    for stop in (1023, 1024, 1025, 1901):
        expected(eng, files, 40, stop, hf)  # the expectations under the default kernel
    try:
        eng.set_hamming_kernel(kernel)
        assert run_split(eng, oracle, files, [1023, 1, 1, 876], 40, MODES[0])
    finally:
        eng.set_hamming_kernel(2)


def test_the_bridge_file_merges_two_resident_groups(eng, files):
    b = lc.BRIDGE
    last = lc.N_FILES - 1
    with eng.library(40) as lib:
        lib.append(files.hashes[:last], files.coeffs[:last], files.has_features[:last], files.quality[:last])
        assert list(lib.labels(b["a"], 2)) == [b["a"]] * 2 and list(lib.labels(b["b"], 2)) == [b["b"]] * 2
        n_before = len(lib.groups())
        labels, _ = lib.append(files.hashes[last:], files.coeffs[last:], files.has_features[last:], files.quality[last:])
        assert list(labels) == [b["a"]]
        # the OLD labels of B's group were flattened again
        assert list(lib.labels(b["b"], 2)) == [b["a"]] * 2 and len(lib.groups()) == n_before - 1


# ---------------------------------------------------------------- dense libraries: the edge buffer's retry loop
# identical files resident, identical files appended, eight rows per file (coefficients all +0.0: eight all-zero variants)
DENSE = {"within-overflows": (0, 1500, False), "cross-overflows": (1100, 1000, False), "sum-overflows": (700, 1000, False),
         "eight-rows-per-file": (300, 400, True)}
DENSE_SIM = 31


def dense_premise(name, cross, inner, cap):
    """the inequality of the case: which sweep runs the edge buffer over"""
    if name == "within-overflows":
        return cross == 0 and inner > cap
    if name == "cross-overflows":
        return cross > cap
    return cross <= cap < cross + inner


def same_state(lib, labels, groups, comparisons):
    assert lib.groups() == groups
    assert np.array_equal(lib.labels(), labels)
    assert lib.comparisons == comparisons


def run_dense(eng, oracle, name):
    from rupphash_amd import EDGE_DTYPE, RphError, _lib

    resident, appended, eight = DENSE[name]
    rows = 8 if eight else 1
    hashes, common = lc.dense_hashes(resident + appended, common=np.zeros(32, np.uint8) if eight else None)
    n = len(hashes)
    cut = int(np.nonzero(common)[0][resident]) if resident else 0
    assert common[:cut].sum() == resident and common[cut:].sum() == appended
    hf = common.astype(np.uint8) if eight else np.zeros(n, np.uint8)  # the unrelated files keep to their hash
    coeffs = np.zeros((n, 256), np.float32)
    variants = np.repeat(hashes[:, None, :], 8, axis=1)  # what zero coefficients hash to is the all-zero hash, eight times
    files = lambda a, b: dict(coeffs=coeffs[a:b], has_features=hf[a:b]) if eight else {}  # noqa: E731

    def by_oracle(stop, features):
        if stop == 0:
            return [], 0
        edges, groups = oracle.group_pdq(hashes[:stop], DENSE_SIM, variants=variants[:stop] if eight else None, has_features=features[:stop] if eight else None)
        return groups, len(edges)

    # the premise, on numbers that do not come from the library
    cross, inner = rows * resident * appended, rows * appended * (appended - 1) // 2
    assert by_oracle(n, hf)[1] - by_oracle(cut, hf)[1] == cross + inner
    assert dense_premise(name, cross, inner, lc.library_first_cap(n - cut)), (name, cross, inner, lc.library_first_cap(n - cut))
    want_labels, want_groups, want_cmp = lc.dense_expectation(common, rows)
    assert (want_groups, want_cmp) == by_oracle(n, hf)
    old_groups, old_cmp = lc.dense_expectation(common[:cut], rows)[1:]

    with eng.library(DENSE_SIM) as lib:
        if cut:
            assert lib.append(hashes[:cut], **files(0, cut))[1] == old_cmp
            same_state(lib, lc.dense_expectation(common[:cut], rows)[0], old_groups, old_cmp)
        labels, new_cmp = lib.append(hashes[cut:], **files(cut, n))
        assert new_cmp == cross + inner and np.array_equal(labels, want_labels[cut:])
        same_state(lib, want_labels, want_groups, want_cmp)
        kw = dict(old_coeffs=coeffs[:cut], old_has_features=hf[:cut], new_coeffs=coeffs[cut:], new_has_features=hf[cut:]) if eight else {}
        if cut:
            assert eng.group_files_pdq_append(hashes[:cut], old_groups, hashes[cut:], DENSE_SIM, **kw) == (want_groups, cross + inner)
        else:  # nothing resident: the split is the one-shot call
            assert eng.group_files_pdq(hashes, DENSE_SIM) == (want_groups, cross + inner)

        # the state after a retry is healthy: ten more files (without coefficients), a query that fits and one that does not
        more = np.concatenate([np.repeat(hashes[:1], 5, axis=0), np.random.default_rng(7).integers(0, 256, (5, 32), dtype=np.uint8)])
        all_hashes, all_common = np.concatenate([hashes, more]), np.concatenate([common, [True] * 5 + [False] * 5])
        all_hf = np.concatenate([hf, np.zeros(10, np.uint8)])
        variants = np.concatenate([variants, np.repeat(more[:, None, :], 8, axis=1)])
        hashes = all_hashes
        ref_groups, ref_cmp = by_oracle(n + 10, all_hf)
        state = (lc.dense_expectation(all_common)[0], ref_groups, ref_cmp)
        assert ref_groups == lc.dense_expectation(all_common)[1] and ref_cmp == want_cmp + rows * (resident + appended) * 5 + 10
        labels, new_cmp = lib.append(more)
        assert new_cmp == ref_cmp - want_cmp and np.array_equal(labels, state[0][n:])
        same_state(lib, *state)
        total = rows * (resident + appended) + 5
        got = lib.query(hashes[:1], cap=total)
        assert len(got) == total and (got["d"] == 0).all() and sorted(set(got["i"].tolist())) == np.nonzero(all_common)[0].tolist()
        same_state(lib, *state)
        edges, found = np.zeros(10, EDGE_DTYPE), C.c_uint64()
        rc = eng.L.rph_library_query(lib.handle, hashes[:1].ctypes.data_as(C.c_void_p), None, 1, edges.ctypes.data_as(C.c_void_p), 10, C.byref(found))
        assert rc == _lib.RPH_ERR_CAPACITY and found.value == total
        with pytest.raises(RphError) as err:
            lib.query(hashes[:1], cap=10)
        assert err.value.status == _lib.RPH_ERR_CAPACITY
        same_state(lib, *state)


@pytest.mark.parametrize("name", list(DENSE))
def test_dense_append_overflows_the_edge_buffer_and_still_equals_the_oracle(eng, oracle, name):
    run_dense(eng, oracle, name)


@pytest.mark.parametrize("kernel", [0, 1])  # (2 is the default: the test above)
def test_the_sum_overflow_under_the_other_hamming_kernels(eng, oracle, kernel):
    try:
        eng.set_hamming_kernel(kernel)
        run_dense(eng, oracle, "sum-overflows")
    finally:
        eng.set_hamming_kernel(2)


def test_reserve_with_files_resident(eng, files):
    f = files
    want_groups, want_cmp = expected(eng, f, 40, lc.N_FILES, f.has_features)
    with eng.library(40) as lib:
        lib.append(f.hashes[:300], f.coeffs[:300], f.has_features[:300], f.quality[:300])
        state = (lib.groups(), lib.labels().tolist(), lib.comparisons)
        assert state[0] == expected(eng, f, 40, 300, f.has_features)[0]
        lib.reserve(3000)  # the resident files move to the new buffers
        assert (lib.groups(), lib.labels().tolist(), lib.comparisons) == state and len(lib) == 300
        lib.reserve(100)  # below the current size: nothing changes
        assert (lib.groups(), lib.labels().tolist(), lib.comparisons) == state and len(lib) == 300
        labels, _ = lib.append(f.hashes[300:], f.coeffs[300:], f.has_features[300:], f.quality[300:])
        assert lib.groups() == want_groups and lib.comparisons == want_cmp
        assert np.array_equal(labels, first_members(want_groups, 300, lc.N_FILES))
        assert np.array_equal(lib.labels(), first_members(want_groups, 0, lc.N_FILES))
        lib.reserve(0)
        assert lib.groups() == want_groups and lib.comparisons == want_cmp


# ---------------------------------------------------------------- restore
@pytest.mark.parametrize("sim", (16, 40))
@pytest.mark.parametrize("n_old", (0, 1, 1500, 1901))
def test_restore_then_append_equals_one_shot(eng, files, sim, n_old):
    f = files
    old_groups, old_cmp = eng.group_files_pdq(f.hashes[:n_old], sim, f.coeffs[:n_old], f.has_features[:n_old], f.quality[:n_old])
    want_groups, want_cmp = expected(eng, f, sim, lc.N_FILES, f.has_features)
    with eng.library(sim) as lib:
        lib.restore(f.hashes[:n_old], old_groups, old_cmp, f.coeffs[:n_old], f.has_features[:n_old], f.quality[:n_old])
        assert len(lib) == n_old and lib.comparisons == old_cmp and lib.groups() == old_groups
        labels, new_cmp = lib.append(f.hashes[n_old:], f.coeffs[n_old:], f.has_features[n_old:], f.quality[n_old:])
        assert lib.groups() == want_groups and old_cmp + new_cmp == want_cmp
        assert np.array_equal(labels, first_members(want_groups, n_old, lc.N_FILES))


def test_restore_refuses_malformed_groups_and_a_library_with_files(eng, files):
    from rupphash_amd import RphError, _lib

    h = files.hashes[:100]
    u32 = lambda *x: np.array(x, np.uint32)  # noqa: E731
    bad = {
        "a member outside n": (u32(3, 100), u32(0, 2)),
        "a member twice": (u32(3, 4, 7, 3), u32(0, 2, 4)),
        "offsets not ascending": (u32(3, 4, 7, 8), u32(0, 3, 2)),
        "offsets do not start at 0": (u32(3, 4, 7, 8), u32(1, 4)),
    }
    with eng.library(40) as lib:
        for name, groups in bad.items():
            with pytest.raises(RphError) as err:
                lib.restore(h, groups)
            assert err.value.status == _lib.RPH_ERR_INVALID_ARG, name
            assert len(lib) == 0 and lib.comparisons == 0 and lib.groups() == [], name
        lib.restore(h, [[3, 4], [7, 8, 50]], 5)
        assert len(lib) == 100 and lib.comparisons == 5 and lib.groups() == [[3, 4], [7, 8, 50]]
        with pytest.raises(RphError) as err:
            lib.restore(h, [[3, 4]])
        assert err.value.status == _lib.RPH_ERR_INVALID_ARG
        assert len(lib) == 100 and lib.groups() == [[3, 4], [7, 8, 50]]


# ---------------------------------------------------------------- query
def test_query_matches_numpy_and_changes_nothing(eng, files):
    from rupphash_amd import EDGE_DTYPE, _lib

    f = files
    n, n_q = 1500, 300
    rng = np.random.default_rng(808)
    hf = effective_features(f, [700, 800, 401], MODES[2])[:n]  # files 700 .. 1499 come without coefficients: they keep to variant 0
    # queries: resident hashes, hashes of files that are not resident (their families are), the mirrored copies of files 10 and 20 (which
    # only a variant of those matches), random ones
    q_hashes = np.concatenate([f.hashes[rng.integers(0, n, 100)], f.hashes[n:n + 150], f.hashes[[1400, 1700]], rng.integers(0, 256, (48, 32), dtype=np.uint8)])
    q_quality = rng.integers(30, 101, n_q).astype(np.int32)
    q_quality[::5] = -1
    rows = np.where(hf[:, None, None] != 0, f.dih[:n], f.hashes[:n, None, :])
    ba = np.unpackbits(rows.reshape(-1, 32), axis=1).astype(np.float32)
    bb = np.unpackbits(q_hashes, axis=1).astype(np.float32)
    dist = (ba.sum(1)[:, None] + bb.sum(1)[None, :] - 2.0 * (ba @ bb.T)).astype(np.int64).reshape(n, 8, n_q)  # exact: integers <= 256
    owned = (hf[:, None] != 0) | (np.arange(8)[None, :] == 0)
    low_a = ((f.quality[:n] >= 0) & (f.quality[:n] < 50)).astype(np.uint8)
    with eng.library(40) as lib40, eng.library(0) as lib0, eng.library(63) as lib63:
        for lib in (lib40, lib0, lib63):
            lib.append(f.hashes[:700], f.coeffs[:700], f.has_features[:700], f.quality[:700])
            lib.append(f.hashes[700:n], quality=f.quality[700:n])
            state = (len(lib), lib.comparisons, lib.groups(), lib.labels().tolist())
            for quality, low_b in ((q_quality, ((q_quality >= 0) & (q_quality < 50)).astype(np.uint8)), (None, np.zeros(n_q, np.uint8))):
                limit = np.where((low_a[:, None] | low_b[None, :]) != 0, 0, lib.similarity)
                i, v, j = np.nonzero((dist <= limit[:, None, :]) & owned[:, :, None])
                want = sorted(zip(i.tolist(), j.tolist(), v.tolist(), dist[i, v, j].tolist()))
                got = lib.query(q_hashes, quality)
                have = sorted(zip(got["i"].tolist(), got["j"].tolist(), ((got["flags"] >> 9) & 7).tolist(), got["d"].tolist()))
                assert have == want, (lib.similarity, quality is None)
                if lib.similarity >= 40:
                    assert any(x[2] != 0 for x in want) and len(want) > 100
            assert (len(lib), lib.comparisons, lib.groups(), lib.labels().tolist()) == state
        # capacity protocol: the total is reported when it does not fit
        total = len(lib40.query(q_hashes))
        edges = np.zeros(10, EDGE_DTYPE)
        found = C.c_uint64()
        rc = eng.L.rph_library_query(lib40.handle, q_hashes.ctypes.data_as(C.c_void_p), None, n_q, edges.ctypes.data_as(C.c_void_p), 10, C.byref(found))
        assert rc == _lib.RPH_ERR_CAPACITY and found.value == total > 10
        assert (edges["i"] < n).all() and (edges["j"] < n_q).all() and (edges["d"] <= 40).all()
        from rupphash_amd import RphError

        with pytest.raises(RphError) as err:
            lib40.query(q_hashes, cap=10)
        assert err.value.status == _lib.RPH_ERR_CAPACITY
        assert len(lib40.query(np.zeros((0, 32), np.uint8))) == 0
    with eng.library(40) as empty:
        assert len(empty.query(q_hashes)) == 0


# ---------------------------------------------------------------- handles and arguments
def test_two_libraries_do_not_see_each_other(eng, files):
    f = files
    with eng.library(40) as one, eng.library(16) as two:
        one.append(f.hashes[:500], f.coeffs[:500], f.has_features[:500], f.quality[:500])
        two.append(f.hashes[500:900], f.coeffs[500:900], f.has_features[500:900], f.quality[500:900])
        one.append(f.hashes[500:600], f.coeffs[500:600], f.has_features[500:600], f.quality[500:600])
        assert (len(one), len(two)) == (600, 400)
        assert (one.groups(), one.comparisons) == expected(eng, f, 40, 600, f.has_features)
        assert (two.groups(), two.comparisons) == eng.group_files_pdq(f.hashes[500:900], 16, f.coeffs[500:900], f.has_features[500:900], f.quality[500:900])


def test_arguments(eng, files):
    from rupphash_amd import RphError, _lib

    f = files
    with pytest.raises(RphError) as err:
        eng.library(64)
    assert err.value.status == _lib.RPH_ERR_INVALID_ARG
    L = eng.L
    h = C.c_void_p()
    assert L.rph_library_create(None, 40, C.byref(h)) == _lib.RPH_ERR_INVALID_ARG
    assert L.rph_library_create(eng.ctx, 40, None) == _lib.RPH_ERR_INVALID_ARG
    assert L.rph_library_destroy(None) == _lib.RPH_ERR_INVALID_ARG
    with eng.library(40) as lib:
        lib.reserve(5000)
        labels, cmp0 = lib.append(f.hashes[:300], f.coeffs[:300], f.has_features[:300], f.quality[:300])
        state = (len(lib), lib.comparisons, lib.groups())
        assert lib.append(np.zeros((0, 32), np.uint8))[1] == 0  # n_new == 0: RPH_OK, nothing changes
        cmp_out = C.c_uint64(99)
        assert L.rph_library_append(lib.handle, None, None, None, None, 5, None, C.byref(cmp_out)) == _lib.RPH_ERR_INVALID_ARG
        assert L.rph_library_append(None, f.hashes.ctypes.data_as(C.c_void_p), None, None, None, 5, None, None) == _lib.RPH_ERR_INVALID_ARG
        assert L.rph_library_append(lib.handle, f.hashes.ctypes.data_as(C.c_void_p), None, None, None, 2**31, None, None) == _lib.RPH_ERR_INVALID_ARG
        ng = C.c_uint32()
        members = np.zeros(300, np.uint32)
        assert L.rph_library_groups(lib.handle, None, members.ctypes.data_as(C.c_void_p), C.byref(ng)) == _lib.RPH_ERR_INVALID_ARG
        assert L.rph_library_query(lib.handle, None, None, 3, None, 0, C.byref(cmp_out)) == _lib.RPH_ERR_INVALID_ARG
        assert L.rph_library_restore(lib.handle, None, None, None, None, 3, None, None, 0, 0) == _lib.RPH_ERR_INVALID_ARG
        for first, count in ((0, 301), (300, 1), (301, 0), (2**40, 1)):
            with pytest.raises(RphError) as err:
                lib.labels(first, count)
            assert err.value.status == _lib.RPH_ERR_INVALID_ARG
        assert len(lib.labels(300, 0)) == 0 and len(lib.labels(299, 1)) == 1
        assert (len(lib), lib.comparisons, lib.groups()) == state


def test_scanner_helper(eng, files):
    from rupphash_amd import scanner

    f = files
    q = [None if x < 0 else int(x) for x in f.quality[:800]]
    want, want_cmp = scanner.group_with_pdqhash(f.hashes[:800], 40, f.coeffs[:800], f.has_features[:800], q, engine=eng)
    with scanner.open_library(40, engine=eng) as lib:
        lib.append(f.hashes[:600], f.coeffs[:600], f.has_features[:600], q[:600])
        labels, _ = lib.append(f.hashes[600:800], f.coeffs[600:800], f.has_features[600:800], q[600:])
        assert lib.groups() == want and lib.comparisons == want_cmp and len(labels) == 200
        assert len(lib.query(f.hashes[:5], [None, 10, 90, None, 60])) >= 3
