"""rph_library_remove on the GPU (-m gpu): after every removal -- and every append after it -- groups, labels, size and comparison count
are those of rph_group_files_pdq on the files that are left, in order, and new_index is what numpy says; a refused call changes nothing;
the regroup survives an edge buffer that is too small; and libraries beyond one grid of the removal kernels compact and relabel right.
test_library_remove_cpu.py pins the expectations used here against the CPU oracle."""
import ctypes as C

import numpy as np
import pytest

import library_corpus as lc
import removal_corpus as rc

pytestmark = pytest.mark.gpu

SIMS = (0, 16, 40, 63)  # those of test_library_gpu.py


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


def stats(eng, lib):
    """(m, edges the regroup found, first edge capacity tried, lanes of one pass of the removal kernels) of the last removal"""
    out = (C.c_uint64 * 4)()
    assert eng.L.rph_debug_library_remove_stats(lib.handle, out) == 0
    return tuple(out)


def regrouped(eng, sim, m):
    """rph_group_files_pdq on the files of the mirror: (groups, comparisons)"""
    if len(m) == 0:
        return [], 0
    if m.hf.any():
        return eng.group_files_pdq(m.hashes, sim, m.coeffs, m.hf, m.quality)
    return eng.group_files_pdq(m.hashes, sim, quality=m.quality)


def labels_of(groups, n):
    want = np.arange(n, dtype=np.uint32)
    for g in groups:
        want[g] = g[0]
    return want


def state_of(lib):
    return lib.groups(), lib.labels().tobytes(), len(lib), lib.comparisons


def check(eng, lib, m, what=None):
    want_groups, want_cmp = regrouped(eng, lib.similarity, m)
    assert len(lib) == len(m), what
    assert lib.groups() == want_groups, what
    assert np.array_equal(lib.labels(), labels_of(want_groups, len(m))), what
    assert lib.comparisons == want_cmp, what
    return want_groups


def append(lib, m, ids, with_coeffs=True):
    hashes, kw = m.appended(ids, with_coeffs)
    return lib.append(hashes, **kw)


def remove(eng, lib, m, indices, what=None):
    """one removal, checked: new_index against numpy, the count against dropped, the state against the regroup of what is left"""
    indices = np.asarray(indices, np.uint32)
    n, before = len(lib), lib.comparisons
    new, dropped = lib.remove(indices)
    assert new.dtype == np.uint32 and np.array_equal(new, rc.new_index(n, indices)), what
    m.removed(indices)
    assert before - dropped == lib.comparisons, what
    groups = check(eng, lib, m, what)
    return new, dropped, groups


def filled(eng, files, sim):
    lib, m = eng.library(sim), rc.Mirror(files)
    append(lib, m, np.arange(lc.N_FILES))
    return lib, m


# ---------------------------------------------------------------- the 1 901-file corpus
def test_removing_the_bridge_splits_its_component(eng, files):
    b = lc.BRIDGE
    lib, m = filled(eng, files, 40)
    with lib:
        assert [b["a"], b["a2"], b["b"], b["b2"], b["c"]] in check(eng, lib, m)
        new, dropped, groups = remove(eng, lib, m, [b["c"]])
        assert [b["a"], b["a2"]] in groups and [b["b"], b["b2"]] in groups and dropped == 4
        assert stats(eng, lib)[0] == 5  # the five members of the one component that lost a file were swept again


@pytest.mark.parametrize("root,other", [(0, 1), (3, 1500)])
def test_removing_a_root_moves_the_label_to_the_next_member(eng, files, root, other):
    lib, m = filled(eng, files, 40)
    with lib:
        assert list(lib.labels(other, 1)) == [root] and [root, other] in lib.groups()
        new, dropped, groups = remove(eng, lib, m, [root])
        assert dropped >= 1 and list(lib.labels(int(new[other]), 1)) == [new[other]]  # the pair dissolved: the other file is its own root
    # a larger component: its root goes, the next member takes over
    lib, m = filled(eng, files, 40)
    with lib:
        big = max(lib.groups(), key=len)
        assert len(big) >= 3
        new, dropped, groups = remove(eng, lib, m, [big[0]])
        rest = [int(new[x]) for x in big[1:]]
        # (remove() has compared the whole state with the regroup.)  The smallest member left is the smallest of whatever part of
        # the component it is in now, so it is its own root; and a part of the old component takes in no file from outside it
        assert list(lib.labels(rest[0], 1)) == [rest[0]]
        assert all(set(g) <= set(rest) for g in groups if set(g) & set(rest))


def test_removing_a_singleton_only_renumbers(eng, files):
    lib, m = filled(eng, files, 40)
    with lib:
        labels = lib.labels()
        alone = np.nonzero((labels == np.arange(len(labels))) & (np.bincount(labels, minlength=len(labels)) == 1))[0]
        x = int(alone[(alone > 500) & (alone < 1400)][0])
        groups_before = lib.groups()
        new, dropped, groups = remove(eng, lib, m, [x])
        assert dropped == 0 and stats(eng, lib)[0] in (0, 1) and stats(eng, lib)[1] == 0
        assert groups == [[int(new[y]) for y in g] for g in groups_before]


def test_removing_low_confidence_and_featureless_files(eng, files):
    for sim in (16, 40):
        lib, m = filled(eng, files, sim)
        with lib:
            low = np.nonzero((m.quality >= 0) & (m.quality < 50))[0]
            assert len(low) > 100
            remove(eng, lib, m, low, "low confidence")
            featureless = np.nonzero(m.hf == 0)[0]
            assert len(featureless) > 50
            remove(eng, lib, m, featureless, "featureless")
            assert m.hf.all() and not ((m.quality >= 0) & (m.quality < 50)).any()


def test_nothing_everything_and_all_but_one(eng, files):
    f = files
    lib, m = filled(eng, files, 40)
    with lib:
        before = state_of(lib)
        new, dropped = lib.remove([])
        assert dropped == 0 and np.array_equal(new, np.arange(lc.N_FILES)) and state_of(lib) == before
        remove(eng, lib, m, np.random.default_rng(1).permutation(lc.N_FILES))  # everything, in any order
        assert len(lib) == 0 and lib.comparisons == 0 and lib.groups() == [] and len(lib.labels()) == 0
        assert len(lib.query(f.hashes[:5])) == 0
        new, dropped = lib.remove([])
        assert len(new) == 0 and dropped == 0
        # the empty library takes a restore again, and appends onto it
        old = rc.Mirror(f)
        old.appended(np.arange(1500))
        old_groups, old_cmp = regrouped(eng, 40, old)
        lib.restore(f.hashes[:1500], old_groups, old_cmp, f.coeffs[:1500], f.has_features[:1500], f.quality[:1500])
        m.appended(np.arange(1500))
        check(eng, lib, m, "restored")
        append(lib, m, np.arange(1500, lc.N_FILES))
        check(eng, lib, m, "restored and appended")
        remove(eng, lib, m, [x for x in range(lc.N_FILES) if x != 1], "all but one")
        assert len(lib) == 1 and list(lib.labels()) == [0]
        append(lib, m, [0])  # file 0 behind file 1: their pair again, the other way round
        assert check(eng, lib, m) == [[0, 1]]
        remove(eng, lib, m, [1, 0])
        append(lib, m, np.arange(300))  # an append onto a library that a removal emptied
        check(eng, lib, m, "emptied and appended")


@pytest.mark.parametrize("seed", (11, 12, 13))
@pytest.mark.parametrize("share", (0, 0.1, 0.5, 0.9), ids=("one-file", "10%", "50%", "90%"))
@pytest.mark.parametrize("sim", SIMS)
def test_random_sets(eng, files, sim, share, seed):
    rng = np.random.default_rng([seed, sim, int(share * 10)])
    lib, m = filled(eng, files, sim)
    with lib:
        new, dropped, _ = remove(eng, lib, m, rng.choice(lc.N_FILES, max(1, int(share * lc.N_FILES)), replace=False))
        if sim >= 40 and share >= 0.5:
            assert dropped > 0
        # twice in a row, then the files come back as new ones behind the rest
        remove(eng, lib, m, rng.choice(len(m), max(1, len(m) // 3), replace=False), "second removal")
        append(lib, m, np.nonzero(new == rc.GONE)[0][:200], with_coeffs=seed != 12)
        check(eng, lib, m, "appended after two removals")


@pytest.mark.parametrize("order", ("append-remove", "remove-append"))
@pytest.mark.parametrize("split", lc.SPLITS[1:], ids=lambda s: "-".join(map(str, s)) if len(s) < 6 else "19x100-1")
def test_interleaved_with_appends(eng, files, split, order):
    rng = np.random.default_rng([77, len(split), order == "append-remove"])
    with eng.library(40) as lib:
        m = rc.Mirror(files)
        if order == "remove-append":  # everything resident first; every batch then replaces a random set of the same size
            append(lib, m, np.arange(lc.N_FILES))
        for k, (first, last) in enumerate(lc.batches(split)):
            if order == "append-remove":
                append(lib, m, np.arange(first, last), with_coeffs=k % 3 != 2)
                check(eng, lib, m, (split, k, "appended"))
                if len(m):
                    remove(eng, lib, m, rng.choice(len(m), (len(m) + 9) // 10, replace=False), (split, k, "removed"))
            else:
                if last > first:
                    remove(eng, lib, m, rng.choice(len(m), min(last - first, len(m) - 1), replace=False), (split, k, "removed"))
                append(lib, m, np.arange(first, last), with_coeffs=k % 3 != 2)
                check(eng, lib, m, (split, k, "appended"))


def test_query_after_a_removal_matches_numpy_on_the_survivors(eng, files):
    f = files
    rng = np.random.default_rng(909)
    with eng.library(40) as lib:
        m = rc.Mirror(f)
        append(lib, m, np.arange(700))
        append(lib, m, np.arange(700, 1500), with_coeffs=False)
        remove(eng, lib, m, rng.choice(1500, 450, replace=False))
        n = len(m)
        assert n == 1050
        q_hashes = np.concatenate([m.hashes[rng.integers(0, n, 100)], f.hashes[1500:1650], f.hashes[[1400, 1700]], rng.integers(0, 256, (48, 32), dtype=np.uint8)])
        n_q = len(q_hashes)
        ba = np.unpackbits(m.rows.reshape(-1, 32), axis=1).astype(np.float32)
        bb = np.unpackbits(q_hashes, axis=1).astype(np.float32)
        dist = (ba.sum(1)[:, None] + bb.sum(1)[None, :] - 2.0 * (ba @ bb.T)).astype(np.int64).reshape(n, 8, n_q)  # exact: integers <= 256
        owned = (m.hf[:, None] != 0) | (np.arange(8)[None, :] == 0)
        low = (m.quality >= 0) & (m.quality < 50)
        limit = np.where(low[:, None], 0, 40) * np.ones((1, n_q), np.int64)
        i, v, j = np.nonzero((dist <= limit[:, None, :]) & owned[:, :, None])
        want = sorted(zip(i.tolist(), j.tolist(), v.tolist(), dist[i, v, j].tolist()))
        before = state_of(lib)
        got = lib.query(q_hashes)
        assert (got["i"] < n).all() and len(want) > 100
        assert sorted(zip(got["i"].tolist(), got["j"].tolist(), ((got["flags"] >> 9) & 7).tolist(), got["d"].tolist())) == want
        assert state_of(lib) == before


def mixed_case(eng, files):
    """appends and removals in turn, every step checked under the kernel that is set; the states it went through"""
    b = lc.BRIDGE
    rng = np.random.default_rng(404)
    states = []
    with eng.library(40) as lib:
        m = rc.Mirror(files)
        append(lib, m, np.arange(1023))
        new, _, _ = remove(eng, lib, m, np.concatenate([[0, b["a"]], rng.choice(np.arange(400, 1023), 150, replace=False)]))
        states.append(state_of(lib))
        append(lib, m, np.arange(1023, lc.N_FILES))
        check(eng, lib, m)
        states.append(state_of(lib))
        c = int(np.nonzero(m.ids == b["c"])[0][0])
        remove(eng, lib, m, np.concatenate([[c], rng.choice(c, 300, replace=False)]))
        states.append(state_of(lib))
    return states


@pytest.mark.parametrize("kernel", [0, 1, 2, 3, 4])
def test_a_mixed_case_under_every_hamming_kernel(eng, files, kernel):
    eng.set_hamming_kernel(2)
    want = mixed_case(eng, files)
    try:
        eng.set_hamming_kernel(kernel)
        assert mixed_case(eng, files) == want
    finally:
        eng.set_hamming_kernel(2)


def test_refused_calls_change_nothing(eng, files):
    from rupphash_amd import RphError, _lib

    lib, m = filled(eng, files, 40)
    with lib:
        remove(eng, lib, m, [5, 900])
        n = len(lib)
        before = state_of(lib)
        new = np.full(n, 7, np.uint32)
        dropped = C.c_uint64(99)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        bad = {"index = size": [3, n], "far outside": [0xFFFFFFFF], "listed twice": [10, 200, 10], "more than there are": list(range(n)) + [0]}
        for name, idx in bad.items():
            idx = np.array(idx, np.uint32)
            assert eng.L.rph_library_remove(lib.handle, ptr(idx), len(idx), ptr(new), C.byref(dropped)) == _lib.RPH_ERR_INVALID_ARG, name
            assert state_of(lib) == before, name
            with pytest.raises(RphError) as err:
                lib.remove(idx)
            assert err.value.status == _lib.RPH_ERR_INVALID_ARG and state_of(lib) == before, name
        assert eng.L.rph_library_remove(lib.handle, None, 3, ptr(new), C.byref(dropped)) == _lib.RPH_ERR_INVALID_ARG
        assert eng.L.rph_library_remove(None, ptr(new), 1, None, None) == _lib.RPH_ERR_INVALID_ARG
        assert state_of(lib) == before
        # both outputs are optional, and a null list of no files is fine
        assert eng.L.rph_library_remove(lib.handle, None, 0, None, None) == _lib.RPH_OK and state_of(lib) == before
        one = np.array([200], np.uint32)
        assert eng.L.rph_library_remove(lib.handle, ptr(one), 1, None, None) == _lib.RPH_OK
        m.removed(one)
        check(eng, lib, m)


def test_two_libraries_on_one_engine(eng, files):
    one, m1 = filled(eng, files, 40)
    two, m2 = filled(eng, files, 16)
    with one, two:
        other = state_of(two)
        remove(eng, one, m1, np.arange(0, lc.N_FILES, 3))
        assert state_of(two) == other
        mine = state_of(one)
        remove(eng, two, m2, np.arange(1, lc.N_FILES, 2))
        assert state_of(one) == mine
        check(eng, one, m1)
        append(one, m1, np.arange(50))
        check(eng, one, m1)
        check(eng, two, m2)


def test_scanner_library_inherits_remove(eng, files):
    from rupphash_amd import scanner

    f = files
    q = [None if x < 0 else int(x) for x in f.quality[:800]]
    keep = np.ones(800, bool)
    keep[[0, 10, 799]] = False
    qk = [x for x, k in zip(q, keep) if k]
    want = scanner.group_with_pdqhash(f.hashes[:800][keep], 40, f.coeffs[:800][keep], f.has_features[:800][keep], qk, engine=eng)
    with scanner.open_library(40, engine=eng) as lib:
        lib.append(f.hashes[:800], f.coeffs[:800], f.has_features[:800], q)
        new, dropped = lib.remove([799, 0, 10])
        assert np.array_equal(new, rc.new_index(800, [0, 10, 799])) and (lib.groups(), lib.comparisons) == want


# ---------------------------------------------------------------- the regroup past its first edge buffer
DENSE_SIM = 31


@pytest.mark.parametrize("eight", (False, True), ids=("one-row-1500", "eight-rows-300+400"))
def test_dense_regroup_overflows_the_edge_buffer(eng, oracle, eight):
    rows = 8 if eight else 1
    c = 700 if eight else 1500
    hashes, common = lc.dense_hashes(c, common=np.zeros(32, np.uint8) if eight else None)
    n = len(hashes)
    hf = common.astype(np.uint8)  # (eight rows: the unrelated files keep to their hash)
    coeffs = np.zeros((n, 256), np.float32)  # zero coefficients hash to the all-zero hash, eight times
    kw = lambda a, b: dict(coeffs=coeffs[a:b], has_features=hf[a:b]) if eight else {}  # noqa: E731
    cut = int(np.nonzero(common)[0][300]) if eight else 0
    victim = int(np.nonzero(common)[0][c // 2])
    with eng.library(DENSE_SIM) as lib:
        if cut:
            lib.append(hashes[:cut], **kw(0, cut))
        lib.append(hashes[cut:], **kw(cut, n))
        labels, groups, cmp_count = lc.dense_expectation(common, rows)
        assert lib.comparisons == cmp_count == rows * c * (c - 1) // 2 and lib.groups() == groups
        new, dropped = lib.remove([victim])
        m, found, first_cap, _ = stats(eng, lib)
        # the premise: the regroup of the c identical files (the removed one included) did not fit the capacity it tried first
        assert m == c and found == cmp_count and found > first_cap, (m, found, first_cap)
        assert np.array_equal(new, rc.new_index(n, [victim]))
        stay = new != rc.GONE
        want_labels, want_groups, want_cmp = lc.dense_expectation(common[stay], rows)
        assert (dropped, want_cmp) == rc.dense_minus_one(c, rows)
        assert lib.comparisons == want_cmp and lib.groups() == want_groups and np.array_equal(lib.labels(), want_labels) and len(lib) == n - 1
        regroup = eng.group_files_pdq(hashes[stay], DENSE_SIM, coeffs[stay], hf[stay]) if eight else eng.group_files_pdq(hashes[stay], DENSE_SIM)
        assert regroup == (want_groups, want_cmp)
        # ten more files (without coefficients) still agree
        more = np.concatenate([np.repeat(hashes[:1], 5, axis=0), np.random.default_rng(7).integers(0, 256, (5, 32), dtype=np.uint8)])
        all_hashes, all_hf = np.concatenate([hashes[stay], more]), np.concatenate([hf[stay], np.zeros(10, np.uint8)])
        labels, new_cmp = lib.append(more)
        assert new_cmp == rows * (c - 1) * 5 + 10 and list(labels[:5]) == [0] * 5
        regroup = eng.group_files_pdq(all_hashes, DENSE_SIM, np.zeros((n + 9, 256), np.float32), all_hf) if eight else eng.group_files_pdq(all_hashes, DENSE_SIM)
        assert (lib.groups(), lib.comparisons) == regroup
        variants = np.repeat(all_hashes[:, None, :], 8, axis=1)
        ref_edges, ref_groups = oracle.group_pdq(all_hashes, DENSE_SIM, variants=variants if eight else None, has_features=all_hf if eight else None)
        assert regroup == (ref_groups, len(ref_edges))


# ---------------------------------------------------------------- past one grid
GRID_CASES = {"G+77": (0, False), "2G+1": (1, False), "2G+1-every-odd-file": (1, True)}


@pytest.mark.parametrize("case", list(GRID_CASES))
def test_libraries_beyond_one_grid(eng, case):
    which, odd = GRID_CASES[case]
    with eng.library(rc.BLOCK_SIM) as lib:
        G = stats(eng, lib)[3]  # lanes of one pass of the removal kernels, as the library says
        assert G >= 256 and G % 256 == 0
        n = lc.grid_sizes(G)[which]
        hashes = rc.block_hashes(n, 31 + which)
        labels, groups, cmp_count = rc.block_state(np.ones(n, bool))
        lib.restore(hashes, groups, cmp_count)  # no sweep
        assert len(lib) == n and lib.comparisons == cmp_count and np.array_equal(lib.labels(), labels)
        # every file with x % 1000 == 1, the first and the last: the flag, label and gather loops (sixteen lanes per file) take more than
        # one pass.  The list of indices and the regroup's edges stay inside one; the third case removes every odd file as well, which
        # takes both past it and regroups every block
        removed = np.union1d(rc.grid_removals(n), np.arange(1, n, 2)).astype(np.uint32) if odd else rc.grid_removals(n)
        assert n > G and 16 * (n - len(removed)) > G and len(removed) * 4 > n // 1000
        new, dropped = lib.remove(removed[np.random.default_rng(3).permutation(len(removed))])
        want_new = rc.new_index(n, removed)
        assert np.array_equal(new, want_new)
        stay = want_new != rc.GONE
        want_labels, want_groups, want_cmp = rc.block_state(stay)
        m, found = stats(eng, lib)[:2]
        if odd:
            assert len(removed) > G and found > G and m == n
        assert m <= 4 * len(removed) and dropped == cmp_count - want_cmp
        assert len(lib) == n - len(removed) and np.array_equal(lib.labels(), want_labels)
        got_groups = lib.groups()
        assert got_groups == rc.groups_as_lists(want_groups) and lib.comparisons == want_cmp
        assert (got_groups, want_cmp) == eng.group_files_pdq(hashes[stay], rc.BLOCK_SIM)  # the rows moved with their files
        # the compacted rows are what later calls sweep: one more copy of a survivor from each end joins its block
        k = len(lib)
        labels, new_cmp = lib.append(hashes[stay][[2, k - 1]])
        assert list(labels) == [want_labels[2], want_labels[k - 1]]
        hits = lib.query(hashes[stay][[k // 2]])
        assert sorted(hits["i"].tolist()) == np.nonzero(want_labels == want_labels[k // 2])[0].tolist()
