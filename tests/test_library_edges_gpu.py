"""An edge-keeping library on the GPU (-m gpu; rph_library_create_tree): after every append and every removal its store holds the edges
of the sweep at `top` among the resident files, rph_library_merge_tree(t <= top) gives the bytes of rph_group_files_pdq_tree(t) without a
sweep, and every existing call answers as a plain library at the same similarity does.  Models: merge_tree_model.py for the files and the
trees, removal_corpus.py for removals, numpy for the pairs of featureless hashes.  Every comparison is of whole arrays, byte for byte;
downloaded stores are sorted by (i, j, d, flags) first."""
import ctypes as C
import functools

import numpy as np
import pytest

import library_corpus as lc
import merge_tree_model as M
import removal_corpus as rc

pytestmark = pytest.mark.gpu

SIM, TOP = 40, 63
CUTS = (0, 1, 31, 39, 40, 41, 62, 63)


@pytest.fixture(scope="module")
def eng():
    from rupphash_amd import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def grid(eng):
    """G: one pass of the kernels' grid-stride loops (rph_stride_lanes_per_pass)"""
    return 8 * eng.device_info()[1] * 256


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def stats(eng, lib):
    """(growths of the store, edges the last append found at top, united of them, edges the last removal dropped, last merge_tree swept)"""
    out = (C.c_uint64 * 5)()
    assert eng.L.rph_debug_library_edge_stats(lib.handle, out) == 0
    return tuple(out)


def by_key(e):
    return e[np.lexsort((e["flags"], e["d"], e["j"], e["i"]))]


def sort3(ijd):
    ijd = np.asarray(ijd, np.int64).reshape(-1, 3)
    return ijd[np.lexsort((ijd[:, 2], ijd[:, 1], ijd[:, 0]))]


def store_of(lib):
    """the store, sorted, as (i, j, d)"""
    e = by_key(lib.edges())
    top, n_edges, _ = lib.edge_info()
    assert n_edges == len(e) and (e["i"] < e["j"]).all() and (len(e) == 0 or e["j"].max() < len(lib)) and (e["d"] <= top).all()
    return np.stack([e["i"], e["j"], e["d"]], axis=1).astype(np.int64)


@functools.lru_cache(maxsize=None)
def file_edges(top, n=None):
    """M.file_edges of the first n files of M.files(), sorted"""
    return sort3(M.file_edges(M.files(), top, n))


def same(tree, want):
    return (tree.into.tobytes(), tree.level.tobytes(), tree.edges_at.tobytes()) == (want.into.tobytes(), want.level.tobytes(), want.edges_at.tobytes())


def state_of(lib):
    return lib.groups(), lib.labels().tobytes(), len(lib), lib.comparisons


def pair_edges(hashes, top):
    """(i, j, d) of every pair i < j of featureless, confident files within top: what the variant sweep reports for them"""
    bits = np.unpackbits(np.ascontiguousarray(hashes, np.uint8).reshape(-1, 32), axis=1).astype(np.float32)
    ones = bits.sum(axis=1)
    d = np.rint(ones[:, None] + ones[None, :] - 2 * (bits @ bits.T)).astype(np.int64)
    i, j = np.nonzero(np.triu(d <= top, 1))
    return sort3(np.stack([i, j, d[i, j]], axis=1))


def mirror_edges(m, top):
    """(i, j, d) of what the variant sweep at top reports among the files of a removal_corpus.Mirror, in numpy: per pair i < j one edge per
    row of file i (its 8 rows if the library holds it with features, else its hash) within the pair's limit, 0 if either is low-confidence"""
    n = len(m)
    if n < 2:
        return np.zeros((0, 3), np.int64)
    cols = np.unpackbits(np.ascontiguousarray(m.hashes), axis=1).astype(np.float32)
    rows = np.unpackbits(np.ascontiguousarray(m.rows).reshape(n * 8, 32), axis=1).astype(np.float32)
    d = np.rint(rows.sum(axis=1)[:, None] + cols.sum(axis=1)[None, :] - 2 * (rows @ cols.T)).astype(np.int16).reshape(n, 8, n)
    low = M.is_low(m.quality)
    limit = np.where(low[:, None] | low[None, :], 0, top)
    owns = (np.arange(8)[None, :] == 0) | (m.hf[:, None] != 0)  # a file without features owns row 0 only
    below = np.arange(n)[:, None] < np.arange(n)[None, :]
    i, v, j = np.nonzero((d <= limit[:, None, :]) & owns[:, :, None] & below[:, None, :])
    return sort3(np.stack([i, j, d[i, v, j]], axis=1))


def removed_edges(n, ijd, removed):
    """the store after a removal: (kept edges renumbered and sorted, dropped in all)"""
    new = rc.new_index(n, removed).astype(np.int64)
    gone = (new[ijd[:, :2]] == rc.GONE).any(axis=1)
    kept = ijd[~gone].copy()
    kept[:, :2] = new[kept[:, :2]]
    return sort3(kept), int(gone.sum())


def nested_flips(base, sizes, seed=5):
    """one hash per entry of sizes: `base` with the first sizes[k] bits of one fixed permutation flipped, so d(a, b) = |sizes[a] - sizes[b]|"""
    perm = np.random.default_rng(seed).permutation(256)
    out = np.repeat(base[None, :], len(sizes), axis=0).copy()
    for k, m in enumerate(sizes):
        for b in perm[:m]:
            out[k, b // 8] ^= np.uint8(1 << (b % 8))
    return out


def check_trees(eng, lib, args, cuts=CUTS, what=None):
    """merge_tree(t) from the store against the file form and the host form on the same files, with no sweep"""
    from rupphash_amd import engine as E

    for t in cuts:
        got = lib.merge_tree(t)
        assert stats(eng, lib)[4] == 0, (what, t)
        assert same(got, eng.group_files_pdq_tree(args["hashes"], t, args.get("coeffs"), args.get("has_features"), args.get("quality"))), (what, t)
        assert same(got, E.merge_tree_host(top=t, **args)), (what, t)


# ---------------------------------------------------------------- real file arguments
def piece(a, first, last):
    return {k: v[first:last] for k, v in a.items()}


def feed(lib, a, first, last):
    p = piece(a, first, last)
    return lib.append(p["hashes"], p["coeffs"], p["has_features"], p["quality"])


@pytest.mark.parametrize("similarity,top", [(SIM, TOP), (40, 40), (0, 0)], ids=["40-63", "40-40", "0-0"])
def test_three_appends_equal_the_file_forms_and_a_plain_library(eng, similarity, top):
    a = M.file_args()
    n = len(a["hashes"])
    rng = np.random.default_rng(31)
    queries = np.concatenate([a["hashes"][rng.choice(n, 20, replace=False)], rng.integers(0, 256, (4, 32), dtype=np.uint8)])
    with eng.library(similarity, top=top) as lib, eng.library(similarity) as plain:
        assert lib.edge_info() == (top, 0, 1 << 28) and len(lib.edges()) == 0
        assert len(lib.merge_tree(top)) == 0 and stats(eng, lib)[4] == 0
        for first, last in ((0, 100), (100, 257), (257, n)):
            got, want = feed(lib, a, first, last), feed(plain, a, first, last)
            assert np.array_equal(got[0], want[0]) and got[1] == want[1], (first, last)  # labels_out, new_comparisons_out
            assert state_of(lib) == state_of(plain), (first, last)
            edges = file_edges(top, last)
            assert np.array_equal(store_of(lib), edges), (first, last)
            assert stats(eng, lib)[2] == want[1] and stats(eng, lib)[1] == len(edges) - (0 if first == 0 else len(file_edges(top, first)))
            prefix = piece(a, 0, last)
            check_trees(eng, lib, prefix, [t for t in CUTS if t <= top], (first, last))
            for s in [s for s in M.SIMS if s <= top]:
                assert lib.groups_at(s) == eng.group_files_pdq(prefix["hashes"], s, prefix["coeffs"], prefix["has_features"], prefix["quality"])[0], (last, s)
            assert state_of(lib) == state_of(plain), (first, last)  # the trees changed nothing
            assert np.array_equal(by_key(lib.query(queries)), by_key(plain.query(queries))), (first, last)
        # the other calls a plain library answers
        groups = plain.groups()
        pivots = [g[0] for g in groups]
        assert lib.group_max_dist(groups, pivots) == plain.group_max_dist(groups, pivots)
        ids = np.array([0, 5, n - 1], np.uint32)
        for x, y in zip(lib.nearest_files(ids, 4), plain.nearest_files(ids, 4)):
            assert np.array_equal(x, y)
        lib.reserve(4 * n)
        assert state_of(lib) == state_of(plain) and np.array_equal(store_of(lib), file_edges(top, n))


def test_a_t_above_the_stores_top_takes_the_sweep(eng):
    a = M.file_args()
    with eng.library(40, top=40) as lib:
        feed(lib, a, 0, 130), feed(lib, a, 130, len(a["hashes"]))
        before, store = state_of(lib), store_of(lib)
        got = lib.merge_tree(63)
        assert stats(eng, lib)[4] == 1
        assert same(got, eng.group_files_pdq_tree(a["hashes"], 63, a["coeffs"], a["has_features"], a["quality"]))
        assert state_of(lib) == before and np.array_equal(store_of(lib), store)
        assert same(lib.merge_tree(40), eng.group_files_pdq_tree(a["hashes"], 40, a["coeffs"], a["has_features"], a["quality"])) and stats(eng, lib)[4] == 0
    with eng.library(40) as plain:  # a plain library sweeps, as ever
        feed(plain, a, 0, len(a["hashes"]))
        assert same(plain.merge_tree(40), eng.group_files_pdq_tree(a["hashes"], 40, a["coeffs"], a["has_features"], a["quality"])) and stats(eng, plain)[4] == 1


def test_scanner_library_passes_top_on(eng):
    from rupphash_amd import scanner

    a = M.file_args(60)
    quality = [None if q < 0 else int(q) for q in a["quality"]]
    with scanner.open_library(SIM, top=TOP, engine=eng) as lib:
        lib.append(a["hashes"], a["coeffs"], a["has_features"], quality)
        assert lib.edge_info()[0] == TOP and np.array_equal(store_of(lib), file_edges(TOP, 60))
        assert lib.groups_at(SIM) == lib.groups()
        with scanner.open_library(SIM, top=TOP, engine=eng) as again:
            again.restore_edges(a["hashes"], lib.edges(), a["coeffs"], a["has_features"], quality)
            assert state_of(again) == state_of(lib)


# ---------------------------------------------------------------- wave and block seams of the append kernel
def seam_hashes(count, spread, first=0):
    """featureless files: all one hash, or (spread) nested flips of 3 x % 7 bits, so that d = 0 .. 6 straddles a similarity of 2 under a
    top of 8 and every file has a neighbour more than 2 away among the files before it"""
    base = np.random.default_rng(404).integers(0, 256, 32, dtype=np.uint8)
    return nested_flips(base, [3 * (first + x) % 7 if spread else 0 for x in range(count)])


@pytest.mark.parametrize("spread", [False, True], ids=["one-hash", "d-0-to-6"])
@pytest.mark.parametrize("k", [1, 63, 64, 65, 255, 256, 257])
def test_cross_and_inner_edges_behind_one_cursor(eng, k, spread):
    from rupphash_amd import engine as E

    similarity, top = (2, 8) if spread else (SIM, TOP)
    for extra in (1, 2):  # k cross edges and no inner one; 2 k cross edges and one inner
        hashes = seam_hashes(k + extra, spread)
        with eng.library(similarity, top=top) as lib, eng.library(similarity) as plain:
            labels, cmp_count = lib.append(hashes[:k])  # into an empty library: inner edges only
            resident = pair_edges(hashes[:k], top)
            assert len(resident) == k * (k - 1) // 2 and np.array_equal(store_of(lib), resident)
            assert stats(eng, lib)[1:3] == (len(resident), int((resident[:, 2] <= similarity).sum())) and cmp_count == stats(eng, lib)[2]
            assert (np.array_equal(labels, plain.append(hashes[:k])[0]))
            labels, cmp_count = lib.append(hashes[k:])
            want = pair_edges(hashes, top)
            added = want[want[:, 1] >= k]
            assert len(added) == extra * k + (extra == 2) and np.array_equal(store_of(lib), want)
            united = int((added[:, 2] <= similarity).sum())
            assert stats(eng, lib)[1:3] == (len(added), united) and cmp_count == united
            assert united < len(added) if spread else united == len(added)
            assert (np.array_equal(labels, plain.append(hashes[k:])[0])) and state_of(lib) == state_of(plain)
            assert np.array_equal(lib.labels(), lc.min_labels(k + extra, want[want[:, 2] <= similarity][:, :2]))
            got = lib.merge_tree(top)
            assert same(got, E.merge_tree_from_edges_host(M.edge_array(want), k + extra, top)) and stats(eng, lib)[4] == 0
            assert lib.groups_at(similarity) == lib.groups()


# ---------------------------------------------------------------- past one grid pass, past the sweep's first capacity
DENSE_M = 1500


@pytest.fixture(scope="module")
def dense():
    """1500 files around one hash, d(a, b) = |a % 64 - b % 64| -- a clique at 63 with every distance 0 .. 63 -- and an unrelated hash behind
    every 40 of them: (hashes, edges at 63)"""
    hashes, common = lc.dense_hashes(DENSE_M)
    ids = np.nonzero(common)[0]
    hashes = hashes.copy()
    hashes[ids] = nested_flips(hashes[ids[0]], [x % 64 for x in range(len(ids))])
    edges = pair_edges(hashes, TOP)
    assert len(edges) == DENSE_M * (DENSE_M - 1) // 2 and set(np.unique(edges[:, 2])) == set(range(64))
    return hashes, edges


def dense_library(eng, dense, first=37):
    hashes, _ = dense
    lib = eng.library(SIM, top=TOP)
    lib.append(hashes[:first])
    lib.append(hashes[first:])
    return lib


def test_a_store_past_one_grid_pass_and_the_sweeps_first_capacity(eng, grid, dense):
    from rupphash_amd import engine as E

    hashes, edges = dense
    n, first = len(hashes), 37
    with dense_library(eng, dense, first) as lib:
        found, united = stats(eng, lib)[1:3]
        added = edges[edges[:, 1] >= first]
        # the premises: the second append's edges overflow the capacity its retry loop tries first, with a store behind it; the store
        # takes the append kernel, and later the filter, round their loops again
        assert found == len(added) > lc.library_first_cap(n - first) and len(edges) > grid and len(edges) - len(added) > 0
        assert united == int((added[:, 2] <= SIM).sum()) < found
        assert np.array_equal(store_of(lib), edges)
        host = E.merge_tree_host(hashes, TOP)
        assert same(lib.merge_tree(TOP), host) and same(lib.merge_tree(SIM), E.merge_tree_truncate(host, SIM)) and stats(eng, lib)[4] == 0
        assert same(host, E.merge_tree_from_edges_host(M.edge_array(edges), n, TOP))
        assert (lib.groups(), lib.comparisons) == eng.group_files_pdq(hashes, SIM) == (host.groups(SIM), host.comparisons(SIM))
        assert lib.groups_at(17) == eng.group_files_pdq(hashes, 17)[0]


def test_removal_from_a_store_past_one_grid_pass(eng, grid, dense):
    from rupphash_amd import engine as E

    hashes, edges = dense
    n = len(hashes)
    removed = np.union1d(rc.grid_removals(n), np.random.default_rng(8).choice(n, 150, replace=False)).astype(np.uint32)
    with dense_library(eng, dense) as lib, eng.library(SIM) as plain:
        plain.append(hashes)
        want, dropped_all = removed_edges(n, edges, removed)
        assert len(want) > grid
        new, dropped = lib.remove(removed)
        assert dropped == plain.remove(removed)[1] == removed_edges(n, edges[edges[:, 2] <= SIM], removed)[1]
        assert np.array_equal(new, rc.new_index(n, removed)) and stats(eng, lib)[3] == dropped_all
        assert np.array_equal(store_of(lib), want) and state_of(lib) == state_of(plain)
        rest = hashes[new != rc.GONE]
        assert same(lib.merge_tree(TOP), E.merge_tree_host(rest, TOP)) and stats(eng, lib)[4] == 0
        assert (lib.groups(), lib.comparisons) == eng.group_files_pdq(rest, SIM)


# ---------------------------------------------------------------- growth and the bound
def test_the_store_grows_and_keeps_its_edges(eng):
    hashes = seam_hashes(48, True)
    with eng.library(2, top=8) as lib:
        assert eng.L.rph_debug_library_edge_store(lib.handle, 64) == 0
        growths = []
        for last in (12, 20, 32, 48):  # 66, 190, 496, 1128 edges: every append adds more than the store held
            before = lib.edge_info()[1]
            lib.append(hashes[len(lib):last])
            want = pair_edges(hashes[:last], 8)
            assert len(want) == last * (last - 1) // 2 > 2 * before and np.array_equal(store_of(lib), want), last
            growths.append(stats(eng, lib)[0])
        assert growths[0] == 0 and growths == sorted(set(growths)) and growths[-1] == 3, growths  # 64 x 2: the first allocation is no growth
        assert np.array_equal(lib.labels(), lc.min_labels(48, want[want[:, 2] <= 2][:, :2]))
        assert eng.L.rph_debug_library_edge_store(lib.handle, 0) == 0


def test_max_edges_refuses_an_append_and_changes_nothing(eng):
    from rupphash_amd import RphError, _lib

    hashes = seam_hashes(23, False)
    with eng.library(SIM, top=TOP, max_edges=100) as lib:
        lib.append(hashes[:10])
        before, store = state_of(lib), store_of(lib)
        assert lib.edge_info() == (TOP, 45, 100)
        with pytest.raises(RphError) as err:
            lib.append(hashes[10:20])  # 100 cross + 45 inner edges more
        assert err.value.status == _lib.RPH_ERR_CAPACITY
        assert state_of(lib) == before and np.array_equal(store_of(lib), store) and lib.edge_info() == (TOP, 45, 100)
        labels, cmp_count = lib.append(hashes[20:])  # 30 + 3
        assert cmp_count == 33 and not labels.any() and lib.edge_info() == (TOP, 78, 100)
        assert np.array_equal(store_of(lib), pair_edges(hashes[:13], TOP)) and lib.groups() == [list(range(13))]


# ---------------------------------------------------------------- removal
def removal_sets():
    f = M.files()
    n = len(f.hashes)
    rng = np.random.default_rng(66)
    clique = np.nonzero(f.family == 0)[0]
    return n, {"grid": rc.grid_removals(n), "random": rng.choice(n, n // 5, replace=False), "all-of-one-clique": clique,
               "none-of-a-clique": np.nonzero(f.family < 0)[0][::3], "every-file": np.arange(n)}


@pytest.mark.parametrize("which", ["grid", "random", "all-of-one-clique", "none-of-a-clique", "every-file"])
def test_removal_filters_the_store(eng, which):
    a = M.file_args()
    n, sets = removal_sets()
    removed = np.asarray(sets[which], np.uint32)
    edges = file_edges(TOP)
    with eng.library(SIM, top=TOP) as lib, eng.library(SIM) as plain:
        for x in (lib, plain):
            feed(x, a, 0, 130), feed(x, a, 130, n)
        want, dropped_all = removed_edges(n, edges, removed)
        _, kept_near, dropped_near, labels, groups = rc.remove_from_edges(n, edges[edges[:, 2] <= SIM][:, :2], removed)
        if which == "none-of-a-clique":
            assert dropped_all == 0 and len(removed) > 10
        if which == "all-of-one-clique":
            assert dropped_near > 0
        new, dropped = lib.remove(removed)
        assert np.array_equal(new, rc.new_index(n, removed)) and dropped == dropped_near == plain.remove(removed)[1]
        assert stats(eng, lib)[3] == dropped_all
        assert np.array_equal(store_of(lib), want) and state_of(lib) == state_of(plain)
        assert (lib.groups(), lib.comparisons) == (groups, len(kept_near)) and np.array_equal(lib.labels(), labels)
        keep = new != rc.GONE
        rest = {k: v[keep] for k, v in a.items()}
        if keep.any():
            check_trees(eng, lib, rest, (0, SIM, TOP), which)
            assert (lib.groups(), lib.comparisons) == eng.group_files_pdq(rest["hashes"], SIM, rest["coeffs"], rest["has_features"], rest["quality"])
        else:
            assert len(lib) == 0 and lib.edge_info() == (TOP, 0, 1 << 28) and len(lib.merge_tree(TOP)) == 0
            feed(lib, a, 0, 130)  # an emptied library goes on
            assert np.array_equal(store_of(lib), file_edges(TOP, 130))


def test_appends_and_removals_interleaved(eng):
    files = lc.corpus()
    rng = np.random.default_rng(4711)
    with eng.library(SIM, top=TOP) as lib, eng.library(SIM) as plain:
        m = rc.Mirror(files)

        def check(what):
            assert state_of(lib) == state_of(plain), what
            args = dict(hashes=m.hashes, coeffs=m.coeffs, has_features=m.hf, quality=m.quality)
            tree = lib.merge_tree(TOP)
            assert stats(eng, lib)[4] == 0 and same(tree, eng.group_files_pdq_tree(m.hashes, TOP, m.coeffs, m.hf, m.quality)), what
            assert (tree.groups(SIM), tree.comparisons(SIM)) == (lib.groups(), lib.comparisons), what
            with eng.library(SIM, top=TOP) as fresh:  # the store of one append of the same files: the records as one sweep emits them
                fresh.append(**args)
                assert np.array_equal(by_key(lib.edges()), by_key(fresh.edges())), what
            assert lib.edge_info()[1] == int(tree.edges_at.sum()), what
            assert np.array_equal(store_of(lib), mirror_edges(m, TOP)), what  # and the pairs of the mirror's files, by numpy

        def append(ids, with_coeffs=True):
            hashes, kw = m.appended(ids, with_coeffs)
            got, want = lib.append(hashes, **kw), plain.append(hashes, **kw)
            assert np.array_equal(got[0], want[0]) and got[1] == want[1]

        def remove(count):
            idx = rng.choice(len(m), count, replace=False).astype(np.uint32)
            got, want = lib.remove(idx), plain.remove(idx)
            assert np.array_equal(got[0], want[0]) and got[1] == want[1]
            m.removed(idx)

        append(np.arange(0, 900)), check("900 appended")
        remove(90), check("90 removed")
        append(np.arange(900, lc.N_FILES), with_coeffs=False), check("the rest appended without coefficients")
        remove(400), check("400 removed")
        append(np.arange(0, 300)), check("300 appended again")


# ---------------------------------------------------------------- persistence
def test_edges_restore_a_library(eng):
    a = M.file_args()
    n = len(a["hashes"])
    with eng.library(SIM, top=TOP) as lib:
        feed(lib, a, 0, 200)
        e = lib.edges()
        with eng.library(SIM, top=TOP) as again, eng.library(31, top=TOP) as other:
            p = piece(a, 0, 200)
            again.restore_edges(p["hashes"], e[np.random.default_rng(2).permutation(len(e))], p["coeffs"], p["has_features"], p["quality"])
            assert state_of(again) == state_of(lib) and np.array_equal(by_key(again.edges()), by_key(e))
            assert same(again.merge_tree(TOP), lib.merge_tree(TOP)) and stats(eng, again)[4] == 0
            got, want = feed(again, a, 200, n), feed(lib, a, 200, n)  # a later append behaves the same
            assert np.array_equal(got[0], want[0]) and got[1] == want[1] and state_of(again) == state_of(lib)
            assert np.array_equal(by_key(again.edges()), by_key(lib.edges()))
            new, dropped = again.remove([0, 7, n - 1])  # and a removal finds the count it expects
            assert (np.array_equal(new, lib.remove([0, 7, n - 1])[0])) and state_of(again) == state_of(lib)
            # the same edges under another similarity: the groups of that similarity
            other.restore_edges(p["hashes"], e, p["coeffs"], p["has_features"], p["quality"])
            assert (other.groups(), other.comparisons) == eng.group_files_pdq(p["hashes"], 31, p["coeffs"], p["has_features"], p["quality"])


def test_restore_edges_refuses_bad_edges_and_stays_empty(eng):
    from rupphash_amd import RphError, _lib

    a = M.file_args(50)
    with eng.library(SIM, top=40) as src:
        feed(src, a, 0, 50)
        good = src.edges()
        assert len(good) > 3
    with eng.library(SIM, top=40) as lib:
        for name, field, value in [("j outside n", "j", 50), ("i not below j", "i", None), ("d above top", "d", 41)]:
            bad = good.copy()
            bad[field][len(bad) // 2] = bad["j"][len(bad) // 2] if value is None else value
            with pytest.raises(RphError) as err:
                lib.restore_edges(a["hashes"], bad, a["coeffs"], a["has_features"], a["quality"])
            assert err.value.status == _lib.RPH_ERR_INVALID_ARG, name
            assert len(lib) == 0 and lib.comparisons == 0 and lib.edge_info() == (40, 0, 1 << 28) and len(lib.edges()) == 0, name
        with pytest.raises(RphError) as err:  # groups alone cannot fill a store
            lib.restore(a["hashes"], src_groups(eng, a), 0, a["coeffs"], a["has_features"], a["quality"])
        assert err.value.status == _lib.RPH_ERR_INVALID_ARG and len(lib) == 0
        lib.restore_edges(a["hashes"], good, a["coeffs"], a["has_features"], a["quality"])  # the next call is right
        assert (lib.groups(), lib.comparisons) == eng.group_files_pdq(a["hashes"], SIM, a["coeffs"], a["has_features"], a["quality"])
        with pytest.raises(RphError) as err:  # only an empty library
            lib.restore_edges(a["hashes"], good, a["coeffs"], a["has_features"], a["quality"])
        assert err.value.status == _lib.RPH_ERR_INVALID_ARG and len(lib) == 50
        # the download's capacity protocol: the count always, the records only if they fit
        out, found = np.full(len(good), 0xA5, np.uint8).repeat(12), C.c_uint64()
        assert eng.L.rph_library_edges(lib.handle, ptr(out), len(good) - 1, C.byref(found)) == _lib.RPH_ERR_CAPACITY
        assert found.value == len(good) and (out == 0xA5).all()
        assert eng.L.rph_library_edges(lib.handle, ptr(out), len(good), C.byref(found)) == _lib.RPH_OK and found.value == len(good)


def test_a_store_that_is_not_the_files_own_refuses_the_removal_and_changes_nothing(eng):
    """restore_edges takes the caller's word: an edge that passes the range check but that no sweep reports.  The removal of one of its
    files then drops one edge more from the store than the regroup counts: RPH_ERR_HIP with both numbers, and the library as it was"""
    from rupphash_amd import RphError, _lib

    a = M.file_args(50)
    own = file_edges(40, 50)
    labels = lc.min_labels(50, own[:, :2])
    alone = [x for x in range(50) if (labels == labels[x]).sum() == 1]
    assert len(alone) >= 3 and len(own) > 3
    x, y, z = alone[0], alone[-1], alone[1]
    with eng.library(SIM, top=40) as src:
        feed(src, a, 0, 50)
        good = src.edges()
    extra = np.zeros(1, M.EDGE)
    extra["i"], extra["j"], extra["d"] = x, y, 17
    with eng.library(SIM, top=40) as lib:
        lib.restore_edges(a["hashes"], np.concatenate([good, extra]), a["coeffs"], a["has_features"], a["quality"])
        assert lib.comparisons == len(own) + 1 and lib.labels()[y] == x  # taken at its word
        before, store = state_of(lib), by_key(lib.edges())
        for victim in (y, x):
            with pytest.raises(RphError) as err:
                lib.remove([victim])
            assert err.value.status == _lib.RPH_ERR_HIP and "regroup counted 0" in str(err.value) and "drops 1 edges" in str(err.value), str(err.value)
            assert state_of(lib) == before and np.array_equal(by_key(lib.edges()), store) and lib.edge_info() == (40, len(own) + 1, 1 << 28)
        new, dropped = lib.remove([z])  # a file the extra edge does not touch: both routes agree, the library goes on
        assert dropped == 0 and len(lib) == 49 and lib.edge_info()[1] == len(own) + 1


def src_groups(eng, a):
    return eng.group_files_pdq(a["hashes"], SIM, a["coeffs"], a["has_features"], a["quality"])[0]


def test_a_plain_library_has_no_store(eng):
    from rupphash_amd import RphError, _lib

    a = M.file_args(50)
    with eng.library(SIM) as plain:
        assert plain.edge_info() == (None, 0, 0)
        with pytest.raises(RphError) as err:
            plain.restore_edges(a["hashes"], np.zeros(0, M.EDGE))
        assert err.value.status == _lib.RPH_ERR_INVALID_ARG and len(plain) == 0
        feed(plain, a, 0, 50)
        before = state_of(plain)
        with pytest.raises(RphError) as err:
            plain.edges()
        assert err.value.status == _lib.RPH_ERR_INVALID_ARG
        top, n_edges, cap = C.c_uint32(7), C.c_uint64(7), C.c_uint64(7)
        assert eng.L.rph_library_edge_info(plain.handle, C.byref(top), C.byref(n_edges), C.byref(cap)) == _lib.RPH_OK
        assert (top.value, n_edges.value, cap.value) == (_lib.RPH_NO_EDGE_STORE, 0, 0) and state_of(plain) == before
        assert stats(eng, plain)[:4] == (0, 0, 0, 0)
    h = C.c_void_p()
    for similarity, top in ((41, 40), (0, 64), (64, 64)):
        assert eng.L.rph_library_create_tree(eng.ctx, similarity, top, 0, C.byref(h)) == _lib.RPH_ERR_INVALID_ARG and not h.value
