"""The merge tree on the GPU (-m gpu): rph_merge_tree_dev on hand-made edge lists and beyond one grid against rph_merge_tree_from_edges_host
and the rule in numpy (merge_tree_model.py; test_merge_tree_cpu.py pins both without a GPU), and the file forms -- rph_group_files_pdq_tree,
rph_library_merge_tree -- against rph_merge_tree_host, the model and, cut at every listed similarity, rph_group_files_pdq itself.  Every
comparison is of whole arrays, byte for byte."""
import ctypes as C

import numpy as np
import pytest

import library_corpus as lc
import merge_tree_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from rupphash_amd import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def caller_stream(eng):
    st = eng.stream_create()
    yield st
    eng.stream_destroy(st)


@pytest.fixture(scope="module")
def grid(eng):
    """G: one pass of the kernels' grid-stride loops (rph_stride_lanes_per_pass)"""
    return 8 * eng.device_info()[1] * 256


class DeviceArray:
    def __init__(self, eng, arr):
        self.eng, self.nbytes = eng, arr.nbytes
        self.ptr = eng.dev_alloc(max(arr.nbytes, 16))
        if arr.nbytes:
            eng.dev_upload(self.ptr, arr)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.eng.dev_free(self.ptr)

    def download(self, dtype):
        out = np.zeros(self.nbytes // np.dtype(dtype).itemsize, dtype)
        if self.nbytes:
            self.eng.dev_download(out, self.ptr)
        return out


def as_edges(ijd):
    e = M.edge_array(ijd)
    e["flags"] = 0x8E2A  # what the tree must not look at
    return e


def same(tree, want):
    return (tree.into.tobytes(), tree.level.tobytes(), tree.edges_at.tobytes()) == (want.into.tobytes(), want.level.tobytes(), want.edges_at.tobytes())


def device_tree(eng, edges, n, top, i_base=0, j_base=0, with_labels=False, stream=None, prefill=None):
    """rph_merge_tree_dev over host edge records: (MergeTree, labels or None).  The outputs start as `prefill` says (or as 0xA5 bytes)."""
    from rupphash_amd import MergeTree

    start = prefill or (np.full(n, 0xA5A5A5A5, np.uint32), np.full(n, 0xA5, np.uint8), np.full(top + 1, 0xA5A5, np.uint64), np.full(n, 0xA5A5A5A5, np.uint32))
    with DeviceArray(eng, edges) as d_e, DeviceArray(eng, start[0]) as d_into, DeviceArray(eng, start[1]) as d_level, DeviceArray(eng, start[2]) as d_at, \
            DeviceArray(eng, start[3]) as d_lab:
        try:
            eng.merge_tree_dev(d_e.ptr if len(edges) else None, len(edges), n, top, d_into.ptr, d_level.ptr, d_at.ptr, d_lab.ptr if with_labels else None, i_base, j_base,
                               stream=stream)
        finally:
            eng.stream_synchronize(stream)
            got = MergeTree(d_into.download(np.uint32), d_level.download(np.uint8), d_at.download(np.uint64)), d_lab.download(np.uint32)
            device_tree.last = got
    return got[0], (got[1] if with_labels else None)


# ---------------------------------------------------------------- the core on hand-made edge lists
CASES = {c.name: c for c in M.edge_cases()}


@pytest.mark.parametrize("with_labels", [False, True], ids=["tree", "tree+labels"])
@pytest.mark.parametrize("name", list(CASES))
def test_core_matches_the_host_form_and_the_rule(eng, caller_stream, name, with_labels):
    from rupphash_amd import engine as E

    c = CASES[name]
    ijd = M.global_ijd(c)
    want = M.tree_of(c.n, ijd, c.top)
    host = E.merge_tree_from_edges_host(M.edge_array(ijd), c.n, c.top)
    got, labels = device_tree(eng, as_edges(c.edges), c.n, c.top, c.i_base, c.j_base, with_labels, stream=caller_stream if with_labels else None)
    assert same(got, host) and same(got, want), name
    if with_labels:  # the flattened min-labels at top: what the union-find over ALL the edges leaves
        assert np.array_equal(labels, want.labels[c.top]), name
        with DeviceArray(eng, np.arange(c.n, dtype=np.uint32)) as d_lab, DeviceArray(eng, as_edges(c.edges)) as d_e:
            eng.union_find_labels_dev(d_e.ptr if len(c.edges) else None, len(c.edges), d_lab.ptr, c.n, c.i_base, c.j_base)
            eng.synchronize()
            assert np.array_equal(labels, d_lab.download(np.uint32)), name


def test_same_level_chain_in_every_order_ends_at_the_final_root(eng):
    """recording the root at CAS time would leave into[3] at 2 or 1 in some order"""
    for name, c in CASES.items():
        if name.startswith("same-level-chain"):
            got, _ = device_tree(eng, as_edges(c.edges), 4, c.top)
            assert got.into.tolist() == [0, 0, 0, 0] and got.level.tolist() == [255, 9, 9, 9], name


def test_the_ladders_queue_a_launch_pair_per_level(eng):
    c = CASES["ladder-0-64"]
    got, _ = device_tree(eng, as_edges(c.edges), c.n, c.top)
    assert got.level.tolist() == [255] + list(range(64)) and not got.into.any() and got.edges_at.tolist() == [1] * 64
    m = CASES["ladder-hub-last"]
    got, _ = device_tree(eng, as_edges(m.edges), m.n, m.top)
    assert got.level.tolist() == [255] + [64 - x for x in range(1, 64)] + [0] and got.into.tolist() == [0] + list(range(63)) + [63]


def test_n_zero_without_edges_is_ok(eng):
    with DeviceArray(eng, np.full(64, 7, np.uint64)) as d_at:
        eng.merge_tree_dev(None, 0, 0, 63, None, None, d_at.ptr)
        eng.synchronize()
        assert not d_at.download(np.uint64).any()


@pytest.mark.parametrize("family,size", M.LARGE_TREE_CASES)
def test_core_beyond_one_grid_matches_the_closed_form(eng, grid, family, size):
    from rupphash_amd import engine as E

    n, ijd, into, level = M.large_tree_case(grid, family, size)
    assert n > grid and len(ijd) >= lc.grid_sizes(grid)[size == "2G+1"]
    got, labels = device_tree(eng, as_edges(ijd), n, 63, with_labels=True)
    assert np.array_equal(got.into, into) and np.array_equal(got.level, level)
    assert np.array_equal(got.edges_at, np.bincount(ijd[:, 2], minlength=64).astype(np.uint64))
    assert np.array_equal(labels, into)  # depth one: the label at top is where the file went
    assert same(got, E.merge_tree_from_edges_host(M.edge_array(ijd), n, 63))


def test_refusals_write_nothing_and_the_next_call_is_right(eng):
    from rupphash_amd import RphError, _lib

    n, top = 300, 40
    good = np.stack([np.arange(0, 200), np.arange(100, 300), np.arange(200) % 41], axis=1)
    want = M.tree_of(n, good, top)
    for name, bad_edge, i_base, j_base in [("d above top", (1, 2, 41), 0, 0), ("j outside n", (0, 300, 3), 0, 0), ("i outside n", (300, 0, 3), 0, 0),
                                             ("j + j_base outside n", (0, 250, 3), 0, 50), ("i + i_base outside n", (250, 0, 3), 50, 0)]:
        # one bad edge behind 200 good ones (under a base: behind one that stays inside n)
        ijd = np.array([(0, 1, 3), bad_edge]) if i_base or j_base else np.concatenate([good, [bad_edge]])
        fill = (np.full(n, 11, np.uint32), np.full(n, 12, np.uint8), np.full(top + 1, 13, np.uint64), np.full(n, 14, np.uint32))
        with pytest.raises(RphError) as err:
            device_tree(eng, as_edges(ijd), n, top, i_base, j_base, with_labels=True, prefill=fill)
        assert err.value.status == _lib.RPH_ERR_INVALID_ARG, name
        tree, labels = device_tree.last
        assert (tree.into == 11).all() and (tree.level == 12).all() and (tree.edges_at == 13).all() and (labels == 14).all(), name
        got, labels = device_tree(eng, as_edges(good), n, top, with_labels=True)
        assert same(got, want) and np.array_equal(labels, want.labels[top]), name
    with pytest.raises(RphError) as err:
        device_tree(eng, as_edges(good), n, 256)
    assert err.value.status == _lib.RPH_ERR_INVALID_ARG
    fill = (np.full(n, 11, np.uint32), np.full(n, 12, np.uint8), np.full(256, 13, np.uint64), np.full(n, 14, np.uint32))
    with pytest.raises(RphError) as err:  # 255 is RPH_TREE_NEVER: the largest top is 254
        device_tree(eng, as_edges(good), n, 255, with_labels=True, prefill=fill)
    tree, labels = device_tree.last
    assert err.value.status == _lib.RPH_ERR_INVALID_ARG and (tree.into == 11).all() and (tree.level == 12).all() and (tree.edges_at == 13).all() and (labels == 14).all()
    with pytest.raises(RphError) as err:
        eng.merge_tree_dev(C.c_void_p(16), 1, 0, 5, None, None, C.c_void_p(16))  # edges over an empty set: refused before anything is read
    assert err.value.status == _lib.RPH_ERR_INVALID_ARG


# ---------------------------------------------------------------- the file forms
@pytest.mark.parametrize("n", M.FILE_SIZES)
def test_file_form_matches_host_form_model_and_every_cut_matches_group_files_pdq(eng, n):
    from rupphash_amd import engine as E
    from rupphash_amd import scanner

    a = M.file_args(n)
    _, want = M.file_tree(n)
    got = eng.group_files_pdq_tree(a["hashes"], M.TOP, a["coeffs"], a["has_features"], a["quality"])
    assert same(got, want) and same(got, E.merge_tree_host(top=M.TOP, **a))
    for s in M.SIMS:
        assert (got.groups(s), got.comparisons(s)) == eng.group_files_pdq(a["hashes"], s, a["coeffs"], a["has_features"], a["quality"]), s
        assert np.array_equal(got.labels(s), want.labels[s]), s
    quality = [None if q < 0 else int(q) for q in a["quality"]]
    assert same(scanner.merge_tree(a["hashes"], M.TOP, a["coeffs"], a["has_features"], quality, engine=eng), want)


def test_file_form_without_coefficients_and_at_a_smaller_top(eng):
    from rupphash_amd import engine as E

    a = M.file_args()
    for top in (0, 31):
        got = eng.group_files_pdq_tree(a["hashes"], top, quality=a["quality"])
        assert same(got, E.merge_tree_host(a["hashes"], top, quality=a["quality"]))
        for s in (0, top):
            assert (got.groups(s), got.comparisons(s)) == eng.group_files_pdq(a["hashes"], s, quality=a["quality"])
    from rupphash_amd import _lib

    # above 63 the PDQ forms refuse, with nothing written
    h = np.ascontiguousarray(a["hashes"])
    into, level, at = np.full(len(h), 11, np.uint32), np.full(len(h), 12, np.uint8), np.full(65, 13, np.uint64)
    assert eng.L.rph_group_files_pdq_tree(eng.ctx, ptr(h), None, None, None, len(h), 64, ptr(into), ptr(level), ptr(at)) == _lib.RPH_ERR_INVALID_ARG
    assert eng.L.rph_group_files_pdq_tree(eng.ctx, None, None, None, None, len(h), 63, ptr(into), ptr(level), ptr(at)) == _lib.RPH_ERR_INVALID_ARG
    assert eng.L.rph_group_files_pdq_tree(eng.ctx, ptr(h), None, None, None, len(h), 63, ptr(into), None, ptr(at)) == _lib.RPH_ERR_INVALID_ARG
    assert eng.L.rph_group_files_pdq_tree(eng.ctx, ptr(h), None, None, None, len(h), 63, ptr(into), ptr(level), None) == _lib.RPH_ERR_INVALID_ARG
    assert (into == 11).all() and (level == 12).all() and (at == 13).all()


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def state_of(lib):
    return lib.groups(), lib.labels().tobytes(), len(lib), lib.comparisons


@pytest.mark.parametrize("similarity", [0, 63])
@pytest.mark.parametrize("n", [1, 2, 257])
def test_library_form_on_the_small_prefixes(eng, n, similarity):
    """one file: no sweep, no edge buffer; two: one pair; 257: past one block"""
    from rupphash_amd import engine as E

    a = M.file_args(n)
    _, want = M.file_tree(n)
    with eng.library(similarity) as lib:
        lib.append(a["hashes"], a["coeffs"], a["has_features"], a["quality"])
        before = state_of(lib)
        got = lib.merge_tree(M.TOP)
        assert same(got, want) and same(got, E.merge_tree_host(top=M.TOP, **a)) and state_of(lib) == before
        for s in M.SIMS:
            assert (got.groups(s), got.comparisons(s)) == eng.group_files_pdq(a["hashes"], s, a["coeffs"], a["has_features"], a["quality"]), s
    with eng.library(similarity) as lib:  # a fresh library whose first call this is: nothing of an append's is there yet
        lib.restore(a["hashes"], want_groups(want, similarity), int(want.edges_at[:similarity + 1].sum()), a["coeffs"], a["has_features"], a["quality"])
        before = state_of(lib)
        assert same(lib.merge_tree(M.TOP), want) and state_of(lib) == before


def want_groups(tree, s):
    return lc.groups_of(tree.labels[s])


def test_library_form_refusals_write_nothing_and_change_nothing(eng):
    from rupphash_amd import _lib

    a = M.file_args(40)
    with eng.library(31) as lib:
        lib.append(a["hashes"], a["coeffs"], a["has_features"], a["quality"])
        before = state_of(lib)
        into, level, at = np.full(40, 11, np.uint32), np.full(40, 12, np.uint8), np.full(65, 13, np.uint64)
        call = eng.L.rph_library_merge_tree
        assert call(lib.handle, 64, ptr(into), ptr(level), ptr(at)) == _lib.RPH_ERR_INVALID_ARG
        assert call(lib.handle, 63, None, ptr(level), ptr(at)) == _lib.RPH_ERR_INVALID_ARG
        assert call(lib.handle, 63, ptr(into), None, ptr(at)) == _lib.RPH_ERR_INVALID_ARG
        assert call(lib.handle, 63, ptr(into), ptr(level), None) == _lib.RPH_ERR_INVALID_ARG
        assert call(None, 63, ptr(into), ptr(level), ptr(at)) == _lib.RPH_ERR_INVALID_ARG
        assert (into == 11).all() and (level == 12).all() and (at == 13).all() and state_of(lib) == before
        assert same(lib.merge_tree(M.TOP), M.file_tree(40)[1]) and state_of(lib) == before  # the next call is right


@pytest.mark.parametrize("similarity", [0, 63])
def test_library_form_after_appends_and_a_removal(eng, similarity):
    from rupphash_amd import engine as E

    a = M.file_args()
    n = len(a["hashes"])
    _, want = M.file_tree()
    with eng.library(similarity) as lib:
        assert len(lib.merge_tree(M.TOP)) == 0
        for first, last in ((0, 130), (130, n)):  # in two pieces
            lib.append(a["hashes"][first:last], a["coeffs"][first:last], a["has_features"][first:last], a["quality"][first:last])
        before = state_of(lib)
        got = lib.merge_tree(M.TOP)
        assert same(got, want) and state_of(lib) == before
        assert (got.groups(similarity), got.comparisons(similarity)) == (before[0], before[3])  # the library's own groups are one cut of it
        for s in M.SIMS:
            assert (got.groups(s), got.comparisons(s)) == eng.group_files_pdq(a["hashes"], s, a["coeffs"], a["has_features"], a["quality"]), s
        # a removal: a root, a bridge of the path family, a filler and the last file
        f = M.files()
        gone = np.array([int(np.nonzero(f.family == 0)[0][0]), int(np.nonzero(f.family == 2)[0][2]), 1, n - 1])
        lib.remove(gone)
        keep = np.setdiff1d(np.arange(n), gone)
        rest = {k: v[keep] for k, v in a.items()}
        before = state_of(lib)
        got = lib.merge_tree(M.TOP)
        assert same(got, E.merge_tree_host(top=M.TOP, **rest)) and state_of(lib) == before
        for s in M.SIMS:
            assert (got.groups(s), got.comparisons(s)) == eng.group_files_pdq(rest["hashes"], s, rest["coeffs"], rest["has_features"], rest["quality"]), s
        assert same(lib.merge_tree(0), E.merge_tree_host(top=0, **rest))


def test_library_form_grows_its_edge_buffer(eng):
    """1500 files that share one hash: 1 124 250 edges at level 0, more than the capacity the call tries first"""
    hashes, common = lc.dense_hashes(1500)
    ids = np.nonzero(common)[0]
    with eng.library(31) as lib:
        lib.append(hashes)
        before = state_of(lib)
        got = lib.merge_tree(40)
        out = (C.c_uint64 * 2)()
        assert eng.L.rph_debug_library_merge_tree_stats(lib.handle, out) == 0
        found, first_cap = out
        assert found == 1500 * 1499 // 2 > first_cap, (found, first_cap)  # the premise
        level = np.full(len(hashes), 255, np.uint8)
        level[ids[1:]] = 0
        into = np.arange(len(hashes), dtype=np.uint32)
        into[ids[1:]] = ids[0]
        assert np.array_equal(got.level, level) and np.array_equal(got.into, into) and got.edges_at.tolist() == [found] + [0] * 40
        assert state_of(lib) == before and got.groups(31) == before[0] and got.comparisons(31) == before[3]
