"""What an edge-keeping library needs without a GPU: rph_merge_tree_truncate against the rule in numpy (merge_tree_model.py) and against
rph_merge_tree_from_edges_host on the filtered edge list, for every hand-made case and every t; its refusals; and the argument checks of
the Python wrappers that touch no device.  Every comparison is of whole arrays, byte for byte."""
import ctypes as C

import numpy as np
import pytest

import library_corpus as lc
import merge_tree_model as M

CASES = {c.name: c for c in M.edge_cases()}


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def same(tree, want):
    return (tree.into.tobytes(), tree.level.tobytes(), tree.edges_at.tobytes()) == (want.into.tobytes(), want.level.tobytes(), want.edges_at.tobytes())


@pytest.fixture
def memo_labels(monkeypatch):
    """M.tree_of asks lc.min_labels for the labels at every s; the trees for t = 0 .. top ask for the same ones over and over.  The function
    is pure: remember its answers for the length of one test."""
    seen, plain = {}, lc.min_labels

    def min_labels(n, edges):
        key = (n, np.asarray(edges).tobytes())
        if key not in seen:
            seen[key] = plain(n, edges)
        return seen[key]

    monkeypatch.setattr(lc, "min_labels", min_labels)


@pytest.mark.parametrize("name", list(CASES))
def test_truncate_is_the_tree_of_the_filtered_edges_at_every_t(name, memo_labels):
    from rupphash_amd import engine as E

    c = CASES[name]
    ijd = M.global_ijd(c)
    full = E.merge_tree_from_edges_host(M.edge_array(ijd), c.n, c.top)
    assert same(full, M.tree_of(c.n, ijd, c.top)), name
    for t in range(c.top + 1):
        below = ijd[ijd[:, 2] <= t]
        got = E.merge_tree_truncate(full, t)
        assert got.top == t and len(got) == c.n
        assert same(got, M.tree_of(c.n, below, t)), (name, t)
        assert same(got, E.merge_tree_from_edges_host(M.edge_array(below), c.n, t)), (name, t)
    assert same(full, E.merge_tree_from_edges_host(M.edge_array(ijd), c.n, c.top))  # the input was not touched


@pytest.mark.parametrize("name", ["ladder-0-64", "every-edge-8-times-differing-d", "empty-levels", "n-1", "random-3000-over-5000"])
def test_truncate_in_place(name):
    from rupphash_amd import _lib
    from rupphash_amd import engine as E

    c = CASES[name]
    ijd = M.global_ijd(c)
    full = E.merge_tree_from_edges_host(M.edge_array(ijd), c.n, c.top)
    for t in sorted({0, 1, c.top // 2, c.top - 1 if c.top else 0, c.top}):
        want = E.merge_tree_truncate(full, t)
        into, level, at = full.into.copy(), full.level.copy(), full.edges_at.copy()
        assert _lib.load().rph_merge_tree_truncate(ptr(into), ptr(level), ptr(at), c.n, c.top, t, ptr(into), ptr(level), ptr(at)) == _lib.RPH_OK
        assert (into.tobytes(), level.tobytes(), at[:t + 1].tobytes()) == (want.into.tobytes(), want.level.tobytes(), want.edges_at.tobytes()), (name, t)
        assert np.array_equal(at[t + 1:], full.edges_at[t + 1:])  # nothing behind the first t + 1 entries


def test_truncate_refusals_write_nothing():
    from rupphash_amd import _lib
    from rupphash_amd import engine as E

    L = _lib.load()
    n, top = 6, 20
    good = E.merge_tree_from_edges_host(M.edge_array([(0, 1, 3), (1, 2, 5), (3, 4, 5), (2, 4, 9)]), n, top)
    assert good.into.tolist() == [0, 0, 0, 0, 3, 5] and good.level.tolist() == [255, 3, 5, 9, 5, 255]

    def call(into, level, at, top, t):
        out = np.full(n, 0xA5A5A5A5, np.uint32), np.full(n, 0xA5, np.uint8), np.full(top + 1, 0xA5A5A5A5A5A5A5A5, np.uint64)
        rc = L.rph_merge_tree_truncate(ptr(into), ptr(level), ptr(at), n, top, t, ptr(out[0]), ptr(out[1]), ptr(out[2]))
        return rc, (out[0] == 0xA5A5A5A5).all() and (out[1] == 0xA5).all() and (out[2] == 0xA5A5A5A5A5A5A5A5).all()

    assert call(good.into, good.level, good.edges_at, top, top) == (_lib.RPH_OK, False)
    assert call(good.into, good.level, good.edges_at, top, top + 1) == (_lib.RPH_ERR_INVALID_ARG, True)  # t above top
    assert call(good.into, good.level, np.zeros(256, np.uint64), 255, 3) == (_lib.RPH_ERR_INVALID_ARG, True)  # 255 is RPH_TREE_NEVER
    bad = []
    into = good.into.copy()
    into[1] = 2  # into[x] above x
    bad.append(("into above x", into, good.level))
    level = good.level.copy()
    level[5] = 7  # into[x] == x with a level
    bad.append(("root with a level", good.into, level))
    level = good.level.copy()
    level[2] = 255  # into[x] < x without one
    bad.append(("joined without a level", good.into, level))
    level = good.level.copy()
    level[4] = 9  # 4 joins 3 at 9, 3 joins 0 at 9: the level does not rise
    bad.append(("level does not rise", good.into, level))
    for name, into, level in bad:
        assert call(into, level, good.edges_at, top, 9) == (_lib.RPH_ERR_INVALID_ARG, True), name
        assert L.rph_merge_tree_labels(ptr(into), ptr(level), n, 9, ptr(np.zeros(n, np.uint32))) == _lib.RPH_ERR_INVALID_ARG, name  # the same sense
    out = np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.zeros(top + 1, np.uint64)
    for k in range(3):  # a null output; a null input is a malformed tree
        args = [ptr(a) for a in out]
        args[k] = None
        assert L.rph_merge_tree_truncate(ptr(good.into), ptr(good.level), ptr(good.edges_at), n, top, 3, *args) == _lib.RPH_ERR_INVALID_ARG
    assert L.rph_merge_tree_truncate(None, ptr(good.level), ptr(good.edges_at), n, top, 3, *[ptr(a) for a in out]) == _lib.RPH_ERR_INVALID_ARG
    assert L.rph_merge_tree_truncate(ptr(good.into), ptr(good.level), None, n, top, 3, *[ptr(a) for a in out]) == _lib.RPH_ERR_INVALID_ARG
    assert not out[0].any() and not out[1].any() and not out[2].any()
    assert L.rph_merge_tree_truncate(None, None, ptr(good.edges_at), 0, top, 3, None, None, ptr(out[2])) == _lib.RPH_OK  # no files: only edges_at
    assert np.array_equal(out[2][:4], good.edges_at[:4]) and not out[2][4:].any()


def test_python_wrappers_check_their_arguments_before_any_device_call():
    from rupphash_amd import Engine, RphError, _lib, scanner
    from rupphash_amd import engine as E

    tree = E.merge_tree_from_edges_host(M.edge_array([(0, 1, 3)]), 2, 10)
    with pytest.raises(ValueError):
        E.merge_tree_truncate(tree, -1)
    with pytest.raises(RphError) as err:
        E.merge_tree_truncate(tree, 11)
    assert err.value.status == _lib.RPH_ERR_INVALID_ARG
    assert E.merge_tree_truncate is Engine.merge_tree_truncate
    nobody = Engine.__new__(Engine)  # never reached: the checks come first
    nobody.L, nobody.ctx = None, None
    for similarity, top in [(40, 39), (40, 64), (0, -1), (64, 64)]:
        with pytest.raises(ValueError):
            E.Library(nobody, similarity, top=top)
        with pytest.raises(ValueError):
            scanner.open_library(similarity, top=top, engine=nobody)
    with pytest.raises(ValueError):
        E.Library(nobody, 40, top=63, max_edges=-1)
    with pytest.raises(TypeError, match="engine="):  # the engine where `top` now stands
        scanner.open_library(40, nobody)
    assert _lib.RPH_NO_EDGE_STORE == 0xFFFFFFFF
    for name in ("rph_library_create_tree", "rph_library_edge_info", "rph_library_edges", "rph_library_restore_edges", "rph_merge_tree_truncate"):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)
    for name in ("rph_debug_library_edge_store", "rph_debug_library_edge_stats"):
        assert name in _lib.DEBUG_SIGNATURES and name not in _lib.SIGNATURES
