"""The merge tree without a device: rph_merge_tree_host and rph_merge_tree_from_edges_host against the rule in numpy
(merge_tree_model.py), the consequences the header states, the cutting calls against counting, every refusal with its outputs untouched,
and the closed forms test_merge_tree_gpu.py uses at grid size against the definition."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import merge_tree_model as M


@pytest.fixture(scope="module")
def L():
    from rupphash_amd import _lib

    return _lib.load()


@pytest.fixture(scope="module")
def E():
    from rupphash_amd import engine

    return engine


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def same(tree, want):
    """identical bytes: into, level, edges_at"""
    return (tree.into.tobytes(), tree.level.tobytes(), tree.edges_at.tobytes()) == (want.into.tobytes(), want.level.tobytes(), want.edges_at.tobytes())


CASES = {c.name: c for c in M.edge_cases()}


@pytest.mark.parametrize("name", list(CASES))
def test_tree_from_edges_is_the_rule(E, name):
    c = CASES[name]
    ijd = M.global_ijd(c)
    want = M.tree_of(c.n, ijd, c.top)
    got = E.merge_tree_from_edges_host(M.edge_array(ijd), c.n, c.top)
    assert same(got, want), name
    M.check_consequences(got.into, got.level, c.top)
    # the tree does not depend on the order of the edges
    again = E.merge_tree_from_edges_host(M.edge_array(ijd[np.random.default_rng(3).permutation(len(ijd))]), c.n, c.top)
    assert same(again, want), name
    for s in range(c.top + 1):
        assert np.array_equal(got.labels(s), want.labels[s]), (name, s)
    groups, grouped = got.profile()
    want_groups, want_grouped = M.profile_of(want.labels)
    assert np.array_equal(groups, want_groups) and np.array_equal(grouped, want_grouped), name


def test_same_level_chain_ends_at_the_final_root(E):
    got = E.merge_tree_from_edges_host(M.edge_array([(2, 3, 9), (1, 2, 9), (0, 1, 9)]), 4, 20)
    assert got.into.tolist() == [0, 0, 0, 0] and got.level.tolist() == [255, 9, 9, 9]


def test_ladder_has_every_level_and_depth_one(E):
    c = CASES["ladder-0-64"]
    got = E.merge_tree_from_edges_host(M.edge_array(c.edges), c.n, c.top)
    assert got.level.tolist() == [255] + list(range(64)) and not got.into.any()
    assert M.check_consequences(got.into, got.level, 63) == 1
    # the mirror: file 64 joins 63 at level 0, and that component is absorbed by a smaller root at every level
    m = CASES["ladder-hub-last"]
    got = E.merge_tree_from_edges_host(M.edge_array(m.edges), m.n, m.top)
    assert got.level[64] == 0 and got.into[64] == 63 and got.level.tolist()[:64] == [255] + [64 - x for x in range(1, 64)]


@pytest.mark.parametrize("n", M.FILE_SIZES)
def test_host_form_is_the_rule_on_the_files(E, L, n):
    edges, want = M.file_tree(n)
    got = E.merge_tree_host(top=M.TOP, **M.file_args(n))
    assert same(got, want)
    M.check_consequences(got.into, got.level, M.TOP)
    assert same(E.merge_tree_from_edges_host(M.edge_array(edges), len(got), M.TOP), want)
    for s in range(M.TOP + 1):
        assert np.array_equal(got.labels(s), want.labels[s]), s
        assert got.comparisons(s) == int((edges[:, 2] <= s).sum()), s
        # the groups are those of the union-find over the edges within s
        within = M.edge_array(edges[edges[:, 2] <= s])
        members, offsets, ng = np.zeros(max(len(got), 1), np.uint32), np.zeros(len(got) // 2 + 2, np.uint32), C.c_uint32()
        assert L.rph_union_find_groups(ptr(within), len(within), len(got), ptr(members), ptr(offsets), C.byref(ng)) == 0
        assert got.groups(s) == [members[offsets[g]:offsets[g + 1]].tolist() for g in range(ng.value)], s
    groups, grouped = got.profile()
    want_groups, want_grouped = M.profile_of(want.labels)
    assert np.array_equal(groups, want_groups) and np.array_equal(grouped, want_grouped)


def test_the_corpus_holds_what_it_is_built_for():
    f = M.files()
    _, t = M.file_tree()
    fam = lambda k: np.nonzero(f.family == k)[0]  # noqa: E731
    assert sorted(t.level[fam(0)].tolist()) == [0, 1, 15, 16, 31, 32, 40, 255] and sorted(t.level[fam(1)].tolist()) == [47, 48, 63, 255]
    assert sorted(t.level[fam(2)].tolist()) == [20, 20, 63, 63, 255]
    i, j = fam(3)
    assert f.has_features[i] and not f.has_features[j] and t.level[j] == 20 and t.into[j] == i  # through variant 5 of file i alone
    assert (t.level[fam(4)] == 255).all()  # the other index order: the featureless file's only row is its hash
    assert t.level[fam(5)].tolist() == [255, 0] and (t.level[fam(6)] == 255).all()  # low-confidence twins: at 0 only
    a, b, c, d = fam(7)
    assert (t.level[b], t.into[b], t.level[c], t.into[c], t.level[d]) == (0, a, 1, a, 255)
    assert sorted(t.level[fam(8)].tolist()) == [0, 63, 255] and (t.level[fam(9)] == 255).all()
    assert len(f.hashes) > 257 and fam(10).min() >= 257 and (f.has_features == 0).sum() > 100


@pytest.mark.parametrize("family,size", M.LARGE_TREE_CASES)
def test_closed_forms_of_the_grid_cases(E, family, size):
    n, ijd, into, level = M.large_tree_case(1024, family, size)
    want = M.tree_of(n, ijd, 63)
    assert np.array_equal(want.into, into) and np.array_equal(want.level, level)
    got = E.merge_tree_from_edges_host(M.edge_array(ijd), n, 63)
    assert same(got, want)


def test_small_sets_and_top_zero(E, L):
    for n in (0, 1, 2):
        got = E.merge_tree_from_edges_host(M.edge_array([]), n, 0)
        assert got.into.tolist() == list(range(n)) and got.level.tolist() == [255] * n and got.edges_at.tolist() == [0]
        got = E.merge_tree_host(np.zeros((n, 32), np.uint8), 0)
        want_level = [255, 0][:n] if n == 2 else [255] * n  # two identical hashes join at 0
        assert got.level.tolist() == want_level and got.edges_at.tolist() == [n == 2] and got.groups(0) == ([[0, 1]] if n == 2 else [])
        assert got.profile()[0].tolist() == [n == 2] and got.labels(0).tolist() == [0] * n
    got = E.merge_tree_from_edges_host(M.edge_array([(1, 0, 0)]), 2, 0)
    assert got.into.tolist() == [0, 0] and got.level.tolist() == [255, 0] and got.edges_at.tolist() == [1]


def filled(n, top):
    return np.full(n, 0xABABABAB, np.uint32), np.full(n, 0xCD, np.uint8), np.full(top + 1, 0xEFEF, np.uint64)


def test_refusals_leave_the_outputs_untouched(E, L):
    from rupphash_amd import _lib

    bad = _lib.RPH_ERR_INVALID_ARG
    for name, edges, n, top in [("file outside n", [(0, 5, 1)], 5, 10), ("i outside n", [(7, 0, 1)], 5, 10), ("d above top", [(0, 1, 11)], 5, 10),
                                ("top above 255", [(0, 1, 1)], 5, 256), ("top 255 is NEVER", [(0, 1, 1)], 5, 255), ("edges over nothing", [(0, 0, 0)], 0, 3)]:
        e = M.edge_array(edges)
        into, level, at = filled(max(n, 1), min(top, 255))
        keep = (into.tobytes(), level.tobytes(), at.tobytes())
        assert L.rph_merge_tree_from_edges_host(ptr(e), len(e), n, top, ptr(into), ptr(level), ptr(at)) == bad, name
        assert (into.tobytes(), level.tobytes(), at.tobytes()) == keep, name
    into, level, at = filled(4, 70)
    keep = (into.tobytes(), level.tobytes(), at.tobytes())
    h = np.zeros((4, 32), np.uint8)
    assert L.rph_merge_tree_host(ptr(h), None, None, None, 4, 64, ptr(into), ptr(level), ptr(at)) == bad  # the PDQ forms stop at 63
    assert L.rph_merge_tree_host(None, None, None, None, 4, 63, ptr(into), ptr(level), ptr(at)) == bad
    assert L.rph_merge_tree_host(ptr(h), None, None, None, 4, 63, ptr(into), ptr(level), None) == bad
    assert L.rph_merge_tree_from_edges_host(None, 3, 4, 63, ptr(into), ptr(level), ptr(at)) == bad
    assert (into.tobytes(), level.tobytes(), at.tobytes()) == keep
    # malformed trees: every cutting call refuses them with nothing written
    good_into, good_level = np.array([0, 0, 1, 3], np.uint32), np.array([255, 9, 4, 255], np.uint8)
    trees = {"into above x": ([0, 2, 1, 3], [255, 9, 4, 255]), "self with a level": ([0, 1, 1, 3], [255, 9, 4, 255]),
             "joined without a level": ([0, 0, 1, 3], [255, 255, 4, 255]), "level falls along the chain": ([0, 0, 1, 3], [255, 4, 9, 255]),
             "level stays along the chain": ([0, 0, 1, 3], [255, 4, 4, 255])}
    labels, members, offsets, ng = np.full(4, 77, np.uint32), np.full(4, 77, np.uint32), np.full(4, 77, np.uint32), C.c_uint32(77)
    groups, grouped = np.full(64, 77, np.uint64), np.full(64, 77, np.uint64)
    assert L.rph_merge_tree_labels(ptr(good_into), ptr(good_level), 4, 9, ptr(labels)) == 0 and labels.tolist() == [0, 0, 0, 3]
    labels[:] = 77
    for name, (i, l) in trees.items():
        i, l = np.array(i, np.uint32), np.array(l, np.uint8)
        assert L.rph_merge_tree_labels(ptr(i), ptr(l), 4, 9, ptr(labels)) == bad, name
        assert L.rph_merge_tree_groups(ptr(i), ptr(l), 4, 9, ptr(members), ptr(offsets), C.byref(ng)) == bad, name
        assert L.rph_merge_tree_profile(ptr(i), ptr(l), 4, 63, ptr(groups), ptr(grouped)) == bad, name
    assert L.rph_merge_tree_profile(ptr(good_into), ptr(good_level), 4, 255, ptr(groups), ptr(grouped)) == bad
    assert L.rph_merge_tree_groups(ptr(good_into), ptr(good_level), 4, 9, None, ptr(offsets), C.byref(ng)) == bad
    assert {labels.min(), labels.max(), members.min(), members.max(), offsets.min(), offsets.max(), ng.value, int(groups.min()), int(groups.max()),
            int(grouped.min()), int(grouped.max())} == {77}


def test_a_plain_c_program_builds_and_cuts_a_tree():
    """the new block of include/rupphash.h is strict C99, and the host calls link and run without a device"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "tests", "c", "merge_tree_smoke")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "c", "merge_tree_smoke.c"),
                           "-o", exe, "-L", os.path.join(root, "rupphash_amd"), "-lrupphash_hip", "-Wl,-rpath," + os.path.join(root, "rupphash_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "merge tree ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
