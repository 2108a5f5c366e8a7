"""The resident library without a GPU: the header declares its calls at ABI version 1 and _lib binds them; the corpus of
library_corpus.py has the properties the GPU tests rely on; and the numpy min-label union-find that those tests compare the device
labels with lists the same groups as the host rph_union_find_groups."""
import os
import re

import numpy as np
import pytest

import library_corpus as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_CALLS = ["rph_union_find_labels_dev", "rph_groups_from_labels_dev", "rph_library_create", "rph_library_destroy", "rph_library_reserve",
             "rph_library_size", "rph_library_append", "rph_library_restore", "rph_library_groups", "rph_library_labels", "rph_library_query"]


def test_header_declares_the_calls_and_lib_binds_them():
    from rupphash_amd import _lib

    header = open(os.path.join(ROOT, "include", "rupphash.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"^#define RPH_ABI_VERSION 1$", header, flags=re.M)  # additive: the version stays
    assert "typedef struct rph_library rph_library;" in code
    L = _lib.load()
    for name in NEW_CALLS:
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    # arity as the header states it
    for name in NEW_CALLS:
        params = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1).split(",")
        assert len(params) == len(_lib.SIGNATURES[name][1]), name
    from rupphash_amd import Engine, scanner
    from rupphash_amd.engine import Library

    for method in ("append", "restore", "groups", "labels", "query", "reserve", "close", "__len__", "__enter__", "__exit__"):
        assert callable(getattr(Library, method))
    assert isinstance(Library.comparisons, property)
    assert callable(Engine.library) and callable(Engine.union_find_labels_dev) and callable(Engine.groups_from_labels_dev)
    assert callable(scanner.open_library)


def host_engine():
    from rupphash_amd import Engine, _lib

    eng = Engine.__new__(Engine)  # host-only entry points need no context
    eng.L = _lib.load()
    eng.ctx = None
    return eng


@pytest.mark.parametrize("case", list(lc.edge_lists()), ids=lambda c: c.name)
def test_numpy_min_labels_list_the_groups_of_the_host_union_find(case):
    from rupphash_amd import EDGE_DTYPE

    g = lc.global_edges(case)
    labels = lc.min_labels(case.n, g)
    assert (labels <= np.arange(case.n)).all() and (labels[labels] == labels).all()  # flattened, root = smallest member
    edges = np.zeros(len(g), EDGE_DTYPE)
    edges["i"], edges["j"] = g[:, 0], g[:, 1]
    assert lc.groups_of(labels) == host_engine().union_find_groups(edges, case.n)


def test_edge_lists_cover_what_the_union_kernel_can_get_wrong():
    cases = {c.name: c for c in lc.edge_lists()}
    assert len(cases) == len(list(lc.edge_lists())) >= 14
    asc = cases["path-65-ascending"].calls[0][0]
    assert (asc[:, 1] == asc[:, 0] + 1).all() and len(asc) == 64  # one wave, every lane hooks its neighbour
    assert (cases["star-hub-last"].calls[0][0][:, 1] == 1999).all() and (cases["star-hub-first"].calls[0][0][:, 0] == 0).all()
    assert len(lc.groups_of(lc.min_labels(4097, lc.global_edges(cases["path-4097-shuffled"])))[0]) == 4097
    forest = cases["forest-plus-one-node"]
    assert len(lc.groups_of(forest.labels)) == 3 and lc.groups_of(lc.min_labels(41, lc.global_edges(forest))) == [[4, 5, 6, 7, 11, 20, 21, 30, 39, 40]]
    two = cases["two-calls-with-bases"]
    assert [(ib, jb) for _, ib, jb in two.calls] == [(0, 700), (700, 700)]
    assert any(len(c.calls[0][0]) == 0 for c in cases.values()) and cases["n-1"].n == 1


def test_label_cases_are_flattened_min_labels():
    seen = set()
    for name, labels in lc.label_cases():
        n = len(labels)
        seen.add(n)
        assert (labels <= np.arange(n)).all() and (labels[labels] == labels).all(), name
        groups = lc.groups_of(labels)
        if name.startswith("interleaved") and n >= 4:
            assert groups[0] == [0, n // 2] and groups[1] == [1, n // 2 + 1]
        if name.startswith("singletons"):
            assert groups == []
    assert seen == {1, 2, 255, 256, 257, 4099}


@pytest.mark.parametrize("case", list(lc.large_edge_lists(4 * 256)), ids=lambda c: c.name)
def test_closed_form_labels_of_the_large_cases_are_the_min_labels(case):
    assert lc.grid_sizes(1024) == (4 * 256 + 77, 2049)
    g = lc.global_edges(case)
    assert len(g) and (g < case.n).all()
    assert case.want.dtype == np.uint32 and np.array_equal(case.want, lc.min_labels(case.n, g))
    for edges, i_base, j_base in case.calls:  # what the device's range check demands of every call
        assert edges.dtype == np.uint32 and ((edges[:, 0].astype(np.int64) + i_base < case.n) & (edges[:, 1].astype(np.int64) + j_base < case.n)).all()
    if "two-calls" in case.name:
        assert all(len(e) >= 48 for e, _, _ in case.calls) and case.calls[1][1:] == (case.n // 2, case.n // 2)
    if case.name.startswith("star-forest") and "8-times" not in case.name:
        e = g[g[:, 0] != g[:, 1]]
        hub_is_j = (e[:, 1] % 1000 == 0).mean()
        assert 0.4 < hub_is_j < 0.6 and len(e) == case.n - (case.n + 999) // 1000
    if case.name.startswith("clique"):
        assert len(case.calls[0][0]) == 1500 * 1499 // 2 == 1124250
    if case.name.startswith("chain"):
        assert (case.labels <= np.arange(case.n)).all() and (case.labels[case.labels] != case.labels)[2:].all()  # legal, not flattened


def test_label_families_and_dense_sets(oracle):
    for n in lc.grid_sizes(1024):
        for name, labels in lc.label_families(n):
            assert (labels <= np.arange(n)).all() and (labels[labels] == labels).all(), name
    hashes, common = lc.dense_hashes(1500)
    assert len(hashes) == 1500 + 37 and common.sum() == 1500 and not common[40] and common[41]
    others = hashes[~common]
    for k, h in enumerate(others):  # the unrelated hashes are more than 63 bits from the common one and from each other
        assert oracle.hamming256(h, hashes[0]) > 63
        assert all(oracle.hamming256(h, o) > 63 for o in others[:k])
    labels, groups, cmp_count = lc.dense_expectation(common)
    edges, ref_groups = oracle.group_pdq(hashes[:300], 31)
    want = lc.dense_expectation(common[:300])
    assert (ref_groups, len(edges)) == want[1:] and np.array_equal(want[0], lc.min_labels(300, edges))
    assert cmp_count == 1124250 and groups[0][:41] == list(range(40)) + [41]


@pytest.fixture(scope="module")
def files(oracle):
    return lc.corpus()


def grouped(oracle, f, sim, stop=lc.N_FILES, has_features=None):
    hf = f.has_features if has_features is None else has_features
    return oracle.group_pdq(f.hashes[:stop], sim, variants=f.dih[:stop], has_features=hf[:stop], quality=f.quality[:stop])[1]


def test_the_bridge_merges_two_groups_at_40_and_not_at_16(oracle, files):
    b = lc.BRIDGE
    assert b["c"] == lc.N_FILES - 1
    d = lambda x, y: oracle.hamming256(files.hashes[b[x]], files.hashes[b[y]])  # noqa: E731
    assert (d("a", "c"), d("b", "c"), d("a", "b"), d("a", "a2"), d("b", "b2")) == (30, 30, 60, 5, 5)
    without, with_c = grouped(oracle, files, 40, lc.N_FILES - 1), grouped(oracle, files, 40)
    assert len(with_c) == len(without) - 1
    assert [b["a"], b["a2"]] in without and [b["b"], b["b2"]] in without
    assert [b["a"], b["a2"], b["b"], b["b2"], b["c"]] in with_c
    assert len(grouped(oracle, files, 16)) == len(grouped(oracle, files, 16, lc.N_FILES - 1))


def test_every_split_has_an_append_that_joins_old_and_new_files(oracle, files):
    assert lc.SPLITS == [[1901], [1, 1900], [1500, 1, 400], [0, 900, 0, 1001], [1023, 1, 1, 876], [100] * 19 + [1]]
    for split in lc.SPLITS:
        spans = [first for first, last in lc.batches(split)
                 if 0 < first < last and any(g[0] < first <= g[-1] for g in grouped(oracle, files, 40, last))]
        assert spans or len(split) == 1, split  # (one batch of everything has no old files to join)
        if split[-1] == 1 and len(split) > 1:  # the last file alone is the bridge: its append merges two old groups
            assert spans[-1] == lc.N_FILES - 1


def test_featureless_files_sit_inside_groups(oracle, files):
    assert 0.05 < (files.has_features == 0).mean() < 0.2
    in_groups = {m for g in grouped(oracle, files, 40) for m in g}
    assert sum(1 for m in in_groups if files.has_features[m] == 0) >= 5
    assert (files.quality < 0).any() and ((files.quality >= 0) & (files.quality < 50)).any()
