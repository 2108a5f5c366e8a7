"""rph_library_remove without a GPU: the header declares it and _lib binds it; the numpy model of removal that the GPU tests rely on
(drop the removed files' edges, renumber, min-label union-find) equals the CPU oracle's grouping of the survivors on the library corpus;
and the closed forms of the dense and the blocks-of-four libraries are what the model gives."""
import os
import re

import numpy as np
import pytest

import library_corpus as lc
import removal_corpus as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_remove_and_lib_binds_it():
    from rupphash_amd import _lib

    header = open(os.path.join(ROOT, "include", "rupphash.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"^#define RPH_ABI_VERSION 1$", header, flags=re.M)  # additive: the version stays
    found = re.search(r"\bint rph_library_remove\s*\((.*?)\)\s*;", code, flags=re.S)
    assert found, "include/rupphash.h does not declare rph_library_remove"
    params = [p.strip() for p in found.group(1).split(",")]
    assert [p.split("*")[0].strip() for p in params] == ["rph_library", "const uint32_t", "uint64_t n_remove", "uint32_t", "uint64_t"]
    assert "rph_library_remove" in _lib.SIGNATURES and len(_lib.SIGNATURES["rph_library_remove"][1]) == len(params)
    assert "rph_debug_library_remove_stats" in _lib.DEBUG_SIGNATURES and "rph_debug_library_remove_stats" not in code  # a debug hook, not ABI
    L = _lib.load()
    assert hasattr(L, "rph_library_remove") and hasattr(L, "rph_debug_library_remove_stats")
    assert "cannot be removed" not in header
    from rupphash_amd import scanner
    from rupphash_amd.engine import Library

    assert callable(Library.remove) and callable(scanner.ScannerLibrary.remove)


def test_new_index_is_the_old_index_minus_the_removed_files_below_it():
    new = rc.new_index(10, [7, 0, 3])
    assert new.tolist() == [rc.GONE, 0, 1, rc.GONE, 2, 3, 4, rc.GONE, 5, 6]
    assert rc.new_index(4, []).tolist() == [0, 1, 2, 3] and rc.new_index(3, [2, 1, 0]).tolist() == [rc.GONE] * 3


def test_the_model_splits_a_bridged_component_and_moves_a_root():
    # 0-1-2 and 4-5 joined through 6; 3 alone; (0, 1) reported twice
    edges = np.array([(0, 1), (0, 1), (1, 2), (4, 5), (2, 6), (5, 6)], np.uint32)
    assert lc.groups_of(lc.min_labels(7, edges)) == [[0, 1, 2, 4, 5, 6]]
    new, kept, dropped, labels, groups = rc.remove_from_edges(7, edges, [6])
    assert dropped == 2 and groups == [[0, 1, 2], [4, 5]] and labels.tolist() == [0, 0, 0, 3, 4, 4]
    new, kept, dropped, labels, groups = rc.remove_from_edges(7, edges, [0, 3])  # the root goes: the label moves to the next member
    assert dropped == 2 and new.tolist() == [rc.GONE, 0, 1, rc.GONE, 2, 3, 4] and groups == [[0, 1, 2, 3, 4]] and (labels == 0).all()
    new, kept, dropped, labels, groups = rc.remove_from_edges(7, edges, [1])  # 0 is cut off
    assert dropped == 3 and groups == [[1, 3, 4, 5]] and labels.tolist() == [0, 1, 2, 1, 1, 1]


@pytest.fixture(scope="module")
def files(oracle):
    return lc.corpus()


def by_oracle(oracle, f, sim, ids):
    return oracle.group_pdq(f.hashes[ids], sim, variants=f.dih[ids], has_features=f.has_features[ids], quality=f.quality[ids])


def removal_sets():
    b = lc.BRIDGE
    rng = np.random.default_rng(515)
    yield "the-bridge", [b["c"]]
    yield "two-roots", [0, 3]
    yield "one-of-each-bridged-pair", [b["a"], b["b2"]]
    for share in (0.1, 0.5, 0.9):
        yield f"random-{share}", rng.choice(lc.N_FILES, int(share * lc.N_FILES), replace=False).tolist()
    yield "all-but-one", [x for x in range(lc.N_FILES) if x != 1]
    yield "everything", list(range(lc.N_FILES))
    yield "nothing", []


@pytest.mark.parametrize("sim", (16, 40))
@pytest.mark.parametrize("name,removed", list(removal_sets()), ids=[n for n, _ in removal_sets()])
def test_the_model_equals_the_oracle_on_the_survivors(oracle, files, sim, name, removed):
    """what the GPU tests expect of a removal is what the reference's grouping gives on the files that stay"""
    everything = np.arange(lc.N_FILES)
    edges, groups = by_oracle(oracle, files, sim, everything)
    assert lc.groups_of(lc.min_labels(lc.N_FILES, edges)) == groups
    new, kept, dropped, labels, model_groups = rc.remove_from_edges(lc.N_FILES, edges, removed)
    survivors = everything[new != rc.GONE]
    assert len(survivors) == lc.N_FILES - len(removed) and np.array_equal(new[survivors], np.arange(len(survivors)))
    if len(survivors) == 0:
        assert dropped == len(edges) and model_groups == []
        return
    ref_edges, ref_groups = by_oracle(oracle, files, sim, survivors)
    assert model_groups == ref_groups
    assert len(kept) == len(ref_edges) == len(edges) - dropped
    assert sorted(map(tuple, kept.tolist())) == sorted(map(tuple, ref_edges.tolist()))  # the same edges, as often
    if name == "the-bridge" and sim == 40:
        b = lc.BRIDGE
        assert [b["a"], b["a2"]] in model_groups and [b["b"], b["b2"]] in model_groups
        assert dropped == 4  # C is 30 bits from A and B and 35 from A' and B'
    if name == "two-roots" and sim == 40:
        before = {tuple(g) for g in groups}
        assert (0, 1) in before and (3, 1500) in before  # two pairs: both dissolve
        assert labels[new[1]] == new[1] and labels[new[1500]] == new[1500]


def test_dense_closed_forms(oracle):
    for c, rows in ((5, 1), (40, 1), (7, 8)):
        hashes = np.zeros((c, 32), np.uint8)
        variants = np.repeat(hashes[:, None, :], 8, axis=1)
        hf = np.full(c, 1 if rows == 8 else 0, np.uint8)
        edges, _ = oracle.group_pdq(hashes, 31, variants=variants, has_features=hf)
        assert len(edges) == rows * c * (c - 1) // 2
        _, kept, dropped, labels, groups = rc.remove_from_edges(c, edges, [c // 2])
        assert (dropped, len(kept)) == rc.dense_minus_one(c, rows) and groups == [list(range(c - 1))]
    assert rc.dense_minus_one(1500) == (1499, 1499 * 1498 // 2) and rc.dense_minus_one(700, 8) == (8 * 699, 8 * 699 * 698 // 2)
    # the regroup of 1500 (and of 700 eight-row) identical files, the removed one included, runs over the first edge capacity
    assert 1500 * 1499 // 2 > max(1 << 20, 32 * 1500) and 8 * 700 * 699 // 2 > max(1 << 20, 32 * 700)
    hashes, common = lc.dense_hashes(1500)
    victim = int(np.nonzero(common)[0][700])
    stay = np.ones(len(common), bool)
    stay[victim] = False
    labels, groups, cmp_count = lc.dense_expectation(common[stay])
    assert cmp_count == rc.dense_minus_one(1500)[1] and len(groups[0]) == 1499 and labels[victim] == 0  # (the next common file took the number)


@pytest.mark.parametrize("n", (1, 4, 9, 1101, 2049))
def test_blocks_of_four_closed_form(oracle, n):
    hashes = rc.block_hashes(n, 5)
    edges, groups = oracle.group_pdq(hashes, rc.BLOCK_SIM)
    want = {(x, y) for x in range(n) for y in range(x + 1, min(n, (x // 4 + 1) * 4))}
    assert {tuple(e) for e in edges.tolist()} == want and len(edges) == len(want)  # exactly the pairs inside a block, once each
    labels, restore_groups, cmp_count = rc.block_state(np.ones(n, bool))
    assert cmp_count == len(edges) and rc.groups_as_lists(restore_groups) == groups and np.array_equal(labels, lc.min_labels(n, edges))
    removed = rc.grid_removals(n)
    assert removed[0] == 0 and removed[-1] == n - 1 and (n < 3 or 1 in removed)
    new, kept, dropped, model_labels, model_groups = rc.remove_from_edges(n, edges, removed)
    labels, after_groups, cmp_count = rc.block_state(new != rc.GONE)
    assert np.array_equal(labels, model_labels) and rc.groups_as_lists(after_groups) == model_groups and cmp_count == len(kept)
    if n >= 1101:
        assert [0, 1] in model_groups  # block 0 lost its first two members: files 2 and 3 are the group now
        assert sum(len(g) == 3 for g in model_groups) >= 1  # a block with one member gone stays one group of three
