"""CPU-side checks of the cross-set calls: the header declares them (ABI version still 1), the library exports them, and the host
half of rph_group_files_pdq_append -- rph_union_find_groups_append -- gives the oracle's groups and refuses malformed old groups."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCTIONS = ["rph_hamming_cross_pairs", "rph_hamming_cross_pairs_dev", "rph_hamming_variant_cross_pairs",
                 "rph_hamming_variant_cross_pairs_dev", "rph_group_files_pdq_append", "rph_union_find_groups_append"]
N_OLD, N_NEW = 700, 300


def clustered_hashes(rng, n, n_clusters, max_flip, members=4):
    hashes = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    for _ in range(n_clusters):
        base = rng.integers(0, 256, 32, dtype=np.uint8)
        for j in rng.choice(n, members, replace=False):
            v = base.copy()
            for b in rng.choice(256, rng.integers(0, max_flip + 1), replace=False):
                v[b // 8] ^= 1 << (b % 8)
            hashes[j] = v
    return hashes


@pytest.fixture(scope="module")
def host():
    """host-only entry points need no context"""
    from rupphash_amd import Engine, _lib

    eng = Engine.__new__(Engine)
    eng.L = _lib.load()
    eng.ctx = None
    return eng


@pytest.fixture(scope="module")
def case(oracle):
    """1000 clustered hashes; the groups of the first 700, and the edges and groups of all of them (computed once, read only)"""
    rng = np.random.default_rng(7003)
    hashes = clustered_hashes(rng, N_OLD + N_NEW, 60, 24, members=5)
    thr = 40
    _, old_groups = oracle.group_pdq(hashes[:N_OLD], thr)
    edges, groups = oracle.group_pdq(hashes, thr)
    return hashes, old_groups, edges, groups


def as_edges(pairs):
    from rupphash_amd import EDGE_DTYPE

    e = np.zeros(len(pairs), EDGE_DTYPE)
    for t, (i, j) in enumerate(pairs):
        e[t] = (i, j, 0, 0)
    return e


def test_header_declares_the_cross_calls_at_abi_version_1():
    src = open(os.path.join(ROOT, "include", "rupphash.h")).read()
    assert re.search(r"#define\s+RPH_ABI_VERSION\s+1\s", src)
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW_FUNCTIONS:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name


def test_cross_symbols_resolve_in_the_library():
    from rupphash_amd import _lib

    L = _lib.load()
    for name in NEW_FUNCTIONS:
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES
    assert L.rph_abi_version() == 1


def test_union_find_append_matches_oracle(host, case):
    _, old_groups, edges, groups = case
    assert len(old_groups) > 5 and any(max(g) >= N_OLD for g in groups) and any(min(g) >= N_OLD for g in groups)
    new_edges = [(int(i), int(j)) for i, j in edges if j >= N_OLD]
    assert 0 < len(new_edges) < len(edges)
    assert host.union_find_groups_append(old_groups, as_edges(new_edges), N_OLD + N_NEW) == groups


def test_union_find_append_without_old_groups_is_plain_union_find(host, case):
    _, _, edges, groups = case
    n = N_OLD + N_NEW
    assert host.union_find_groups_append([], as_edges([tuple(map(int, e)) for e in edges]), n) == groups
    empty = (np.zeros(0, np.uint32), np.zeros(0, np.uint32))  # null-sized arrays with n_old_groups = 0
    assert host.union_find_groups_append(empty, as_edges([(0, 1)]), n) == [[0, 1]]


def test_union_find_append_without_edges_returns_old_groups(host, case):
    _, old_groups, _, _ = case
    assert host.union_find_groups_append(old_groups, as_edges([]), N_OLD + N_NEW) == old_groups
    assert host.union_find_groups_append([], as_edges([]), 5) == []
    assert host.union_find_groups_append([], as_edges([]), 0) == []


def test_one_new_file_joins_two_old_groups(host):
    old = [[0, 3], [1, 4, 5], [2, 6]]
    got = host.union_find_groups_append(old, as_edges([(3, 8), (5, 8)]), 10)
    assert got == [[0, 1, 3, 4, 5, 8], [2, 6]]
    # a new file that joins a library file which had no group, and two new files that only join each other
    assert host.union_find_groups_append(old, as_edges([(7, 8), (8, 9)]), 10) == [[0, 3], [1, 4, 5], [2, 6], [7, 8, 9]]


@pytest.mark.parametrize("members, offsets", [
    ([0, 10], [0, 2]),            # member >= n_total
    ([0, 0xFFFFFFFF], [0, 2]),    # ... by a lot
    ([0, 1, 1], [0, 3]),          # a member twice in one group
    ([0, 1, 2, 1], [0, 2, 4]),    # a member in two groups
    ([0, 1, 2, 3], [0, 3, 2]),    # offsets descending
    ([0, 1, 2, 3], [1, 4]),       # offsets not starting at 0
    ([0, 1], [0, 2000000]),       # offsets far past anything the arrays hold
])
def test_malformed_old_groups_are_refused(host, members, offsets):
    from rupphash_amd import _lib

    om, oo = np.array(members, np.uint32), np.array(offsets, np.uint32)
    n = 10
    out_m, out_o = np.full(n + 8, 0xABABABAB, np.uint32), np.full(n // 2 + 2 + 8, 0xABABABAB, np.uint32)
    ng = C.c_uint32(77)
    rc = host.L.rph_union_find_groups_append(om.ctypes.data_as(C.c_void_p), oo.ctypes.data_as(C.c_void_p), len(offsets) - 1, None, 0, n,
                                             out_m.ctypes.data_as(C.c_void_p), out_o.ctypes.data_as(C.c_void_p), C.byref(ng))
    assert rc == _lib.RPH_ERR_INVALID_ARG
    assert (out_m[n:] == 0xABABABAB).all() and (out_o[n // 2 + 2:] == 0xABABABAB).all()  # nothing written past the capacities
    assert host.L.rph_last_error()
