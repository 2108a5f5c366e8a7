"""The device union-find and the component export (-m gpu): rph_union_find_labels_dev against the numpy min-labels that
test_library_cpu.py pins, rph_groups_from_labels_dev against the host rph_union_find_groups, on the context's stream and on a caller's."""
import ctypes as C

import numpy as np
import pytest

import library_corpus as lc

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


def as_edges(pairs):
    from rupphash_amd import EDGE_DTYPE

    e = np.zeros(len(pairs), EDGE_DTYPE)
    e["i"], e["j"] = pairs[:, 0], pairs[:, 1]
    e["d"], e["flags"] = 7, 0x0E00  # what the union must not look at
    return e


@pytest.mark.parametrize("own_stream", [False, True], ids=["context-stream", "caller-stream"])
@pytest.mark.parametrize("case", list(lc.edge_lists()), ids=lambda c: c.name)
def test_labels_and_groups_match_numpy_and_the_host_union_find(eng, caller_stream, case, own_stream):
    st = caller_stream if own_stream else None
    g = lc.global_edges(case)
    want = lc.min_labels(case.n, g)
    start = np.arange(case.n, dtype=np.uint32) if case.labels is None else case.labels
    with DeviceArray(eng, start) as d_labels:
        for pairs, i_base, j_base in case.calls:
            with DeviceArray(eng, as_edges(pairs)) as d_edges:
                eng.union_find_labels_dev(d_edges.ptr if len(pairs) else None, len(pairs), d_labels.ptr, case.n, i_base, j_base, stream=st)
                eng.stream_synchronize(st)
        got = d_labels.download(np.uint32)
        assert np.array_equal(got, want)
        groups = eng.groups_from_labels_dev(d_labels.ptr, case.n, stream=st)
    assert groups == eng.union_find_groups(as_edges(g), case.n) == lc.groups_of(want)


@pytest.fixture(scope="module")
def grid(eng):
    """G: the lanes of the largest launch grid_for() makes, one pass of every grid-stride loop"""
    return 8 * eng.device_info()[1] * 256


@pytest.mark.parametrize("name", lc.LARGE_CASES)
def test_labels_beyond_one_grid_match_the_closed_form(eng, grid, name):
    case = lc.large_case(grid, name)
    assert case.n > grid or case.n in (2000, 4097)
    if name.startswith("clique"):
        assert len(case.calls[0][0]) == 1124250 > 8 * 256 * 256  # more than one pass on a part of 256 CUs
    start = np.arange(case.n, dtype=np.uint32) if case.labels is None else case.labels
    with DeviceArray(eng, start) as d_labels:
        for pairs, i_base, j_base in case.calls:
            with DeviceArray(eng, as_edges(pairs)) as d_edges:
                eng.union_find_labels_dev(d_edges.ptr if len(pairs) else None, len(pairs), d_labels.ptr, case.n, i_base, j_base)
                eng.synchronize()
        got = d_labels.download(np.uint32)
        assert np.array_equal(got, case.want)
        groups = eng.groups_from_labels_dev(d_labels.ptr, case.n)
    assert groups == lc.groups_of(case.want)


@pytest.mark.parametrize("which", [0, 1], ids=["G+77", "2G+1"])
@pytest.mark.parametrize("family", [0, 1, 2, 3], ids=["singletons", "one-component", "pairs", "interleaved"])
def test_export_beyond_one_grid(eng, grid, family, which):
    n = lc.grid_sizes(grid)[which]
    name, labels = list(lc.label_families(n))[family]
    with DeviceArray(eng, labels) as d_labels:
        assert eng.groups_from_labels_dev(d_labels.ptr, n) == lc.groups_of(labels), name


def test_refusals_beyond_the_first_pass(eng, grid):
    from rupphash_amd import RphError, _lib

    # a bad edge at index G + 5: the range check's second pass finds it, nothing is written
    n = grid + 77
    edges, _ = lc.blocks_of_four(n)
    assert len(edges) > grid + 5
    edges[grid + 5] = (7, n)
    start = np.arange(n, dtype=np.uint32)
    with DeviceArray(eng, start) as d_labels, DeviceArray(eng, as_edges(edges)) as d_edges:
        with pytest.raises(RphError) as err:
            eng.union_find_labels_dev(d_edges.ptr, len(edges), d_labels.ptr, n)
        assert err.value.status == _lib.RPH_ERR_INVALID_ARG
        eng.synchronize()
        assert np.array_equal(d_labels.download(np.uint32), start)
    # a label outside n at the last index of a large array: the export refuses, the outputs are untouched
    for n in lc.grid_sizes(grid):
        labels = np.arange(n, dtype=np.uint32) & ~np.uint32(1)
        labels[n - 1] = 0xFFFFFFFF
        with DeviceArray(eng, labels) as d_labels:
            members, offsets = np.full(n, 77, np.uint32), np.full(n // 2 + 2, 77, np.uint32)
            ng = C.c_uint32(77)
            rc = eng.L.rph_groups_from_labels_dev(eng.ctx, d_labels.ptr, n, members.ctypes.data_as(C.c_void_p), offsets.ctypes.data_as(C.c_void_p),
                                                  C.byref(ng), None)
            assert rc == _lib.RPH_ERR_INVALID_ARG and ng.value == 0 and (members == 77).all()


def test_an_edge_outside_n_is_refused_and_nothing_is_written(eng):
    from rupphash_amd import RphError, _lib

    n = 300
    rng = np.random.default_rng(5)
    pairs = np.stack([rng.integers(0, n, 500), rng.integers(0, n, 500)], axis=1).astype(np.uint32)
    start = np.arange(n, dtype=np.uint32)
    start[[10, 11]] = 9
    for bad, i_base, j_base in (((7, n), 0, 0), ((n, 7), 0, 0), ((7, n - 5), 0, 5), ((n - 5, 7), 5, 0), ((0xFFFFFFFF, 0), 1, 0)):
        e = np.minimum(pairs, n - 6)  # the good edges stay inside n under the bases
        e[333] = bad
        with DeviceArray(eng, start) as d_labels, DeviceArray(eng, as_edges(e)) as d_edges:
            with pytest.raises(RphError) as err:
                eng.union_find_labels_dev(d_edges.ptr, len(e), d_labels.ptr, n, i_base, j_base)
            assert err.value.status == _lib.RPH_ERR_INVALID_ARG
            eng.synchronize()
            assert np.array_equal(d_labels.download(np.uint32), start)
    # a label above its file would send the walk out of the array: refused the same way
    up = start.copy()
    up[20] = 4000
    with DeviceArray(eng, up) as d_labels, DeviceArray(eng, as_edges(np.minimum(pairs, n - 1))) as d_edges:
        with pytest.raises(RphError) as err:
            eng.union_find_labels_dev(d_edges.ptr, len(pairs), d_labels.ptr, n)
        assert err.value.status == _lib.RPH_ERR_INVALID_ARG
        assert np.array_equal(d_labels.download(np.uint32), up)


@pytest.mark.parametrize("own_stream", [False, True], ids=["context-stream", "caller-stream"])
def test_export_of_every_label_case(eng, caller_stream, own_stream):
    for name, labels in lc.label_cases():
        with DeviceArray(eng, labels) as d_labels:
            assert eng.groups_from_labels_dev(d_labels.ptr, len(labels), stream=caller_stream if own_stream else None) == lc.groups_of(labels), name


def test_export_refuses_labels_that_are_not_flattened(eng):
    from rupphash_amd import RphError, _lib

    big = np.arange(5000, dtype=np.uint32)
    big[4321] = 0xFFFFFFFF  # far outside every array of the export: refused without being used as an index
    small = np.arange(300, dtype=np.uint32)
    small[299] = 0xFFFFFFF0
    cases = [np.array([0, 0, 1, 3], np.uint32), np.array([0, 1, 9, 3], np.uint32), np.array([1, 1, 2, 3], np.uint32), big, small,
             np.array([0, 0xFFFFFFFF], np.uint32), np.array([7], np.uint32)]
    for labels in cases:
        with DeviceArray(eng, labels) as d_labels:
            members, offsets = np.full(len(labels), 77, np.uint32), np.full(len(labels) // 2 + 2, 77, np.uint32)
            ng = C.c_uint32(77)
            rc = eng.L.rph_groups_from_labels_dev(eng.ctx, d_labels.ptr, len(labels), members.ctypes.data_as(C.c_void_p), offsets.ctypes.data_as(C.c_void_p),
                                                  C.byref(ng), None)
            assert rc == _lib.RPH_ERR_INVALID_ARG and ng.value == 0 and (members == 77).all()
            with pytest.raises(RphError) as err:
                eng.groups_from_labels_dev(d_labels.ptr, len(labels))
            assert err.value.status == _lib.RPH_ERR_INVALID_ARG
    with DeviceArray(eng, np.arange(5000, dtype=np.uint32)) as d_labels:  # the engine still works
        assert eng.groups_from_labels_dev(d_labels.ptr, 5000) == []
