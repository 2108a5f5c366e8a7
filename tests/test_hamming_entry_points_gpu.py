"""What the Hamming and grouping entry points promise around their sweeps (-m gpu), through the C ABI: the answers to degenerate sizes
and bad arguments and the order in which they are checked, the capacity protocol of every host and _dev form under the three
formulations of the fast path, and one round of every retry loop that grows an edge buffer.  The edge sets themselves are the business of
test_sweep_grid_gpu.py and test_cross_grid_gpu.py; expected counts here are numpy brute force (sweep_grid.py, cross_grid.py) or the CPU
oracle, never the library."""
import ctypes as C

import numpy as np
import pytest

import cross_grid as cg
import sweep_grid as sg

pytestmark = pytest.mark.gpu

KERNELS = (2, 1, 0)   # fp4 MFMA, int8 MFMA, VALU xor + popcount
FORMS = ("all_pairs", "variant_pairs", "cross_pairs", "variant_cross_pairs", "all_pairs64")
N = 1025              # two tiles
N_SAME = 1500         # identical hashes: 1 124 250 pairs, past the 2^20 edges every C retry loop starts with


@pytest.fixture(scope="module")
def eng():
    from rupphash_amd import Engine

    e = Engine(0)
    try:
        yield e
    finally:
        e.set_hamming_kernel(2)
        e.close()


def _p(a):
    return None if a is None else np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)


def _same256(n):
    return np.tile(np.random.default_rng(77).integers(0, 256, 32, dtype=np.uint8), (n, 1))


def _tuples(e):
    """(i, j, variant, d) of an edge list"""
    v = (e["flags"].astype(np.int64) >> sg.RPH_EDGE_VARIANT_SHIFT) & 7
    return set(zip(e["i"].tolist(), e["j"].tolist(), v.tolist(), e["d"].tolist()))


_CASES = {}


def case(form):
    """(host arrays in the order of the C arguments, truth: the (i, j, variant, d) a sweep must report) of one form on N planted hashes.
    Entries of the list: arrays are passed as pointers, integers as they are."""
    if form in _CASES:
        return _CASES[form]
    if form == "all_pairs":
        h = sg.sizes(N)
        args, truth = [h, N, 40], {(i, j, 0, d) for i, j, d in sg.brute256(h, 40).tolist()}
    elif form == "all_pairs64":
        h = sg.sizes(N, 64)
        args, truth = [h, N, 16], {(i, j, 0, d) for i, j, d in sg.brute64(h, 16).tolist()}
    elif form == "variant_pairs":
        h = sg.sizes(N)
        rng = np.random.default_rng(78)
        var = rng.integers(0, 256, (N, 8, 32), dtype=np.uint8)
        var[:, 0] = h
        for i, v, j, d in ((0, 3, 1024, 5), (10, 1, 11, 0), (512, 7, 1000, 40), (700, 2, 900, 41)):  # variant v of i near hash j
            var[i, v] = sg.flip(h[j], d, rng)
        low = (np.arange(N) % 7 == 3).astype(np.uint8)  # file 10 among them: its equal pair is still reported
        args, truth = [var, 8, h, low, N, 40], {(i, j, v, d) for i, j, v, d in sg.variant_brute(var, h, low, 40).tolist()}
        assert {(0, 1024, 3, 5), (10, 11, 1, 0), (512, 1000, 7, 40)} <= truth
    else:
        var, b = cg.sizes(N, N)
        if form == "cross_pairs":
            a = np.ascontiguousarray(var[:, :1])
            args, truth = [a, N, b, N, 40], {(i, j, v, d) for i, j, v, d in cg.brute(a, b, None, None, 40).tolist()}
        else:
            la, lb = (np.arange(N) % 7 == 3).astype(np.uint8), (np.arange(N) % 5 == 2).astype(np.uint8)
            args, truth = [var, 8, la, N, b, lb, N, 40], {(i, j, v, d) for i, j, v, d in cg.brute(var, b, la, lb, 40).tolist()}
    assert len(truth) >= 3
    _CASES[form] = (args, truth)
    return _CASES[form]


def host_call(eng, form, args, part, nparts, edges, cap):
    """(status, *n_edges_out) of the host form"""
    found = C.c_uint64(0xdead)
    fn = getattr(eng.L, "rph_hamming_" + form)
    rc = fn(eng.ctx, *[_p(a) if isinstance(a, np.ndarray) or a is None else a for a in args], part, nparts, _p(edges), cap, C.byref(found))
    return rc, found.value


class DevArgs:
    """the arrays of a case on the device, an edge buffer with `slack` records behind it and the counter"""

    def __init__(self, eng, args, room, slack=8):
        from rupphash_amd import EDGE_DTYPE

        self.eng, self.room, self.slack, self.item = eng, room, slack, EDGE_DTYPE.itemsize
        self.bufs, self.args = [], []
        for a in args:
            if isinstance(a, np.ndarray):
                a = np.ascontiguousarray(a)
                d = eng.dev_alloc(max(a.nbytes, 1))
                self.bufs.append(d)
                if a.nbytes:
                    eng.dev_upload(d, a)
                self.args.append(d)
            else:
                self.args.append(a)
        self.d_e = eng.dev_alloc((room + slack) * self.item)
        self.d_c = eng.dev_alloc(8)
        self.bufs += [self.d_e, self.d_c]

    def call(self, form, part, nparts, cap, null_edges=False, stream=None):
        """(status, the counter, the whole edge buffer with its slack) of the _dev form; the buffer is filled with 0xA5 first"""
        from rupphash_amd import EDGE_DTYPE

        eng = self.eng
        eng.dev_memset(self.d_e, 0xA5, (self.room + self.slack) * self.item)
        eng.dev_memset(self.d_c, 0, 8)
        eng.synchronize()
        fn = getattr(eng.L, f"rph_hamming_{form}_dev")
        rc = fn(eng.ctx, *self.args, part, nparts, None if null_edges else self.d_e, cap, self.d_c, stream)
        eng.synchronize()
        cnt = np.zeros(1, np.uint64)
        eng.dev_download(cnt, self.d_c)
        raw = np.zeros(self.room + self.slack, EDGE_DTYPE)
        eng.dev_download(raw, self.d_e)
        return rc, int(cnt[0]), raw

    def free(self):
        for d in self.bufs:
            self.eng.dev_free(d)


def untouched(raw):
    return (raw.view(np.uint8) == 0xA5).all()


# ------------------------------------------------------------------ capacity protocol
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("form", FORMS)
def test_capacity_protocol_host(eng, form, kernel):
    from rupphash_amd import EDGE_DTYPE, _lib

    args, truth = case(form)
    n_true = len(truth)
    eng.set_hamming_kernel(kernel)
    try:
        edges = np.zeros(n_true + 8, EDGE_DTYPE)
        rc, found = host_call(eng, form, args, 0, 1, edges, n_true)
        assert (rc, found) == (_lib.RPH_OK, n_true)
        assert _tuples(edges[:n_true]) == truth and not edges[n_true:].view(np.uint8).any()
        edges = np.zeros(n_true + 8, EDGE_DTYPE)
        rc, found = host_call(eng, form, args, 0, 1, edges, n_true - 1)
        assert (rc, found) == (_lib.RPH_ERR_CAPACITY, n_true)
        assert str(n_true).encode() in eng.L.rph_last_error()
        got = _tuples(edges[:n_true - 1])
        assert len(got) == n_true - 1 and got <= truth and not edges[n_true - 1:].view(np.uint8).any()
        rc, found = host_call(eng, form, args, 0, 1, None, 0)
        assert (rc, found) == (_lib.RPH_ERR_CAPACITY, n_true)
    finally:
        eng.set_hamming_kernel(2)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("form", FORMS)
def test_capacity_protocol_dev(eng, form, kernel):
    """a _dev form launches and returns: its status is RPH_OK whatever the sweep finds, the counter holds the full count, and no record
    past `cap` is written"""
    from rupphash_amd import _lib

    args, truth = case(form)
    n_true = len(truth)
    dev = DevArgs(eng, args, n_true)
    eng.set_hamming_kernel(kernel)
    try:
        rc, cnt, raw = dev.call(form, 0, 1, n_true)
        assert (rc, cnt) == (_lib.RPH_OK, n_true)
        assert _tuples(raw[:n_true]) == truth and untouched(raw[n_true:])
        rc, cnt, raw = dev.call(form, 0, 1, n_true - 1)
        assert (rc, cnt) == (_lib.RPH_OK, n_true)
        got = _tuples(raw[:n_true - 1])
        assert len(got) == n_true - 1 and got <= truth and untouched(raw[n_true - 1:])
        rc, cnt, raw = dev.call(form, 0, 1, 0, null_edges=True)
        assert (rc, cnt) == (_lib.RPH_OK, n_true) and untouched(raw)
    finally:
        eng.set_hamming_kernel(2)
        dev.free()


# ------------------------------------------------------------------ degenerate sizes and the order of the checks
def shrunk(form, n):
    """the arguments of case(form) cut down to n files per set"""
    args, _ = case(form)
    return [a[:n] if isinstance(a, np.ndarray) else (n if a == N else a) for a in args]


BAD_PARTS = ((5, 2), (1, 1), (0, 0))  # part >= nparts, nparts == 0


@pytest.mark.parametrize("form", ("all_pairs", "variant_pairs", "all_pairs64"))
def test_host_square_forms_answer_small_sets_before_they_look_at_the_parts(eng, form):
    from rupphash_amd import EDGE_DTYPE, _lib

    edges = np.zeros(4, EDGE_DTYPE)
    for n in (0, 1):
        for part, nparts in ((0, 1),) + BAD_PARTS:
            assert host_call(eng, form, shrunk(form, n), part, nparts, edges, 4) == (_lib.RPH_OK, 0), (n, part, nparts)
    for part, nparts in BAD_PARTS:  # from two files on the parts are checked
        assert host_call(eng, form, shrunk(form, 2), part, nparts, edges, 4) == (_lib.RPH_ERR_INVALID_ARG, 0), (part, nparts)
    if form == "variant_pairs":  # and so is the number of variants
        var3 = np.zeros((2, 3, 32), np.uint8)
        for n, want in ((0, _lib.RPH_OK), (1, _lib.RPH_OK), (2, _lib.RPH_ERR_INVALID_ARG)):
            assert host_call(eng, form, [var3[:n], 3, var3[:n, 0], None, n, 40], 0, 1, edges, 4) == (want, 0), n
    assert not edges.view(np.uint8).any()


@pytest.mark.parametrize("form", ("cross_pairs", "variant_cross_pairs"))
def test_host_cross_forms_check_their_arguments_before_they_look_at_the_sizes(eng, form):
    from rupphash_amd import EDGE_DTYPE, _lib

    edges = np.zeros(4, EDGE_DTYPE)
    args, _ = case(form)
    sizes = [k for k, a in enumerate(args) if not isinstance(a, np.ndarray) and a == N]
    for n_a, n_b in ((0, 0), (0, 5), (5, 0), (5, 5)):
        cut = list(args)
        cut[sizes[0]], cut[sizes[1]] = n_a, n_b
        for part, nparts in BAD_PARTS:
            assert host_call(eng, form, cut, part, nparts, edges, 4) == (_lib.RPH_ERR_INVALID_ARG, 0), (n_a, n_b, part, nparts)
        if form == "variant_cross_pairs":
            three = list(cut)
            three[1] = 3
            assert host_call(eng, form, three, 0, 1, edges, 4) == (_lib.RPH_ERR_INVALID_ARG, 0), (n_a, n_b)
        if n_a == 0 or n_b == 0:
            assert host_call(eng, form, cut, 0, 1, edges, 4) == (_lib.RPH_OK, 0), (n_a, n_b)
    assert not edges.view(np.uint8).any()


@pytest.mark.parametrize("form", FORMS)
def test_dev_forms_check_their_arguments_at_any_size(eng, form):
    from rupphash_amd import _lib

    args, _ = case(form)
    dev = DevArgs(eng, args, 4)
    sizes = [k for k, a in enumerate(args) if not isinstance(a, np.ndarray) and a == N]
    try:
        for n in (0, 1, 2, N):
            cut = list(dev.args)
            for k in sizes:
                cut[k] = n
            full, dev.args = dev.args, cut
            try:
                for part, nparts in BAD_PARTS:
                    rc, cnt, raw = dev.call(form, part, nparts, 4)
                    assert (rc, cnt) == (_lib.RPH_ERR_INVALID_ARG, 0) and untouched(raw), (n, part, nparts)
                if form in ("variant_pairs", "variant_cross_pairs"):
                    dev.args = list(cut)
                    dev.args[1] = 3
                    rc, cnt, raw = dev.call(form, 0, 1, 4)
                    assert (rc, cnt) == (_lib.RPH_ERR_INVALID_ARG, 0) and untouched(raw), n
                    dev.args = cut
                if n < 2:  # no pair, but for the one of a cross sweep of one file against one: cross_grid.sizes plants a[0] == b[0]
                    rc, cnt, raw = dev.call(form, 0, 1, 4)
                    want = 1 if n == 1 and "cross" in form else 0
                    assert (rc, cnt) == (_lib.RPH_OK, want), n
            finally:
                dev.args = full
    finally:
        dev.free()


def test_grouping_calls_refuse_a_similarity_above_the_maximum(eng):
    from rupphash_amd import _lib

    h = _same256(4)
    m, o, ng = np.zeros(8, np.uint32), np.zeros(8, np.uint32), C.c_uint32(9)
    old_m, old_o = np.array([0, 1], np.uint32), np.array([0, 2], np.uint32)
    for n in (0, 4):
        assert eng.L.rph_group_files_pdq(eng.ctx, _p(h), None, None, None, n, 64, _p(m), _p(o), C.byref(ng), None) == _lib.RPH_ERR_INVALID_ARG
        assert eng.L.rph_group_files_pdq_append(eng.ctx, _p(h), None, None, None, 2, _p(old_m), _p(old_o), 1, _p(h), None, None, None, n, 64, _p(m),
                                                _p(o), C.byref(ng), None) == _lib.RPH_ERR_INVALID_ARG
    assert ng.value == 9 and not m.any() and not o.any()
    assert eng.group_files_pdq(h, 63) == ([[0, 1, 2, 3]], 6)


# ------------------------------------------------------------------ growth paths: one round of every retry loop
def test_growth_find_groups(eng, oracle):
    h = _same256(N_SAME)
    assert eng.find_groups256(h, 32) == oracle.find_groups(oracle.KIND_PDQ, h, 32)
    h64 = np.full(N_SAME, 0x0123456789ABCDEF, np.uint64)
    assert eng.find_groups64(h64, 8) == oracle.find_groups(oracle.KIND_U64, h64, 8)


def test_growth_group_files_pdq_and_append(eng, oracle):
    n_old = 100
    h = _same256(n_old + N_SAME)
    ref_edges, ref_groups = oracle.group_pdq(h[n_old:], 31)
    assert len(ref_edges) == N_SAME * (N_SAME - 1) // 2 > 1 << 20
    assert eng.group_files_pdq(h[n_old:], 31) == (ref_groups, len(ref_edges))
    old_edges, old_groups = oracle.group_pdq(h[:n_old], 31)
    all_edges, all_groups = oracle.group_pdq(h, 31)
    assert len(all_edges) - len(old_edges) == n_old * N_SAME + N_SAME * (N_SAME - 1) // 2
    assert eng.group_files_pdq_append(h[:n_old], old_groups, h[n_old:], 31) == (all_groups, len(all_edges) - len(old_edges))


def pair_keys(i, j):
    return np.sort(np.asarray(i, np.int64) * 4096 + np.asarray(j, np.int64))


def check_equal_pairs(e, want, what):
    """the edge list holds exactly the pairs `want` (pair_keys), all at distance 0"""
    assert len(e) == len(want) and not e["d"].any() and np.array_equal(pair_keys(e["i"], e["j"]), want), what


def test_growth_python_wrappers(eng):
    """cap=None: the wrappers start at 65 536 edges and come back with all of them"""
    h = _same256(N_SAME)
    square = pair_keys(*np.triu_indices(N_SAME, k=1))
    assert len(square) == N_SAME * (N_SAME - 1) // 2
    check_equal_pairs(eng.hamming_all_pairs(h, 10), square, "hamming_all_pairs")
    check_equal_pairs(eng.hamming_all_pairs64(np.full(N_SAME, 0x0123456789ABCDEF, np.uint64), 4), square, "hamming_all_pairs64")
    check_equal_pairs(eng.hamming_variant_pairs(h.reshape(N_SAME, 1, 32), h, 10), square, "hamming_variant_pairs")
    rect = pair_keys(np.repeat(np.arange(70), 1000), np.tile(np.arange(1000), 70))  # 70 000 pairs
    check_equal_pairs(eng.hamming_cross_pairs(h[:70], h[:1000], 10), rect, "hamming_cross_pairs")
    low = np.zeros(1000, np.uint8)
    check_equal_pairs(eng.hamming_variant_cross_pairs(h[:70].reshape(70, 1, 32), h[:1000], 10, low_conf_b=low), rect, "hamming_variant_cross_pairs")


def test_sets_that_alias_on_the_host(eng):
    """Rows and columns given as overlapping views of ONE host array: each side is what its own pointer and count say.  A set against a
    prefix of itself in both orders, 8 variants whose array is also the array of the hashes, and the variant form with one variant and
    variants == hashes (which the parent ran as rows of their own, so never on the popcount-sorted path: kernel 4 would take it)."""
    h = _same256(1000)
    tall = pair_keys(np.repeat(np.arange(1000), 70), np.tile(np.arange(70), 1000))
    wide = pair_keys(np.repeat(np.arange(70), 1000), np.tile(np.arange(1000), 70))
    square = pair_keys(*np.triu_indices(125, k=1))
    for kernel in KERNELS + (4,):
        eng.set_hamming_kernel(kernel)
        try:
            check_equal_pairs(eng.hamming_cross_pairs(h[:1000], h[:70], 10, cap=80000), tall, f"1000 x its first 70, kernel {kernel}")
            check_equal_pairs(eng.hamming_cross_pairs(h[:70], h[:1000], 10, cap=80000), wide, f"70 x the set they begin, kernel {kernel}")
            low = np.zeros(70, np.uint8)
            check_equal_pairs(eng.hamming_variant_cross_pairs(h[:1000].reshape(1000, 1, 32), h[:70], 10, low_conf_b=low, cap=80000), tall,
                              f"variant form, 1000 x its first 70, kernel {kernel}")
            # 125 files x 8 variants = the 1000 hashes; the files' own hashes are the first 125 of the same array
            e = eng.hamming_variant_cross_pairs(h.reshape(125, 8, 32), h[:70], 10, cap=80000)
            assert len(e) == 125 * 8 * 70 and not e["d"].any(), kernel
            e = eng.hamming_variant_pairs(h.reshape(125, 8, 32), h[:125], 10, cap=80000)
            assert len(e) == 8 * len(square) and not e["d"].any() and (e["i"] < e["j"]).all() and e["j"].max() == 124, kernel
            check_equal_pairs(eng.hamming_variant_pairs(h[:125].reshape(125, 1, 32), h[:125], 10, cap=80000), square,
                              f"one variant, variants == hashes, kernel {kernel}")
        finally:
            eng.set_hamming_kernel(2)


def test_growth_multi_two_ranks_on_one_device():
    from rupphash_amd import MultiEngine

    m = MultiEngine(devices=[0, 0])
    try:
        e = m.hamming_all_pairs(_same256(N_SAME), 10)
    finally:
        m.close()
    check_equal_pairs(e, pair_keys(*np.triu_indices(N_SAME, k=1)), "rph_multi_hamming_all_pairs")
