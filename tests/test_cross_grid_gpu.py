"""The cross-set Hamming sweeps on the grids of cross_grid.py, under every kernel setting.  Every expected value is the numpy brute force
plus the restated probe key (both pinned against the C oracle in test_cross_grid_cpu.py); no kernel is compared with another one and
there is no tolerance.  An edge list is compared as its sorted (i, j, d, flags) tuples, packed into one integer each; a difference names
the first tuples that are missing and that are extra or reported twice, from which the block, wave, pass, row block, lane and chunk
follow."""
import numpy as np
import pytest

import cross_grid as cg
import sweep_grid as sg

pytestmark = pytest.mark.gpu

KERNELS = (2, 1, 0)   # fp4 MFMA, int8 MFMA, VALU xor + popcount
FP4_TWINS = (3, 4)    # both run the fp4 form in a cross sweep
NPARTS = (2, 3, 7, 64)
FORMS = ("ab", "ba", "var")  # one variant a against b (swapped), one variant b against a (not swapped), 8 variants of a against b


@pytest.fixture(scope="module")
def eng():
    from rupphash_amd import Engine

    e = Engine(0)
    try:
        yield e
    finally:
        e.set_hamming_kernel(2)
        e.close()


def check_edges(e, var_a, b, want, what):
    """the edge list against the expected keys; indices within their sets and no (i, j, variant) twice"""
    n_a, n_b = len(var_a), len(b)
    assert (e["i"] < n_a).all() and (e["j"] < n_b).all(), what
    v = (e["flags"].astype(np.int64) >> sg.RPH_EDGE_VARIANT_SHIFT) & 7
    assert len(np.unique((e["i"].astype(np.int64) * n_b + e["j"]) * 8 + v)) == len(e), what
    diff = sg.difference(sg.edge_keys(e), want)
    assert not diff, f"{what}: {diff}"


def sweep(eng, kernel, var_a, b, thr, want, low_a=None, low_b=None, what="", **parts):
    """one sweep under a kernel setting; the capacity is passed explicitly (what is expected, and room to report too much).  Without
    flags a one-variant set goes through rph_hamming_cross_pairs, everything else through rph_hamming_variant_cross_pairs."""
    eng.set_hamming_kernel(kernel)
    try:
        e = eng.hamming_variant_cross_pairs(var_a, b, thr, low_conf_a=low_a, low_conf_b=low_b, cap=len(want) + 4096, **parts)
    finally:
        eng.set_hamming_kernel(2)
    if not parts:
        check_edges(e, var_a, b, want, f"{what} kernel={kernel} threshold={thr}")
    return e


def check_positions(eng, kernel, thresholds):
    counts = []
    for form in FORMS:
        var_a, b, _, _ = cg.positions_forms()[form]
        for thr in thresholds:
            want = cg.expected_once(("positions", form), var_a, b, None, None, thr)
            counts.append(len(sweep(eng, kernel, var_a, b, thr, want, what=f"positions {form}")))
    return counts


# ------------------------------------------------------------------ positions
@pytest.mark.parametrize("kernel", KERNELS)
def test_cross_positions(eng, kernel):
    """an edge at every row and column of block (0, 0), in every block of the 3 x 3 rectangle, in both short tiles; copies of either side's
    hash 0 in every tile of the other; variants 1 .. 7 in the corner blocks -- with a on the columns, b on the rows, and 8 variants"""
    thresholds = cg.THR["positions"]
    counts = check_positions(eng, kernel, thresholds)
    n = len(thresholds)
    assert counts[:n] == counts[n:2 * n] and counts[1] >= 1024 + 100 and counts[2 * n + 1] >= counts[1] + 150 and counts[-1] > counts[2 * n + 1]


@pytest.mark.parametrize("kernel", FP4_TWINS)
def test_cross_positions_fp4_settings(eng, kernel):
    check_positions(eng, kernel, (40, 75))


@pytest.mark.parametrize("kernel", KERNELS)
def test_cross_positions_low_confidence(eng, kernel):
    """both low-confidence arrays, and either alone, on the row side and on the column side (the one-variant forms with flags are
    rph_hamming_variant_cross_pairs with n_variants = 1, which swaps like the plain call)"""
    for form in FORMS:
        var_a, b, low_a, low_b = cg.positions_forms()[form]
        for which, la, lb in (("both", low_a, low_b), ("a", low_a, None), ("b", None, low_b)):
            for sim in cg.VARIANT_SIMS:
                want = cg.expected_once(("positions", form, which), var_a, b, la, lb, sim)
                plain = cg.expected_once(("positions", form), var_a, b, None, None, sim)
                assert len(want) < len(plain) or sim == 0
                sweep(eng, kernel, var_a, b, sim, want, la, lb, what=f"positions {form} low-confidence flags of {which}")


@pytest.mark.parametrize("kernel", KERNELS)
def test_cross_positions_sharded(eng, kernel):
    var_a, b, _, _ = cg.positions_forms()["var"]
    want = cg.expected_once(("positions", "var"), var_a, b, None, None, 40)
    for nparts in NPARTS:
        parts = [sweep(eng, kernel, var_a, b, 40, want, part=p, nparts=nparts) for p in range(nparts)]
        for e in parts:
            assert (e["i"] < len(var_a)).all() and (e["j"] < len(b)).all()
        diff = sg.difference(np.sort(np.concatenate([sg.edge_keys(e) for e in parts])), want)  # a pair reported by two parts shows as one reported twice
        assert not diff, f"positions var kernel={kernel} nparts={nparts}: {diff}"
        if nparts == 64:  # more parts than blocks: 3 x 3 of them
            assert sum(len(e) == 0 for e in parts) >= 55 and sum(len(e) > 0 for e in parts) >= 2


# ------------------------------------------------------------------ dense families
@pytest.mark.parametrize("kernel", KERNELS)
def test_cross_dense(eng, kernel):
    """cliques along one lane, across chunk edges and the tile seam, in both short tiles together with either hash 0, and the family that
    fills one wave's queue to 127 entries -- in both orders of the arguments (a rides on the rows in either)"""
    for form in ("ab", "ba"):
        var_a, b = cg.dense_forms()[form]
        for thr in cg.THR["dense"]:
            sweep(eng, kernel, var_a, b, thr, cg.expected_once(("dense", form), var_a, b, None, None, thr), what=f"dense {form}")


# ------------------------------------------------------------------ sizes
@pytest.mark.parametrize("n_a", cg.N_A)
def test_cross_sizes(eng, n_a):
    """row sets around every pass, wave, block and tile edge against one, two and three column tiles, pairs planted at the first and the
    last index of either side; with 8 variants the handful of rows stays on the rows"""
    for n_b in cg.N_B:
        for form, (var_a, b) in cg.sizes_forms(n_a, n_b).items():
            for thr in cg.THR["sizes"] + (cg.THR_SMALL_SIZES if max(n_a, n_b) <= 129 else ()):
                want = cg.expected(var_a, b, None, None, thr)
                for kernel in KERNELS:
                    sweep(eng, kernel, var_a, b, thr, want, what=f"sizes n_a={n_a} n_b={n_b} {form}")


# ------------------------------------------------------------------ the _dev form on a caller's stream
def test_cross_dev_forms(eng):
    from rupphash_amd import EDGE_DTYPE

    var_a, b, low_a, low_b = cg.positions_forms()["var"]
    thr = 50
    want = cg.expected_once(("positions", "var", "both"), var_a, b, low_a, low_b, thr)
    cap = len(want) + 4096
    n_a, n_b = len(var_a), len(b)
    bufs = [eng.dev_alloc(x) for x in (var_a.nbytes, b.nbytes, n_a, n_b, cap * EDGE_DTYPE.itemsize, 8)]
    d_a, d_b, d_la, d_lb, d_e, d_c = bufs
    st = eng.stream_create()
    try:
        for d, x in ((d_a, var_a), (d_b, b), (d_la, low_a), (d_lb, low_b)):
            eng.dev_upload(d, np.ascontiguousarray(x))
        eng.synchronize()
        for kernel in KERNELS:
            eng.set_hamming_kernel(kernel)
            eng.dev_memset(d_c, 0, 8, stream=st)
            eng.hamming_variant_cross_pairs_dev(d_a, 8, n_a, d_b, n_b, thr, d_e, cap, d_c, d_low_conf_a=d_la, d_low_conf_b=d_lb, stream=st)
            eng.stream_synchronize(st)
            cnt = np.zeros(1, np.uint64)
            eng.dev_download(cnt, d_c)
            assert int(cnt[0]) == len(want), kernel
            edges = np.zeros(int(cnt[0]), EDGE_DTYPE)
            eng.dev_download(edges, d_e)
            check_edges(edges, var_a, b, want, f"positions var on a stream, kernel={kernel}")
    finally:
        eng.set_hamming_kernel(2)
        eng.stream_destroy(st)
        for p in bufs:
            eng.dev_free(p)
