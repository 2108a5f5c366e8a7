"""The square Hamming sweeps on the grids of sweep_grid.py, under every kernel setting.  Every expected value is the numpy brute force
plus the restated probe key (both pinned against the C oracle in test_sweep_grid_cpu.py); no kernel is compared with another one.
An edge list is compared as its sorted (i, j, d, flags) tuples, packed into one integer each; a difference names the first tuples that
are missing and that are extra or reported twice, from which the tile pair, wave, row block, lane and chunk follow."""
import numpy as np
import pytest

import sweep_grid as sg

pytestmark = pytest.mark.gpu

# 2 = fp4 MFMA (+-1 operands at these sizes), 4 = its popcount-sorted {0,1} form, 3 = fp4 +-1 forced, 1 = int8 MFMA, 0 = VALU xor + popcount
K256 = (2, 4, 3, 1, 0)
K64 = (2, 0)  # fp4 MFMA with the whole hash as one slice, VALU
NPARTS = (2, 3, 7, 64)


@pytest.fixture(scope="module")
def eng():
    from rupphash_amd import Engine

    e = Engine(0)
    try:
        yield e
    finally:
        e.set_hamming_kernel(2)
        e.close()


def sweep(eng, kernel, h, thr, bits, want, **parts):
    """one sweep under a kernel setting; the capacity is passed explicitly (what is expected, and room to report too much)"""
    eng.set_hamming_kernel(kernel)
    try:
        return (eng.hamming_all_pairs if bits == 256 else eng.hamming_all_pairs64)(h, thr, cap=want + 4096, **parts)
    finally:
        eng.set_hamming_kernel(2)


def check(eng, kernel, name, thr, bits=256, n=None):
    h, want = sg.grid(name, bits, n), sg.expected(name, thr, bits, n)
    e = sweep(eng, kernel, h, thr, bits, len(want))
    size = len(h)
    assert (e["i"] < e["j"]).all() and (e["j"] < size).all(), (name, bits, n, kernel, thr)
    assert len(np.unique(e["i"].astype(np.int64) * size + e["j"])) == len(e), (name, bits, n, kernel, thr)  # no pair twice
    diff = sg.difference(sg.edge_keys(e), want)
    assert not diff, f"{name} bits={bits} n={n} kernel={kernel} threshold={thr}: {diff}"
    return len(e)


def check_sharded(eng, kernel, name, thr, bits):
    h, want = sg.grid(name, bits), sg.expected(name, thr, bits)
    for nparts in NPARTS:
        parts = [sweep(eng, kernel, h, thr, bits, len(want), part=p, nparts=nparts) for p in range(nparts)]
        diff = sg.difference(np.sort(np.concatenate([sg.edge_keys(e) for e in parts])), want)  # a pair reported by two parts shows as one reported twice
        assert not diff, f"{name} bits={bits} kernel={kernel} nparts={nparts}: {diff}"
        if nparts == 64:  # more parts than blocks: 4 tiles make 10 tile pairs
            assert sum(len(e) == 0 for e in parts) >= 54 and sum(len(e) > 0 for e in parts) >= 2


# ------------------------------------------------------------------ 256-bit hashes
@pytest.mark.parametrize("kernel", K256)
def test_sweep_positions(eng, kernel):
    """an edge at every row and column position of a tile, in every 32-row block, in the short last tile; a copy of hash 0 there"""
    counts = [check(eng, kernel, "positions", thr) for thr in sg.THR[("positions", 256)]]
    assert counts[1] >= 1024 + 512 + 31 and counts[-1] > counts[1]


@pytest.mark.parametrize("kernel", K256)
def test_sweep_positions_sharded(eng, kernel):
    check_sharded(eng, kernel, "positions", 40, 256)


@pytest.mark.parametrize("kernel", K256)
def test_sweep_dense_families(eng, kernel):
    """cliques along one lane, along row-block pairs, across chunk edges and tile seams, and in the short tile together with hash 0"""
    for thr in sg.THR[("dense", 256)]:
        check(eng, kernel, "dense", thr)


@pytest.mark.parametrize("n", sg.SIZES)
def test_sweep_sizes(eng, n):
    """sizes around every block, chunk and tile edge, with pairs planted at the first and the last index"""
    for kernel in K256:
        for thr in sg.THR[("sizes", 256)] + (sg.THR_SMALL_SIZES if n <= 129 else ()):
            check(eng, kernel, "sizes", thr, n=n)


@pytest.mark.parametrize("kernel", K256)
def test_sweep_variants(eng, kernel):
    """8 variants per row against the hashes: the pass loop, (owner * 8 + v) addressing, the low-confidence limit"""
    var, h, low = sg.variants()
    eng.set_hamming_kernel(kernel)
    try:
        for sim in sg.VARIANT_SIMS:
            want = sg.variant_brute(var, h, low, sim)
            e = eng.hamming_variant_pairs(var, h, sim, low_conf=low, cap=len(want) + 4096)
            got = np.stack([e["i"], e["j"], (e["flags"] >> sg.RPH_EDGE_VARIANT_SHIFT) & 7, e["d"]], axis=1).astype(np.int64)
            assert sorted(map(tuple, got.tolist())) == sorted(map(tuple, want.tolist())), (kernel, sim)
            # the probe key rides along: that of (variant v of i, hash j)
            x = var[got[:, 0], got[:, 2]] ^ h[got[:, 1]]
            assert np.array_equal(e["flags"] & ~np.uint16(7 << sg.RPH_EDGE_VARIANT_SHIFT), sg._flags(x, 16, 16, sim)), (kernel, sim)
    finally:
        eng.set_hamming_kernel(2)


# ------------------------------------------------------------------ 64-bit hashes
@pytest.mark.parametrize("kernel", K64)
def test_sweep_u64_positions(eng, kernel):
    for thr in sg.THR[("positions", 64)]:
        check(eng, kernel, "positions", thr, bits=64)


@pytest.mark.parametrize("kernel", K64)
def test_sweep_u64_positions_sharded(eng, kernel):
    check_sharded(eng, kernel, "positions", 16, 64)
    check_sharded(eng, kernel, "positions", 40, 64)  # nearly every pair is an edge: 4.75 million of them


@pytest.mark.parametrize("kernel", K64)
def test_sweep_u64_dense_families(eng, kernel):
    for thr in sg.THR[("dense", 64)]:
        check(eng, kernel, "dense", thr, bits=64)


@pytest.mark.parametrize("n", sg.SIZES)
def test_sweep_u64_sizes(eng, n):
    for kernel in K64:
        for thr in sg.THR[("sizes", 64)]:
            check(eng, kernel, "sizes", thr, bits=64, n=n)
