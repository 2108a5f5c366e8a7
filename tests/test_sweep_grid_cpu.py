"""The grids and references of sweep_grid.py, host half (no GPU).  The GPU tests compare the sweeps with the numpy references alone, so
those are pinned here first: the brute force against the oracle's all-pairs loop, the restated probe key against the oracle's own MIH
probing (the order in which a query meets its neighbours IS the key), and the grids against the coverage they promise -- an edge for
every row and column position of a tile, for every 32-row block, in the short last tile, and near duplicates of hash 0 there."""
import numpy as np
import pytest

import sweep_grid as sg

T = sg.TILE


def _all_grids():
    out = [("positions", 256, None), ("dense", 256, None), ("positions", 64, None), ("dense", 64, None)]
    return out + [("sizes", bits, n) for bits in (256, 64) for n in sg.SIZES]


def test_grids_are_seeded_and_built_once():
    for name, bits, n in _all_grids():
        h = sg.grid(name, bits, n)
        assert h is sg.grid(name, bits, n) and not h.flags.writeable
        assert h.dtype == (np.uint8 if bits == 256 else np.uint64) and len(h) == {"positions": sg.POSITIONS_N, "dense": sg.DENSE_N}.get(name, n)
    var, hashes, low = sg.variants()
    assert var is sg.variants()[0]
    saved = dict(sg._CACHE)
    sg._CACHE.clear()
    try:
        for name, bits, n in _all_grids():
            assert sg.grid(name, bits, n).tobytes() == saved[(name, bits) if n is None else (name, bits, n)].tobytes()
        again = sg.variants()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again, (var, hashes, low)))
    finally:
        sg._CACHE.clear()
        sg._CACHE.update(saved)


def test_flip_flips_distinct_bits_in_its_range():
    rng = np.random.default_rng(1)
    h = rng.integers(0, 256, 32, dtype=np.uint8)
    for d in (0, 1, 40, 128):
        x = np.unpackbits(sg.flip(h, d, rng, lo=128) ^ h, bitorder="little")
        assert x.sum() == d and x[:128].sum() == 0
    assert np.unpackbits(sg.flip(h, 256, rng) ^ h).sum() == 256


# ------------------------------------------------------------------ the brute force
@pytest.mark.parametrize("name", ["positions", "dense", "sizes"])
def test_brute256_equals_the_oracle_loop(oracle, name):
    for n in (sg.SIZES if name == "sizes" else (None,)):
        h = sg.grid(name, 256, n)
        thrs = sg.THR[(name, 256)] + (sg.THR_SMALL_SIZES if name == "sizes" and n <= 129 else ())
        for thr in thrs:
            want = oracle.all_pairs256(h, thr).astype(np.int64)  # ascending in (i, j), as np.nonzero is
            assert np.array_equal(sg.edges(name, thr, 256, n), want), (name, n, thr)
        assert np.array_equal(sg.brute256(h, thrs[1]), sg.edges(name, thrs[1], 256, n))


@pytest.mark.parametrize("name", ["positions", "dense", "sizes"])
def test_brute64_equals_the_oracle_distance(oracle, name):
    """the oracle has no u64 all-pairs loop: the distance matrix against the bit-matrix product (exact), and its own hamming64 on the
    edges of a threshold and on a sample of the other pairs"""
    rng = np.random.default_rng(2)
    for n in ((2, 33, 257, 1025) if name == "sizes" else (None,)):
        h = sg.grid(name, 64, n)
        d = sg.distances(name, 64, n)
        b = np.unpackbits(h.astype("<u8").view(np.uint8).reshape(-1, 8), axis=1).astype(np.float32)
        full = b.sum(1)[:, None] + b.sum(1)[None, :] - 2.0 * (b @ b.T)
        assert np.array_equal(np.triu(d, 1), np.triu(full, 1).astype(np.uint8))
        e = sg.brute64(h, 16)
        assert np.array_equal(e, sg.edges(name, 16, 64, n)) and (e[:, 0] < e[:, 1]).all()
        sample = np.concatenate([e[:300, :2], rng.integers(0, len(h), (300, 2))])
        for i, j in sample.tolist():
            if i < j:
                assert oracle.hamming64(h[i], h[j]) == d[i, j]


# ------------------------------------------------------------------ what the grids promise
def test_positions_cover_every_row_and_column_of_a_tile():
    e = sg.edges("positions", 40)
    i, j, d = e[:, 0], e[:, 1], e[:, 2]
    pairs = set(zip(i.tolist(), j.tolist()))
    # tile pair (0, 1): every owner position, every column position, either row half of every row block
    m = (i < T) & (j >= T) & (j < 2 * T)
    assert set(i[m].tolist()) == set(range(T)) and set((j[m] - T).tolist()) == set(range(T))
    assert {(r // 32, sg.lane_of(r, 0)[1]) for r in i[m].tolist()} == {(rb, half) for rb in range(32) for half in range(2)}
    # (the bijection sends a row to a column whose residue mod 32 depends on the row's alone: 32 lanes here, all 64 over the whole grid)
    assert {sg.lane_of(r % T, c % T) for r, c in pairs} == {(c32, half) for c32 in range(32) for half in range(2)}
    for k in range(T):
        assert (k, sg.tile1_partner(k)) in pairs
    # tile pair (2, 2): every position is owner or column, every 32-row block owns an edge, the explicit pairs
    m = (i >= 2 * T) & (j < 3 * T)
    assert set(i[m].tolist()) | set(j[m].tolist()) == set(range(2 * T, 3 * T))
    assert set(((i[m] - 2 * T) // 32).tolist()) == set(range(32))
    assert all(p in pairs for p in sg.POSITIONS_EXPLICIT)
    # the short tile: every column carries an edge or is a near miss; hash 0 has near duplicates there (one of them equal)
    cols = set((j[j >= 3 * T] - 3 * T).tolist())
    assert cols | set(sg.POSITIONS_NEAR_MISS) == set(range(37)) and not cols & set(sg.POSITIONS_NEAR_MISS)
    zero = sorted((int(b), int(c)) for a, b, c in e.tolist() if a == 0 and b >= 3 * T)
    assert len(zero) >= 2 and zero[0] == (3 * T, 0) and zero[-1][0] == sg.POSITIONS_N - 1
    assert set(d.tolist()) == set(range(41))
    # the near misses are pairs of their own at 41 .. 46, found by the wider thresholds only
    wide = {(a, b): c for a, b, c in sg.edges("positions", 46).tolist() if c > 40}
    assert [wide[tuple(sorted((sg.tail_source(t), 3 * T + t)))] for t in sg.POSITIONS_NEAR_MISS] == [41, 42, 43, 44, 45, 46]


def test_dense_families_are_cliques_where_they_should_be():
    fam = sg.dense_families()
    members = [m for f in fam.values() for m in f]
    assert len(members) == len(set(members))  # disjoint
    assert len({m % 32 for m in fam["lane"]}) == 1 and len(fam["lane"]) == 24 and fam["lane"][-1] // 256 == 2
    assert len({sg.lane_of(m, 0) for m in fam["rows64"]}) == 1 and len({m // 64 for m in fam["rows64"]}) == 16
    for start, length, column in sg.DENSE_RUNS:
        run = fam[f"run{length}"]
        assert len(run) == length and run[0] - T < column <= run[-1] - T
    assert {m // T for m in fam["seam"]} == {0, 1, 2} and fam["tail"][0] == 0 and fam["tail"][-1] == sg.DENSE_N - 1
    for bits in (256, 64):
        pairs = {(a, b): d for a, b, d in sg.edges("dense", 4, bits).tolist()}
        prefix = sg.grid("dense", bits)
        prefix = prefix[:, :16] if bits == 256 else (prefix & np.uint64(0xFFFFFFFF))
        differs = 0
        for f in fam.values():
            for x in range(len(f)):
                for y in range(x + 1, len(f)):
                    a, b = min(f[x], f[y]), max(f[x], f[y])
                    assert (a, b) in pairs
                    differs += pairs[(a, b)] > 0 and bool(np.all(prefix[a] == prefix[b]))
        assert differs > 500  # pairs that are equal in the screen's prefix and differ behind it
    assert 9000 < len(sg.edges("dense", 40)) < 11000


def test_sizes_hold_their_planted_pairs():
    for bits, main in ((256, 40), (64, 16)):
        for n in sg.SIZES:
            planted = sg.sizes_pairs(n, bits)
            assert len(planted) == (4 if n >= 5 else {2: 1, 3: 2}[n])
            d = sg.distances("sizes", bits, n)
            assert all(d[a, b] == dist for a, b, dist in planted)
            within = {(a, b) for a, b, _ in sg.edges("sizes", main, bits, n).tolist()}
            for a, b, dist in planted:
                assert ((a, b) in within) == (dist <= main)


def test_variants_hold_their_planted_triples():
    var, h, low = sg.variants()
    planted = sg.variants_planted()
    assert len(planted) >= 200 and planted[0][0] == 0 and planted[0][2] == sg.VARIANTS_N - 1
    assert len({(i, v) for i, v, _, _ in planted}) == len(planted) and all(j > i for i, _, j, _ in planted)
    assert {v for _, v, _, _ in planted} == set(range(1, 8)) and {d for _, _, _, d in planted} == set(range(46))
    assert {(i // T, j // T) for i, _, j, _ in planted} == {(0, 0), (0, 1), (1, 1)}
    assert np.array_equal(var[:, 0], h) and 0.10 < low.mean() < 0.20
    for sim in sg.VARIANT_SIMS:
        got = {(i, j, v): d for i, j, v, d in sg.variant_brute(var, h, low, sim).tolist()}
        want = {(i, j, v): d for i, v, j, d in planted if d <= (0 if low[i] | low[j] else sim)}
        assert got == want, sim  # unrelated variants and hashes are ~128 apart: the planted triples are all there is
    # a low-confidence side keeps an equal pair and drops a near one
    kept = {(i, j, v) for i, j, v, _ in sg.variant_brute(var, h, low, 40).tolist()}
    for t, there in ((46, True), (92, True), (47, False), (93, False)):
        i, v, j, d = planted[t]
        assert (low[i] | low[j]) and (d == 0) == there and ((i, j, v) in kept) == there


# ------------------------------------------------------------------ the probe key, against the oracle's own probing
def _neighbours_by_key(n, edges, flags):
    """for every i: the other ends of its edges that carry RPH_EDGE_MIH_R1, ordered by (probe key, id)"""
    keep = (flags & sg.RPH_EDGE_MIH_R1) != 0
    a = np.concatenate([edges[keep, 0], edges[keep, 1]])
    b = np.concatenate([edges[keep, 1], edges[keep, 0]])
    key = np.concatenate([flags[keep], flags[keep]]).astype(np.int64) & sg.RPH_EDGE_PROBE_MASK
    order = np.lexsort((b, key, a))
    a, b = a[order], b[order]
    start = np.searchsorted(a, np.arange(n + 1))
    return [b[start[i]:start[i + 1]] for i in range(n)]


def _pin_flags(oracle, h, bits, thr):
    kind = oracle.KIND_PDQ if bits == 256 else oracle.KIND_U64
    e = (sg.brute256 if bits == 256 else sg.brute64)(h, thr)
    flags = (sg.flags256 if bits == 256 else sg.flags64)(h, e[:, 0], e[:, 1], thr)
    assert ((flags & ~np.uint16(sg.RPH_EDGE_MIH_R1 | sg.RPH_EDGE_PROBE_MASK)) == 0).all()
    mine = _neighbours_by_key(len(h), e, flags)
    index = oracle.MIHIndex(kind, h)
    for i in range(len(h)):
        assert np.array_equal(index.query(i, thr, cap=4096), mine[i]), (bits, thr, i)
    return e, flags


@pytest.mark.parametrize("name", ["positions", "dense"])
@pytest.mark.parametrize("bits,thr", [(256, 40), (256, 10), (64, 16), (64, 5)])  # chunk tolerance 1 and 0 for either width
def test_restated_probe_key_orders_neighbours_as_the_oracle_meets_them(oracle, name, bits, thr):
    e, flags = _pin_flags(oracle, sg.grid(name, bits), bits, thr)
    keys = flags & sg.RPH_EDGE_PROBE_MASK
    if thr in (40, 16):
        assert (keys & 31).max() > 0 and (keys >> 5).max() > 0  # flipped-bit slots and chunks beyond the first occur
    else:
        assert ((keys & 31) == 0).all()


def test_restated_probe_key_on_the_unreachable_pair(oracle):
    """two bits in every 16-bit chunk: 32 apart, an edge at threshold 40, and not reachable by probing with one flipped bit"""
    a = np.zeros(32, np.uint8)
    b = np.zeros(32, np.uint8)
    b[0::2] = 0x03
    h = np.concatenate([sg.sizes(33), [a, b]])
    e, flags = _pin_flags(oracle, h, 256, 40)
    at = [k for k, (i, j, d) in enumerate(e.tolist()) if (i, j) == (33, 34)]
    assert len(at) == 1 and e[at[0], 2] == 32 and flags[at[0]] == 0
    # by hand.  hash 1: chunk 0 differs in two bits (passed over), chunk 1 is equal -> slot 0 of chunk 1.  hash 2: chunks 0 and 1 differ in
    # many bits, chunk 2 in bit 9 alone -> slot 10 of chunk 2 with one flipped bit allowed, unreachable without
    x = np.zeros((3, 32), np.uint8)
    x[1, 0] = 0x03
    x[2] = 0xFF
    x[2, 1] = 0x00
    x[2, 4:6] = (0x00, 0x02)
    assert sg.flags256(x, [0, 0], [1, 2], 40).tolist() == [0x8000 | 1 << 5, 0x8000 | 2 << 5 | 10]
    assert sg.flags256(x, [0, 0], [1, 2], 15).tolist() == [0x8000 | 1 << 5, 0]
    u = np.array([0, 0x00FF_FFFF_FF00_FF03, 0xFFFF_FFFF_FF20_FF03], np.uint64)
    assert sg.flags64(u, [0, 0], [1, 2], 8).tolist() == [0x8000 | 2 << 5, 0x8000 | 2 << 5 | 6]
    assert sg.flags64(u, [0, 0], [1, 2], 7).tolist() == [0x8000 | 2 << 5, 0]


# ------------------------------------------------------------------ the thresholds reach every prefix width
def test_thresholds_reach_every_prefix_width():
    from rupphash_amd import _lib

    L = _lib.load()
    thrs = sg.THR[("positions", 256)]
    assert thrs == sg.THR[("sizes", 256)]
    for kernel in (0, 1):
        assert {L.rph_hamming_prefix_dwords(t, kernel) for t in thrs} == {4, 5, 6, 7, 8}
    for kernel in (2, 3, 4):
        assert {L.rph_hamming_prefix_dwords(t, kernel) for t in thrs} == {4, 6, 8}
    assert [L.rph_hamming_prefix_dwords(t, 1) for t in (40, 50, 60, 75, 100)] == [4, 5, 6, 7, 8]
    assert [L.rph_hamming_prefix_dwords(t, 2) for t in (40, 50, 60, 75, 100)] == [4, 6, 6, 8, 8]


def test_keys_tell_edge_lists_apart():
    want = sg.pack([0, 5, 5], [1, 6, 7], [0, 256, 3], [0x8000, 0, 0x81FF])
    assert sg.unpack(want) == [(0, 1, 0, 0x8000), (5, 6, 256, 0), (5, 7, 3, 0x81FF)]
    assert sg.difference(want, want) == ""
    assert "missing [(5, 7, 3, 33279)]" in sg.difference(want[:2], want)
    assert "twice [(0, 1, 0, 32768)]" in sg.difference(np.sort(np.concatenate([want, want[:1]])), want)
    assert "extra or reported twice [(5, 6, 256, 1)]" in sg.difference(sg.pack([0, 5, 5], [1, 6, 7], [0, 256, 3], [0x8000, 1, 0x81FF]), want)
