"""The grids and references of cross_grid.py, host half (no GPU).  The GPU tests compare the cross sweeps with the numpy references alone,
so those are pinned here first: the one-variant brute force against the oracle's all-pairs loop on the concatenation of the two sets, the
8-variant brute force with its two low-confidence arrays against the oracle's grouping, the probe key against sweep_grid.flags256 (itself
pinned against the oracle's MIH probing), and the grids against the coverage they promise."""
import ctypes as C

import numpy as np
import pytest

import cross_grid as cg
import sweep_grid as sg

T = cg.T


def _all_grids():
    var, b, low_a, low_b, _ = cg.positions()
    out = [("positions", x) for x in (var, b, low_a, low_b)] + [("dense", x) for x in cg.dense()]
    return out + [(("sizes", n_a, n_b), x) for n_a in cg.N_A for n_b in cg.N_B for x in cg.sizes(n_a, n_b)]


def _cross_of_square(e, n_a):
    """the edges (i, j, ...) of a sweep of a ++ b that have one end on each side, j counted within b"""
    e = e[(e[:, 0] < n_a) & (e[:, 1] >= n_a)].copy()
    e[:, 1] -= n_a
    return e


def test_grids_are_seeded_built_once_and_read_only():
    first = _all_grids()
    assert all(x is y and not x.flags.writeable for (_, x), (_, y) in zip(first, _all_grids()))
    var, b, low_a, low_b, _ = cg.positions()
    assert var.shape == (cg.POS_NA, 8, 32) and b.shape == (cg.POS_NB, 32) and (len(low_a), len(low_b)) == (cg.POS_NA, cg.POS_NB)
    assert [len(x) for x in cg.dense()] == [cg.DENSE_NA, cg.DENSE_NB] and cg.DENSE_NA > cg.DENSE_NB
    for name, forms in (("positions", cg.positions_forms()), ("dense", cg.dense_forms()), ("sizes", cg.sizes_forms(33, 129))):
        for form in forms.values():
            assert all(not x.flags.writeable for x in form) and form[0].ndim == 3 and form[0].shape[1] in (1, 8), name
    saved = dict(cg._CACHE)
    cg._CACHE.clear()
    try:
        assert all(x.tobytes() == y.tobytes() for (_, x), (_, y) in zip(first, _all_grids()))
    finally:
        cg._CACHE.clear()
        cg._CACHE.update(saved)


# ------------------------------------------------------------------ the brute force
def _pin_one_variant(oracle, a, b, thr):
    both = np.concatenate([a, b])
    want = _cross_of_square(oracle.all_pairs256(both, thr).astype(np.int64), len(a))  # ascending in (i, j), as np.nonzero is
    got = cg.brute(a.reshape(-1, 1, 32), b, None, None, thr)
    assert (got[:, 2] == 0).all() and np.array_equal(got[:, [0, 1, 3]], want), thr
    return len(want)


@pytest.mark.parametrize("name", ["positions", "dense"])
def test_one_variant_brute_force_equals_the_oracle_loop(oracle, name):
    a, b = cg.positions_forms()["ab"][:2] if name == "positions" else cg.dense_forms()["ab"]
    counts = [_pin_one_variant(oracle, a[:, 0], b, thr) for thr in cg.THR[name]]
    assert counts[0] > 0 and counts[-1] > counts[0]
    # ... and the other order of the arguments is the transpose
    x, y = (cg.positions_forms() if name == "positions" else cg.dense_forms())["ba"][:2]
    ab, ba = cg.brute(a, b, None, None, 40), cg.brute(x, y, None, None, 40)
    assert sorted(map(tuple, ab[:, [0, 1, 3]].tolist())) == sorted(map(tuple, ba[:, [1, 0, 3]].tolist()))


def test_sizes_brute_force_equals_the_oracle_loop(oracle):
    for n_a in cg.N_A:
        for n_b in cg.N_B:
            a, b = cg.sizes_forms(n_a, n_b)["one"]
            assert _pin_one_variant(oracle, a[:, 0], b, 40) >= 1
    for n_a, n_b in ((1, 33), (129, 129), (33, 1)):  # the thresholds at which nearly every pair is an edge
        a, b = cg.sizes_forms(n_a, n_b)["one"]
        assert _pin_one_variant(oracle, a[:, 0], b, 200) > 0.99 * n_a * n_b and _pin_one_variant(oracle, a[:, 0], b, 256) == n_a * n_b


def _pin_variants(oracle, var, b, low_a, low_b, sim):
    """the oracle's grouping of a ++ b: A's files own 8 variants, B's own one (has_features 0); low confidence through the quality"""
    n_a, n_b = len(var), len(b)
    from rupphash_amd import _lib

    L = _lib.load()
    assert L.rph_is_low_pdq_quality(10) == 1 and L.rph_is_low_pdq_quality(90) == 0
    hashes = np.concatenate([var[:, 0], b])
    variants = np.concatenate([var, np.repeat(b[:, None, :], 8, axis=1)])
    has_features = np.concatenate([np.ones(n_a, np.uint8), np.zeros(n_b, np.uint8)])
    quality = np.where(np.concatenate([low_a, low_b]) != 0, 10, 90).astype(np.int32)
    edges, _ = oracle.group_pdq(hashes, sim, variants=variants, has_features=has_features, quality=quality)
    want = _cross_of_square(edges.astype(np.int64), n_a)
    got = cg.brute(var, b, low_a, low_b, sim)
    assert sorted(map(tuple, got[:, :2].tolist())) == sorted(map(tuple, want.tolist())), sim  # one entry per variant that matches
    return got


def test_variant_brute_force_equals_the_oracle_grouping(oracle):
    var, b, low_a, low_b, _ = cg.positions()
    for sim in cg.VARIANT_SIMS:
        got = _pin_variants(oracle, var, b, low_a, low_b, sim)
        assert (sim == 0 or (got[:, 2] > 0).sum() > 50) and len(got) > 30
    n_a, n_b = 33, 129
    var, b = cg.sizes(n_a, n_b)
    rng = np.random.default_rng(5)
    for sim in cg.VARIANT_SIMS:
        _pin_variants(oracle, var, b, (rng.random(n_a) < 0.3).astype(np.uint8), (rng.random(n_b) < 0.3).astype(np.uint8), sim)
    # missing flags are flags of zero
    zeros_a, zeros_b = np.zeros(len(var), np.uint8), np.zeros(len(b), np.uint8)
    assert np.array_equal(cg.brute(var, b, None, None, 40), cg.brute(var, b, zeros_a, zeros_b, 40))


# ------------------------------------------------------------------ the probe key
@pytest.mark.parametrize("name", ["positions", "dense"])
@pytest.mark.parametrize("thr", [40, 10])  # chunk tolerance 1 and 0
def test_probe_key_of_cross_edges_is_that_of_the_square_sweep(name, thr):
    """cross edges are exactly the square edges of a ++ b with one end on each side, and carry the same flags"""
    a, b = cg.positions_forms()["ab"][:2] if name == "positions" else cg.dense_forms()["ab"]
    both = np.concatenate([a[:, 0], b])
    e = sg.brute256(both, thr)
    flags = sg.flags256(both, e[:, 0], e[:, 1], thr)
    keep = (e[:, 0] < len(a)) & (e[:, 1] >= len(a))
    want = sg.pack(e[keep, 0], e[keep, 1] - len(a), e[keep, 2], flags[keep])
    got = cg.expected(a, b, None, None, thr)
    assert len(want) > 30 and not sg.difference(got, want)
    keys = got & np.uint64(sg.RPH_EDGE_PROBE_MASK)
    assert (keys >> np.uint64(5)).max() > 0 and ((keys & np.uint64(31)).max() > 0) == (thr == 40)


def test_expected_carries_the_variant_above_the_probe_key():
    var, b, low_a, low_b, info = cg.positions()
    rows = sg.unpack(cg.expected(var, b, low_a, low_b, 40))
    e = cg.brute(var, b, low_a, low_b, 40)
    assert sorted((i, j, f >> sg.RPH_EDGE_VARIANT_SHIFT & 7, d) for i, j, d, f in rows) == sorted(map(tuple, e.tolist()))
    i, v, j, d = info["triples"][3]
    assert d <= 40 and [f for x, y, _, f in rows if (x, y) == (i, j)] == [int(v << 9 | sg._flags((var[i, v] ^ b[j])[None], 16, 16, 40)[0])]


# ------------------------------------------------------------------ what the grids promise
def test_positions_block_00_has_an_edge_at_every_row_and_column():
    var, b, _, _, _ = cg.positions()
    e = cg.brute(var, b, None, None, 40)
    e = e[e[:, 2] == 0]
    m = (e[:, 0] < T) & (e[:, 1] < T)
    i, j = e[m, 0], e[m, 1]
    # (a) every row and every column position; both halves of every row block and all 64 lanes, whichever side becomes the rows
    assert set(i.tolist()) == set(range(T)) and set(j.tolist()) == set(range(T))
    lanes = {(c32, half) for c32 in range(32) for half in range(2)}
    for rows, cols in ((i, j), (j, i)):
        assert {(r // 32, sg.lane_of(r, 0)[1]) for r in rows.tolist()} == {(rb, half) for rb in range(32) for half in range(2)}
        assert {sg.lane_of(r, c) for r, c in zip(rows.tolist(), cols.tolist())} == lanes
    partner = cg.block00_partner()
    assert sorted(partner.tolist()) == list(range(T))
    pairs = set(zip(i.tolist(), j.tolist()))
    assert all((k, int(partner[k])) in pairs for k in range(T))
    # what the square rule `col <= owner` would drop
    assert (j < i).sum() >= 100 and (j == i).sum() >= 100 and (j > i).sum() >= 100
    assert all((k, k) in pairs for k in (0, 31, 32, 1023))
    # (g) every distance 0 .. 40
    assert set(e[m, 3].tolist()) == set(range(41))


def test_positions_cover_every_block_the_short_tiles_and_hash_0():
    var, b, _, _, info = cg.positions()
    e = cg.brute(var, b, None, None, 40)
    e = e[e[:, 2] == 0]
    i, j = e[:, 0], e[:, 1]
    # (b) every one of the 3 x 3 blocks, the short x short corner included
    blocks = {(I, J): int(((i // T == I) & (j // T == J)).sum()) for I in range(3) for J in range(3)}
    assert min(blocks.values()) >= 8, blocks
    # (c) every row of a's short tile and every column of b's carries an edge or is a listed near miss; partners in all tiles of the other side
    rows, cols = set((i[i >= 2 * T] - 2 * T).tolist()), set((j[j >= 2 * T] - 2 * T).tolist())
    assert rows | set(cg.POS_A_NEAR_MISS) == set(range(37)) and not rows & set(cg.POS_A_NEAR_MISS)
    assert cols | set(cg.POS_B_NEAR_MISS) == set(range(41)) and not cols & set(cg.POS_B_NEAR_MISS)
    assert set((j[i >= 2 * T] // T).tolist()) == {0, 1, 2} and set((i[j >= 2 * T] // T).tolist()) == {0, 1, 2}
    # (d) near duplicates of a[0] in every tile of b, one equal to it, one in b's last column -- and of b[0] in a likewise
    for mine, theirs, n in ((e[i == 0][:, [1, 3]], b, cg.POS_NB), (e[j == 0][:, [0, 3]], var[:, 0], cg.POS_NA)):
        at = dict(mine.tolist())
        assert {k // T for k in at} == {0, 1, 2} and n - 1 in at and at[2 * T] == 0 and 0 < at[n - 1] <= 40
    assert np.array_equal(var[0, 0], b[0]) and np.array_equal(var[0, 0], b[2 * T]) and np.array_equal(b[0], var[2 * T, 0])
    # (g) the planted pairs are there at their distances; the near misses are pairs of their own at 41 .. 46
    d = cg.distances(var, b)
    assert all(d[x, 0, y] == dist for x, y, dist in info["pairs"] + info["near_miss"])
    assert sorted(dist for _, _, dist in info["near_miss"]) == [41, 42, 43, 44, 45, 46]
    within = set(zip(i.tolist(), j.tolist()))
    assert all((x, y) in within for x, y, _ in info["pairs"]) and not any((x, y) in within for x, y, _ in info["near_miss"])
    wide = cg.brute(var, b, None, None, 46)
    wide = {(x, y) for x, y, v, dist in wide.tolist() if v == 0 and dist > 40}
    assert {(x, y) for x, y, _ in info["near_miss"]} <= wide


def test_positions_variants_and_low_confidence_flags():
    var, b, low_a, low_b, info = cg.positions()
    triples = info["triples"]
    # (e)
    assert len(triples) >= 200 and {v for _, v, _, _ in triples} == set(range(1, 8)) and {d for _, _, _, d in triples} == set(range(46))
    assert {(i // T, j // T) for i, _, j, _ in triples} >= {(0, 0), (0, 2), (2, 0), (2, 2)}
    assert len({(i, v) for i, v, _, _ in triples}) == len(triples) and np.array_equal(var[:, 0], cg.positions_forms()["ab"][0][:, 0])
    d = cg.distances(var, b)
    assert all(d[i, v, j] == dist for i, v, j, dist in triples)
    got = {(i, j, v) for i, j, v, _ in cg.brute(var, b, None, None, 40).tolist()}
    assert all(((i, j, v) in got) == (dist <= 40) for i, v, j, dist in triples)
    # (f) ~15 % low-confidence files, none of them planted but for the four exceptions: equal pairs stay, near pairs go
    assert 0.10 < low_a.mean() < 0.20 and 0.10 < low_b.mean() < 0.20
    assert not any(low_a[i] or low_b[j] for i, v, j, _ in triples)
    exceptions = {(i, j) for i, j, _, _ in info["exceptions"]}
    assert all(not (low_a[i] or low_b[j]) for i, j, _ in info["pairs"] if (i, j) not in exceptions)
    assert [(dist == 0, side) for _, _, dist, side in info["exceptions"]] == [(True, "a"), (True, "b"), (False, "a"), (False, "b")]
    for sim in (31, 40, 63):
        kept = {(i, j) for i, j, v, _ in cg.brute(var, b, low_a, low_b, sim).tolist() if v == 0}
        plain = {(i, j) for i, j, v, _ in cg.brute(var, b, None, None, sim).tolist() if v == 0}
        for i, j, dist, side in info["exceptions"]:
            assert (low_a[i], low_b[j]) == ((1, 0) if side == "a" else (0, 1)) and (i, j) in plain and ((i, j) in kept) == (dist == 0)
        # either array alone drops its own near pair only
        only_a = {(i, j) for i, j, v, _ in cg.brute(var, b, low_a, None, sim).tolist() if v == 0}
        only_b = {(i, j) for i, j, v, _ in cg.brute(var, b, None, low_b, sim).tolist() if v == 0}
        near_a, near_b = info["exceptions"][2][:2], info["exceptions"][3][:2]
        assert near_a not in only_a and near_b in only_a and near_a in only_b and near_b not in only_b


def test_dense_families_are_where_they_should_be():
    a, b = cg.dense()
    fam = cg.dense_families()
    rows = [r for rr, _ in fam.values() for r in rr] + [cg.QUEUE_HUB]
    cols = [c for _, cc in fam.values() for c in cc] + [cg.QUEUE_LONE_COLUMN]
    assert len(rows) == len(set(rows)) and len(cols) == len(set(cols))  # disjoint
    lane_rows, lane_cols = fam["lane"]
    assert len(lane_cols) == 24 and len({c % 32 for c in lane_cols}) == 1 and len({sg.lane_of(r, 0)[1] for r in lane_rows}) == 1
    assert len({sg.lane_of(r, c) for r in lane_rows for c in lane_cols}) == 1
    run_rows, run_cols = fam["runs"]
    assert run_rows == list(range(run_rows[0], run_rows[0] + 70)) and run_rows[0] < 256 <= run_rows[-1]
    assert sorted(run_cols) == sorted(c for s, n, _ in cg.DENSE_RUNS for c in range(s, s + n))
    assert [n for _, n, _ in cg.DENSE_RUNS] == [63, 64, 65] and all(s % T < edge <= (s + n - 1) % T for s, n, edge in cg.DENSE_RUNS)
    for side in fam["seam"]:
        assert {x // T for x in side} == {0, 1}
    assert fam["tail"][0][0] == 0 and fam["tail"][0][-1] == cg.DENSE_NA - 1 and fam["tail"][1][0] == 0 and fam["tail"][1][-1] == cg.DENSE_NB - 1
    assert min(fam["tail"][0][1:]) >= T and min(fam["tail"][1][1:]) >= T
    d = cg.distances(*cg.dense_forms()["ab"])[:, 0, :]
    prefix = cg.prefix_distances(a, b)
    differs = 0
    for rr, cc in fam.values():
        block = d[np.ix_(rr, cc)]
        assert block.max() <= 4
        differs += int(((block > 0) & (prefix[np.ix_(rr, cc)] == 0)).sum())
    assert differs > 500  # pairs that are equal in the screen's prefix and differ behind it
    assert set(d[np.ix_(fam["queue1"][0], fam["queue1"][1])].ravel().tolist()) <= {0, 1, 2, 3, 4}
    assert 17_000 < len(cg.brute(*cg.dense_forms()["ab"], None, None, 40)) < 60_000
    assert len(cg.brute(*cg.dense_forms()["ab"], None, None, 0)) > 1000


def test_dense_queue_fill_family_fills_one_waves_queue_to_127():
    """two rows of opposite halves near all 32 columns 256 .. 287; in another row-block pair of the same wave, the hub near all 32 columns
    224 .. 255 and a row of the other half near 31 of them: 63 entries carried (fewer than the 64 that start a drain) and 64 new"""
    a, b = cg.dense()
    fam = cg.dense_families()
    lo, hi = cg.QUEUE_WAVE_ROWS
    (r1, r2), (r4,), hub = fam["queue1"][0], fam["queue2"][0], cg.QUEUE_HUB
    assert all(lo <= r < hi for r in (r1, r2, r4, hub)) and hi - lo == 256 and lo % 256 == 0
    assert sg.lane_of(r1, 0)[1] != sg.lane_of(r2, 0)[1] and sg.lane_of(hub, 0)[1] != sg.lane_of(r4, 0)[1]
    assert r1 // 64 == r2 // 64 and hub // 64 == r4 // 64 and r1 // 64 != hub // 64
    d = cg.distances(*cg.dense_forms()["ab"])[:, 0, :]
    prefix = cg.prefix_distances(a, b)
    for dist in (d, prefix):
        near = dist[lo:hi, :T] <= 40
        assert {(lo + r, c) for r, c in zip(*map(np.ndarray.tolist, np.nonzero(near)))} == (
            {(r, c) for r in (r1, r2) for c in range(256, 288)} | {(hub, c) for c in range(224, 256)}
            | {(r4, c) for c in range(224, 256) if c != cg.QUEUE_LONE_COLUMN})
    assert cg.queue_fill(128) == [0, 63, 64, 0, 0, 0, 0, 0] and cg.queue_fill(256) == [63, 64, 0, 0]


def test_sizes_hold_their_planted_pairs():
    assert {511, 512, 513} <= set(cg.N_A) and {1, 2, 1023, 1024, 1025} <= set(cg.N_A) and max(cg.N_B) == 2 * T + 1
    for n_a in cg.N_A:
        for n_b in cg.N_B:
            var, b = cg.sizes(n_a, n_b)
            planted = cg.sizes_pairs(n_a, n_b)
            assert len(planted) == len({(i, j) for i, j, _ in planted}) == (5 if n_a > 2 and n_b > 1 else len(planted)) and planted[0] == (0, 0, 0)
            assert all(0 <= i < n_a and 0 <= j < n_b for i, j, _ in planted)
            d = cg.distances(var, b)
            assert all(d[i, 0, j] == dist for i, j, dist in planted) and d[n_a - 1, 7, n_b - 1] == 5
            one = cg.sizes_forms(n_a, n_b)["one"]
            assert one[0].shape == (n_a, 1, 32) and np.array_equal(one[0][:, 0], var[:, 0])
            within = {(i, j) for i, j, _, _ in cg.brute(one[0], b, None, None, 40).tolist()}
            assert all(((i, j) in within) == (dist <= 40) for i, j, dist in planted)
            assert (n_a - 1, n_b - 1, 7, 5) in set(map(tuple, cg.brute(var, b, None, None, 40).tolist()))
    assert cg.sizes_pairs(1025, 2049) == [(0, 0, 0), (0, 2048, 40), (1024, 0, 41), (1024, 2048, 7), (512, 1024, 3)]
    assert cg.sizes_pairs(1, 1) == [(0, 0, 0)] and cg.sizes_pairs(1, 33) == [(0, 0, 0), (0, 32, 40), (0, 16, 3)]


# ------------------------------------------------------------------ thresholds and layout
def test_thresholds_reach_every_prefix_width():
    from rupphash_amd import _lib

    L = _lib.load()
    assert cg.THR["positions"] == cg.THR["sizes"] == (0, 40, 50, 60, 75, 100) and cg.THR["dense"] == (0, 4, 40)
    for kernel in (0, 1):
        assert {L.rph_hamming_prefix_dwords(t, kernel) for t in cg.THR["positions"]} == {4, 5, 6, 7, 8}
    for kernel in (2, 3, 4):
        assert {L.rph_hamming_prefix_dwords(t, kernel) for t in cg.THR["positions"]} == {4, 6, 8}
        assert {L.rph_hamming_prefix_dwords(t, kernel) for t in (40, 75)} == {4, 8}
    assert {L.rph_hamming_prefix_dwords(t, k) for t in cg.THR["dense"] for k in range(5)} == {4}  # the queue fill is counted at width 4


def _layout(n_a, n_variants, n_b, nparts=1, kernel=2):
    from rupphash_amd import _lib

    swap, seg, segs, blocks = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint64()
    _lib.load().rph_debug_hamming_cross_layout(n_a, n_variants, n_b, nparts, kernel, C.byref(swap), C.byref(seg), C.byref(segs), C.byref(blocks))
    return bool(swap.value), seg.value, segs.value, blocks.value


def test_layout_rule_swaps_where_the_grids_say_it_does():
    for kernel in (2, 1, 0):
        assert _layout(cg.POS_NA, 1, cg.POS_NB, kernel=kernel) == (True, 1, 3, 9)    # (a, b): a is the smaller set
        assert _layout(cg.POS_NB, 1, cg.POS_NA, kernel=kernel) == (False, 1, 3, 9)   # (b, a)
        assert _layout(cg.POS_NA, 8, cg.POS_NB, kernel=kernel) == (False, 1, 3, 9)   # variants stay on the rows
        assert _layout(cg.POS_NB, 8, cg.POS_NA, kernel=kernel) == (False, 1, 3, 9)
        assert _layout(cg.POS_NA, 8, cg.POS_NB, nparts=64, kernel=kernel)[3] == 9    # 64 parts: 55 of them own no block
        assert _layout(cg.DENSE_NA, 1, cg.DENSE_NB, kernel=kernel) == (False, 1, 2, 4)
        assert _layout(cg.DENSE_NB, 1, cg.DENSE_NA, kernel=kernel) == (True, 1, 2, 4)
        assert _layout(1, 8, 2049, kernel=kernel) == (False, 1, 3, 3)                # one row (8 variants) against three column tiles
        assert _layout(1, 1, 2049, kernel=kernel) == (True, 1, 1, 3)
        assert _layout(1025, 1, 2049, kernel=kernel)[0] and not _layout(1025, 1, 1025, kernel=kernel)[0] and not _layout(1025, 1, 257, kernel=kernel)[0]
