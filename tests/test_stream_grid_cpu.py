"""What tests/stream_grid.py claims about itself, without a GPU: its geometry model of the streaming PDQ kernels (csrc/pdq_stream_stages.hpp)
is sane at every width and height 128..512, and its sweep lists reach every behaviour the model tells apart -- computed from the model
here, not written down.  The counts the model gives are pinned with their names, so a change to the kernels' constants shows up here."""
import os
import re

import numpy as np

import stream_grid as sg

# what the model gives today; a different count means the kernels' constants or rules changed and the sweep lists want another look
COUNTS = {"flush patterns": 44, "strip distributions": 144, "band distributions": 194, "empty last band": 15, "two trailing bands": 29,
          "one more strip": 4, "steps past the last pixel": 193}


def _stages():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "rupphash_amd", "csrc", "pdq_stream_stages.hpp")) as f:
        return f.read()


def test_model_constants_are_the_kernels():
    src = _stages()
    assert int(re.search(r"constexpr\s+int\s+ST_BAND\s*=\s*(\d+)\s*;", src).group(1)) == sg.BAND
    assert re.search(r"typedef\s+float\s+f32x32\s+__attribute__\(\(ext_vector_type\((\d+)\)\)\)", src).group(1) == str(sg.FILE)
    assert int(re.search(r"ST_OFF_DIV\s*=\s*ST_OFF_EDGE\s*\+\s*(\d+)\s*;", src).group(1)) == sg.FILE  # edge[] has 32 slots
    assert f"__builtin_popcountll(em) > {sg.FILE}" in src
    assert "((2 * jn + 1) * g.W) / 128 + g.lead_r" in src and "((2 * ni + 1) * g.H) / 128 + 2 * g.lead_c < T0 + ST_BAND" in src
    assert "g.ns_c = ((127 * g.W) / 128 + g.lead_r) / 64 + 1;" in src and "g.nb = (g.H + 2 * g.lead_c + ST_BAND - 1) / ST_BAND;" in src


def test_model_is_sane_for_every_width():
    for W in sg.ALL:
        m = sg.width_model(W)
        assert 2 <= m.win <= 8 and m.lead == (m.win + 2) // 2 - 1 and m.a + m.lead + 1 == m.win, W
        assert len(m.emit) == 64 and all(b > a for a, b in zip(m.emit, m.emit[1:])), W  # 64 kept columns, no two on one step
        assert sum(m.per_strip) == 64 and max(m.per_strip) <= sg.FILE, (W, m.per_strip)
        assert m.emit[-1] < 64 * m.ns_c and m.emit[-1] >= 64 * (m.ns_c - 1), W  # the last walked strip is the one of the last kept column
        assert sum(m.flushes) == 64 and max(m.flushes) <= sg.FILE and min(m.flushes) >= 1, (W, m.flushes)
        assert m.ns_c - m.ns_b in (0, 1), W
        assert m.past == sum(t >= W for t in m.emit) <= m.lead, W
        if m.ns_c > m.ns_b:  # the strip past the pixels holds kept columns: that is why it is walked
            assert m.per_strip[-1] >= 1 and m.past >= m.per_strip[-1], W


def test_model_is_sane_for_every_height():
    for H in sg.ALL:
        m = sg.height_model(H)
        assert 2 <= m.win <= 8 and m.nb == len(m.per_band) == len(m.steady), H
        assert sum(m.per_band) == 64 and max(m.per_band) <= sg.FILE, (H, m.per_band)
        assert not m.steady[0] and not m.steady[-1], H  # the first band grows the window, the last one shrinks it
        assert 56 * (m.nb - 1) < H + 2 * m.lead <= 56 * m.nb, H
        # the kernels' cursor: it starts every band where the band before stopped, a D pass emits what the model counts, all 64 leave
        starts, emitted, end = sg.band_cursor(H)
        assert tuple(emitted) == m.per_band and end == 64, H
        assert starts == [sum(m.per_band[:k]) for k in range(m.nb)], H


def test_counts_of_the_model():
    c = sg.census()
    got = {k: len(v) for k, v in c.items()}
    assert got == COUNTS, f"the model gives {got}, recorded are {COUNTS}"
    assert c["one more strip"] == {128, 256, 384, 512}
    print(f"model over 385 widths and 385 heights: {got}")


def test_pairings_hold_every_width_and_height_once():
    for name, lst in (("A", sg.PAIRING_A), ("B", sg.PAIRING_B)):
        assert len(lst) == sg.SIDES
        assert sorted(w for w, _ in lst) == list(sg.ALL) and sorted(h for _, h in lst) == list(sg.ALL), name
        size = sum(w * h for w, h in lst)
        assert 38e6 < size < 41e6, (name, size)
        # the order of the ragged calls: the same geometries, neighbours never of one window
        order = sg.ragged_order(lst)
        assert sorted(order) == sorted(lst)
        assert all(sg.axis(a[0]).win != sg.axis(b[0]).win for a, b in zip(order, order[1:])), name
        same_h = sum(sg.axis(a[1]).win == sg.axis(b[1]).win for a, b in zip(order, order[1:]))
        assert same_h < sg.SIDES // 4, (name, same_h)
    assert not set(sg.PAIRING_A) & set(sg.PAIRING_B)


def test_cross_list_meets_every_rare_width_with_rare_heights():
    pat = sg.widths_of_pattern()
    for W in sg.UNIQUE_PATTERN_WIDTHS:
        assert pat[sg.width_model(W).flushes] == [W], W
    for W, family in sg.PATTERN_FAMILIES.items():
        assert W in family and len({sg.width_model(x).flushes for x in family}) == 1, W
        assert len(pat[sg.width_model(W).flushes]) > 1
    assert {W for W in sg.ALL if sg.one_more_strip(W)} <= set(sg.CROSS_WIDTHS)
    assert {H for H in sg.ALL if sg.empty_last_band(H)} <= set(sg.CROSS_HEIGHTS)
    for win in range(2, 9):  # a height that ends in two non-steady bands per window that has one (window 2 has none: H = 128 is 3 bands)
        two = [H for H in sg.ALL if sg.axis(H).win == win and sg.two_trailing_bands(H)]
        assert not two or set(two) & set(sg.CROSS_HEIGHTS), win
    assert len(set(sg.CROSS_WIDTHS)) == len(sg.CROSS_WIDTHS) == 15 and len(set(sg.CROSS_HEIGHTS)) == len(sg.CROSS_HEIGHTS)
    # axis coverage of the thinned list
    assert len(set(sg.CROSS)) == len(sg.CROSS) <= 200
    for W in sg.CROSS_WIDTHS:
        assert len({h for w, h in sg.CROSS if w == W}) >= 2, W
    for H in sg.CROSS_HEIGHTS:
        assert len({w for w, h in sg.CROSS if h == H}) >= 2, H
    assert {w for w, _ in sg.CROSS} == set(sg.CROSS_WIDTHS) and {h for _, h in sg.CROSS} == set(sg.CROSS_HEIGHTS)
    # every height of the list meets a width at which the recurrence walks a strip past the pixels
    for H in sg.CROSS_HEIGHTS:
        assert any(sg.one_more_strip(w) for w, h in sg.CROSS if h == H), H


def test_sweeps_reach_everything_the_model_tells_apart():
    everything = sg.census()
    for name, lst in (("PAIRING_A", sg.PAIRING_A), ("PAIRING_B", sg.PAIRING_B)):  # each pairing alone: both kernels see all of it
        got = sg.reached(lst)
        for k, want in everything.items():
            assert got[k] == want, f"{name} reaches {len(got[k])} of {len(want)} {k}"
    # CROSS: what is rare on one axis against what is rare on the other
    got = sg.reached(sg.CROSS)
    assert got["empty last band"] == everything["empty last band"], f"CROSS: {len(got['empty last band'])} of {len(everything['empty last band'])}"
    assert got["one more strip"] == everything["one more strip"]
    rare = {p for p, ws in sg.widths_of_pattern().items() if set(ws) & set(sg.CROSS_WIDTHS)}
    assert got["flush patterns"] == rare and len(rare) == 12, sorted(rare)  # 8 unique + 3 families + the one of 128 / 256 / 384 / 512
    assert {sg.axis(H).win for H in got["two trailing bands"]} == {sg.axis(H).win for H in everything["two trailing bands"]}
    print("reached by each pairing: " + ", ".join(f"{len(v)} {k}" for k, v in everything.items())
          + f"; CROSS: {len(sg.CROSS)} geometries of {len(sg.CROSS_WIDTHS)} widths x {len(sg.CROSS_HEIGHTS)} heights")


def test_contents():
    for w, h in [(128, 128), (129, 511), (512, 131), (333, 200), (512, 509)]:
        a, b, c = (sg.image(w, h, k) for k in sg.KINDS)
        for im in (a, b, c):
            assert im.shape == (h, w) and im.dtype == np.uint8
        assert a.min() == 0 and a.max() == 255 and len(np.unique(a)) == 256
        nb, nc = np.count_nonzero(b), np.count_nonzero(c == 0)
        pts = sg.seam_points(w, h, np.random.default_rng([w, h, 1, 0]))
        assert {(y, x) for y, x, _ in pts} == set(zip(*np.nonzero(b))) and b[0, 0] and b[-1, -1]
        passes = len(sg.width_model(w).flushes)
        cells = (len(pts) - 5) // (2 * (passes - 1))  # pixels per seam point
        assert passes >= 2 and len(pts) == 2 * (passes - 1) * cells + 5 and cells in (1, 4, 9) and nb <= len(pts)
        assert abs(int(b.max()) * cells -sg.POINT_PEAK * sg.axis(w).win * sg.axis(h).win) < cells
        first = sg.width_model(w).flushes[0]  # the first boundary: a point at kept column first - 1, one at kept column first
        assert pts[0][1] - sg.sample_pos(first - 1, w) in (0, 1) and pts[cells][1] - sg.sample_pos(first, w) in (0, 1)
        assert 16 <= nc + 2 <= w * h // 250 + 4 and set(np.unique(c)) == {0, 255}
        assert np.array_equal(a, sg.image(w, h, "a")) and not np.array_equal(a, sg.image(w, h, "a", 1))  # seeded by (w, h, kind)
        rgb = sg.image_rgb(w, h)
        assert rgb.shape == (h, w, 3) and not np.array_equal(rgb[..., 0], rgb[..., 1]) and not np.array_equal(rgb[..., 1], rgb[..., 2])
    assert not np.array_equal(sg.image(200, 300, "a"), sg.image(300, 200, "a").T)
