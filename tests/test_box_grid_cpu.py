"""What tests/box_grid.py claims about itself, without a GPU: its geometry lists hold every seam class that the control-flow model of the
multi-pass PDQ kernels (csrc/pdq_kernels.hip) derives, each with named witnesses; the one-loop box pass the tiled kernels rely on is the
reference's four-phase one for every line length and window; the luma residue triples exist."""
import numpy as np
import pytest

import box_grid as bg


def _hold(lengths, classes_of, wanted, what):
    wit = bg.witnesses(lengths, classes_of)
    report = "\n".join(f"  {c}: {wit.get(c, [])[:12]}" for c in wanted)
    missing = [c for c in wanted if not wit.get(c)]
    assert not missing, f"{what}: no geometry has {missing}; witnesses:\n{report}"
    return report


def test_grid_holds_every_seam_class_on_both_axes():
    ws, hs = [w for w, _ in bg.GRID], [h for _, h in bg.GRID]
    print("row axis (w)\n" + _hold(ws, bg.row_classes, bg.ROW_CLASSES, "row axis of GRID"))
    print("column axis (h), tail_sampled_kernel\n" + _hold(hs, bg.col_classes, bg.COL_CLASSES, "column axis of GRID"))
    print("box_cols_kernel (h)\n" + _hold(hs, bg.cols_kernel_classes, bg.COLS_KERNEL_CLASSES, "box_cols_kernel over GRID"))
    # the two axis sets the list is built from are all there, on both axes, and nothing is listed twice
    assert set(bg.SMALL + bg.LARGE) <= set(ws) and set(bg.SMALL + bg.LARGE) <= set(hs)
    assert len(set(bg.GRID)) == len(bg.GRID) and 290 <= len(bg.GRID) <= 310
    assert all(5 <= w <= 512 and 5 <= h <= 512 for w, h in bg.GRID)
    assert sorted((w, h) for w in bg.GRID_WIDTHS for h in bg.grid_heights(w)) == bg.GRID


def test_colour_subset_holds_every_class_of_the_row_axis():
    print(_hold([w for w, _ in bg.COLOUR_GRID], bg.row_classes, bg.ROW_CLASSES, "row axis of COLOUR_GRID"))
    assert 35 <= len(set(bg.COLOUR_GRID)) == len(bg.COLOUR_GRID) <= 45
    assert all(5 <= w <= 512 and 5 <= h <= 512 for w, h in bg.COLOUR_GRID)


def test_thumbnails_hold_the_sides_no_caller_can_pass(oracle):
    for (w, h), thumb in bg.THUMBS.items():
        assert oracle.target_dimensions(w, h) == thumb, (w, h)
        assert min(w, h) >= 5 and max(w, h) > 512  # hashable, and behind the pre-downsample
    sides = {min(t) for t in bg.THUMBS.values()}
    assert sides == {1, 2, 3, 4, 5, 63, 64, 65, 127} and all(max(t) == 512 for t in bg.THUMBS.values())
    _hold([nh for _, nh in bg.THUMBS.values()], bg.col_classes, bg.THUMB_COL_CLASSES, "column axis of the thumbnails")
    # on the row axis a side of 1..4 is one partial tile like any w < 64; its partner is w = 512: the extra tile of 4 steps, slot -8
    for nw, nh in bg.THUMBS.values():
        if nh <= 4:
            assert nw == 512 and {"extra tile of 4 steps", "sample from slot -8", "sample from the extra tile"} <= bg.row_classes(nw)
            assert bg.box_geo(nh).win == 1 and "bulk shorter than one unrolled round" in bg.cols_kernel_classes(nh)


def test_extra_tile_lengths_are_the_hand_derived_ones():
    """(len + lead - 1) // 64 > (len - 1) // 64: the window's lead pushes the last outputs past the last loaded tile.  By hand: lead is 1 for
    windows 2 and 3, 2 for 4 and 5, 3 for 6 and 7, 4 for 8, so the lengths are the last `lead` ones up to each multiple of 64 from 128 on --
    128 | 192 | 255, 256 | 319, 320 | 382..384 | 446..448 | 509..512."""
    by_hand = [128, 192, 255, 256, 319, 320, 382, 383, 384, 446, 447, 448, 509, 510, 511, 512]
    assert [n for n in range(1, 513) if bg.has_extra_tile(n)] == by_hand
    assert [n for n in range(1, 513) if any(t.extra for t in bg.line_tiles(n)[1])] == by_hand
    assert set(by_hand) <= set(bg.LARGE)
    for n in by_hand:
        extra = [t for t in bg.line_tiles(n)[1] if t.extra]
        assert len(extra) == 1 and extra[0].steps == n + bg.box_geo(n).lead - extra[0].c0 and 1 <= extra[0].steps <= 4


def test_model_invariants_for_every_length():
    for n in range(1, 513):
        g, tiles = bg.line_tiles(n)
        assert g.win == max(1, (n + 63) // 64) and g.lead == (g.win + 2) // 2 - 1 <= 4 and g.win <= bg.HIST
        assert sum(t.steps for t in tiles) == g.total and [t.c0 for t in tiles] == list(range(0, g.total, 64))
        assert [s.j for t in tiles for s in t.samples] == list(range(64))
        for t in tiles:
            assert t.loaded != t.extra and not (t.fast and not t.loaded)
            assert t.fetches_next == any(u.c0 == t.c0 + 64 and u.loaded for u in tiles)
            if t.fast:
                assert t.steps == 64
            for s in t.samples:
                assert -bg.HIST <= s.slot < 64 - g.win and s.col == ((2 * s.j + 1) * n) // 128 < n
                assert (s.slot < 0) == (s.step < g.win)  # the first `win` steps of a tile put their outputs into the history slots


def test_batch_sets_straddle_images_and_end_in_partial_workgroups():
    calls = [(n, h) for h in bg.BATCH_H for n in bg.BATCH_N]
    spans = {(n, h): max(last - first + 1 for _, _, first, last in bg.batch_blocks(n, h)) for n, h in calls}
    tails = {(n, h): bg.batch_blocks(n, h)[-1][1] for n, h in calls}
    wide = sorted(k for k, v in spans.items() if v >= 3)
    one = sorted(k for k, v in tails.items() if v == 1)
    sixty_three = sorted(k for k, v in tails.items() if v == 63)
    print(f"(n, h) with a workgroup over >= 3 images: {wide}\n(n, h) whose last workgroup has 1 line: {one}\n63 lines: {sixty_three}")
    assert wide and one and sixty_three, (wide, one, sixty_three)
    assert max(spans.values()) >= 13  # h = 5: thirteen images in one workgroup
    for n in bg.BATCH_COLOUR_N:
        assert n in bg.BATCH_N and any(spans[(n, h)] >= 3 for h in bg.BATCH_H)
    for n, h in calls:
        blocks = bg.batch_blocks(n, h)
        assert sum(b[1] for b in blocks) == n * h and len(blocks) == (n * h + 63) // 64


def test_dispatch_threshold_is_the_documented_one():
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rupphash.h")).read()
    assert f"from {bg.stream_min_images()} images per call" in re.sub(r"\s*\n\s*\*\s*", " ", header)


def test_contents_at_the_smallest_sizes():
    for h, w in [(1, 1), (1, 512), (5, 5), (3, 7), (64, 64), (37, 100)]:
        imgs = bg.contents(np.random.default_rng(1), h, w)
        assert imgs.shape == (8, h, w) and len(bg.CONTENT_NAMES) == 8
        assert not imgs[2].any() and (imgs[3] == 255).all() and 1 <= np.count_nonzero(imgs[4]) <= min(40, h * w)
        if h * w >= 64:
            assert len({im.tobytes() for im in imgs}) == 8  # neighbouring lines of a straddling workgroup differ


def test_luma_residue_triples():
    t = bg.luma_residue_triples()
    for res in (-1, 0, 1):
        assert len(set(t[res])) >= 64
        for r, g, b in t[res]:
            assert 0 <= min(r, g, b) and max(r, g, b) <= 255 and (299 * r + 587 * g + 114 * b + 500 - res) % 1000 == 0
    img = bg.residue_image(9, 300)
    seen = {(int(r), int(g), int(b)) for r, g, b in img.reshape(-1, 3)}
    assert seen <= set(t[-1]) | set(t[0]) | set(t[1]) and all(len(seen & set(t[res])) >= 64 for res in (-1, 0, 1))


def test_colour_contents_and_embedding():
    imgs = bg.colour_contents(np.random.default_rng(2), 9, 33, 4)
    assert imgs.shape == (9, 9, 33, 4) and imgs[..., 3].min() >= 1 and len(np.unique(imgs[..., 3])) == 255
    buf, rs, st = bg.embed(imgs, 3, 5, lead=1)
    assert rs == 33 * 4 + 3 and st == rs * 9 + 5 and buf.size == 1 + 9 * st
    for k in (0, 8):
        for y in (0, 8):
            assert np.array_equal(buf[1 + k * st + y * rs:][:33 * 4], imgs[k, y].reshape(-1))
    assert np.count_nonzero(buf == 0xA5) >= 9 * (9 * 3 + 5)


def test_one_loop_box_pass_is_the_four_phase_one():
    """every line length 1..512 under every window 1..8 (the kernels clamp a window to the length), on sparse, flat, saturated, step and
    noise lines: the bits of box_one_loop are those of box_four_phase"""
    rng = np.random.default_rng(20261020)
    for length in range(1, 513):
        x = bg.probe_lines(rng, length)
        for win in range(1, 9):
            a, b = bg.box_one_loop(x, win), bg.box_four_phase(x, win)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (length, win)


def test_four_phase_restatement_is_the_oracles(oracle):
    """oracle.jarosz on a plane of one row is one pass of box_along_rows (the column pass over one row is the identity: in / 1)"""
    rng = np.random.default_rng(7)
    for length in [1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 127, 128, 129, 255, 256, 300, 448, 509, 512]:
        x = bg.probe_lines(rng, length)
        for win in range(1, min(length, 8) + 1):
            ours = bg.box_four_phase(x, win)
            for k in range(len(x)):
                ref = oracle.jarosz(x[k:k + 1], win, 1, nreps=1)
                assert np.array_equal(ours[k:k + 1].view(np.uint32), ref.view(np.uint32)), (length, win, k)


@pytest.mark.parametrize("w,h", [(5, 5), (5, 7), (6, 6), (7, 5), (8, 8), (9, 9), (15, 15), (16, 5), (17, 17), (64, 5), (5, 64), (33, 31), (65, 9), (127, 7)])
def test_two_one_loop_passes_and_decimation_are_the_oracles_buffer(oracle, w, h):
    imgs = bg.contents(np.random.default_rng(w * 1009 + h), h, w)
    for k in (0, 1, 3, 4, 5, 7):
        rc, _, _, b64 = oracle.pdq_from_luma(imgs[k], want_buf64=True)
        assert rc == 0
        assert np.array_equal(bg.buffer64_one_loop(imgs[k]).view(np.uint32), b64.view(np.uint32)), bg.CONTENT_NAMES[k]
