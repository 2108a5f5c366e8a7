"""What tests/blake3_grid.py claims about itself, without a GPU: its case lists hold every seam class that the control-flow model of the
BLAKE3 kernels (csrc/blake3_kernels.hip) derives, each with named witnesses; the model's group_first is a plain cumulative sum; the tree
the model's schedule builds is the one of the specification's chaining-value stack; the bytes a modelled pixel block reads are the RGBA16
stream of the image."""
import numpy as np
import pytest

import blake3_grid as g
import blake3_util as b3
import png_util


def _hold(wit, wanted, what):
    table = g.report(wit, wanted)
    missing = [c for c in wanted if not wit.get(c)]
    assert not missing, f"{what}: no case has {missing}; witnesses:\n{table}"
    print(f"{what}\n{table}")


# ---- byte strings
def test_in_wave_list_holds_every_count_and_every_block_class():
    lens = g.IN_WAVE_LENGTHS
    assert len(lens) == len(set(lens)) == 448 and sum(lens) < 24 << 20
    for d in g.TAILS:
        assert {k * g.CHUNK - d for k in range(1, 65)} <= set(lens)
    assert all(any(g.GROUP_BYTES + k * g.CHUNK - d in lens for d in g.TAILS) for k in range(1, 65))
    host = g.byte_classes(lens, 256, 0)               # the host form packs from offset 0
    dev = g.byte_classes(lens, 256, g.IN_WAVE_START)  # the _dev form of the test starts at an odd address
    _hold(host, g.COUNT_CLASSES + g.BLOCK_CLASSES[:-1], "in-wave list, host form")
    _hold(dev, g.COUNT_CLASSES + g.BLOCK_CLASSES[:-1], "in-wave list, _dev form")
    assert "group in the second grid pass" not in host


def test_fold_list_holds_every_round_and_carry():
    wit = g.merge((f"{n} groups", {c: ["-"] for c in g.fold_classes(n)}) for n in g.FOLD_GROUPS)
    _hold(wit, g.FOLD_CLASSES, "fold counts")
    assert [g.groups_of(x) for x in g.FOLD_LENGTHS] == list(g.FOLD_GROUPS) and sum(g.FOLD_LENGTHS) < 80 << 20
    assert max(g.FOLD_GROUPS) <= 4096
    _hold(g.byte_classes(g.FOLD_LENGTHS, 256), g.FOLD_CLASSES, "fold strings as one call")
    # by hand: a level has 2 rounds from 129 nodes, 3 from 257; the odd node of 129 is node 64 of 65 (round 2), of 257 node 128 of 129 (round 3)
    assert [(a.cnt, a.next, a.rounds, a.carry_round) for a in g.fold_levels(129)[:2]] == [(129, 65, 2, 2), (65, 33, 1, 1)]
    assert g.fold_levels(257)[0] == g.Level(257, 129, 3, 3, False) and g.fold_levels(128)[0] == g.Level(128, 64, 1, 0, False)
    assert [a.root for a in g.fold_levels(5)] == [False, False, True] and [a.carry_round for a in g.fold_levels(5)] == [1, 1, 0]


@pytest.mark.parametrize("n", g.PLAN_SIZES)
def test_plan_model_is_a_cumulative_sum(n):
    lens = g.plan_lengths(n)
    p = g.plan(lens)
    want = np.concatenate([[0], np.cumsum([g.groups_of(x) for x in lens])])
    assert np.array_equal(p.group_first, want), n
    assert p.per == {1: 1, 2: 1, 1023: 1, 1024: 1, 1025: 2, 2047: 2, 2048: 2, 2049: 3}[n]
    assert max(lens) == g.PLAN_LONG and (n <= 2 or min(lens) == 0)


def test_plan_model_on_other_sizes():
    rng = np.random.default_rng(1)
    for n in (3, 64, 65, 1000, 4097, 10_000):
        lens = (rng.integers(0, 5, n) * rng.integers(0, 2, n) * 40_000).tolist()
        assert np.array_equal(g.plan(lens).group_first, np.concatenate([[0], np.cumsum([g.groups_of(x) for x in lens])])), n


def test_plan_sizes_hold_every_thread_and_wave_edge():
    wit = g.merge((f"n={n}", g.byte_classes(g.plan_lengths(n), 256)) for n in g.PLAN_SIZES)
    _hold(wit, g.PLAN_CLASSES, "plan sizes")
    per_n = {n: g.byte_classes(g.plan_lengths(n), 256) for n in g.PLAN_SIZES}
    assert "plan thread with 0 strings" in per_n[1023] and "plan thread with 0 strings" not in per_n[1024]
    assert "plan thread with 0 strings" in per_n[1025] and "plan thread with 1 string" in per_n[1025] and "plan thread with 2 strings" in per_n[1025]
    assert set(k for k in per_n[2048] if k.startswith("plan thread")) == {"plan thread with 2 strings"}
    for n in g.PLAN_SIZES[2:]:
        for c in ("multi-group string last in a thread range", "multi-group string at lane 63", "multi-group string at lane 0 of a later wave",
                  "multi-group string in the last thread that has strings"):
            assert per_n[n].get(c), (n, c)


@pytest.mark.parametrize("cus", g.GRID_PASS_CUS)
def test_grid_pass_case_straddles_the_pass(cus):
    lens = g.grid_pass_lengths(cus)
    assert len(lens) == cus * 64 + 64 + 3
    waves, cap = g.bytes_launch(len(lens), sum(lens), cus)
    assert waves == cus * 64 < sum(g.groups_of(x) for x in lens) <= cap
    wit = g.byte_classes(lens, cus)
    _hold(wit, g.PASS_CLASSES, f"grid-pass case at {cus} compute units")
    assert wit["string straddling the grid pass"] == [f"{cus * 64 - 1}:{2 * g.GROUP_BYTES + 777}"]
    wv = g.bytes_waves(lens, cus)
    mine = wv.string == cus * 64 - 1
    assert wv.pass_no[mine].tolist() == [0, 1, 1] and wv.k[mine].tolist() == [0, 1, 2] and wv.in_group[mine].tolist() == [64, 64, 1]
    assert (wv.pass_no == 1).sum() == 64 + 3 + 2 and wv.pass_no.max() == 1


# ---- the tree
@pytest.mark.parametrize("key", [None, g.KEY], ids=["hash", "keyed"])
def test_model_tree_is_the_stack_tree_at_the_fold_counts(key):
    """fold_kernel's schedule on n nodes (chunk values stand in for group values: the tree over n leaves is the same) against blake3_stack"""
    for n in g.FOLD_GROUPS:
        data = b3.test_input(n * g.CHUNK - 5)
        cv, kw, base = b3.chunk_cvs(data, key)
        assert cv.shape[1] == n
        assert g.fold_kernel(cv, kw, base) == b3.blake3_stack(data, key), n


def test_wave_fold_is_the_stack_tree_at_every_count():
    for key in (None, g.KEY):
        for c in range(1, 65):
            data = b3.test_input(c * g.CHUNK - c)
            assert g.model_digest(data, key) == (b3.blake3_stack(data) if key is None else b3.blake3(data, key)), c


def test_model_digest_of_multi_group_strings():
    """wave_fold without ROOT under fold_kernel: counts 1, 2 and 63 in the last group, 2, 3 and 5 groups"""
    for n in (g.GROUP_BYTES + 1, g.GROUP_BYTES + 1025, 2 * g.GROUP_BYTES - 1024, 2 * g.GROUP_BYTES + 7, 4 * g.GROUP_BYTES + 3000):
        data = b3.test_input(n)
        assert g.model_digest(data) == b3.blake3(data) and g.model_digest(data, g.KEY) == b3.blake3(data, g.KEY), n


# ---- pixels
def _uniform_wit(geos, n=2, lead=1):
    return {ch: g.merge((f"{w}x{h}", {c: ["-"] for c in g.uniform_walk_classes(w, h, ch, n, lead)}) for w, h in geos) for ch in g.UNIFORM_CHANNELS}


def test_block_geometries_hold_every_block_class_for_every_channel_count():
    for ch, wit in _uniform_wit(g.BLOCK_GEOS).items():
        _hold(wit, g.pixel_block_classes(False), f"uniform kernel, {ch} channel(s), d_px + 1")


def test_block_geometries_hold_every_block_class_for_every_layout():
    specs = g.ragged_block_specs()
    offs, strides, _ = g.ragged_place(specs)
    by_layout = {}
    for (lay, w, h), o, st in zip(specs, offs, strides):
        assert lay < 16 or (o % 2 == 0 and st % 4 == 2)
        assert lay > 16 or st % 2 == 1
        by_layout.setdefault(lay, []).append((f"{w}x{h}@{o}", {c: ["-"] for c in g.pixel_classes(w, h, lay, st, o)}))
    assert sorted(by_layout) == list(g.LAYOUTS)
    for lay, tables in by_layout.items():
        _hold(g.merge(tables), g.pixel_block_classes(lay > 16), f"ragged kernel, layout {lay}")


def test_pixel_count_lists_hold_every_count():
    wit = g.merge((f"{w}x{h}", {c: ["-"] for c in g.pixel_count_classes(w, h)}) for w, h in g.COUNT_GEOS + g.EDGE_GEOS)
    wit = g.merge([("", wit)] + [(f"{n} of {w}x{h}", {c: ["-"] for c in g.pixel_count_classes(w, h, n)}) for n, w, h in g.NG_CASES])
    _hold(wit, g.PIXEL_COUNT_CLASSES, "uniform pixel counts")
    assert all(w * h <= 2 * g.GROUP_PX for w, h in g.COUNT_GEOS)
    specs = g.ragged_count_specs()
    wit = g.merge((f"layout {lay} {w}x{h}", {c: ["-"] for c in g.pixel_count_classes(w, h)}) for lay, w, h in specs)
    _hold(wit, g.PIXEL_COUNT_CLASSES[:-4], "ragged pixel counts")
    assert {lay for lay, _, _ in specs} == set(g.LAYOUTS)
    big = g.merge((f"{w}x{h}", {c: ["-"] for c in g.pixel_count_classes(w, h)}) for w, h in g.BIG_GEOS)
    _hold(big, g.FOLD_CLASSES, "129 and 257 groups per image")
    assert [len(g.pixel_groups(w, h)) for w, h in g.BIG_GEOS] == [129, 257]
    assert [len(g.pixel_groups(w, h)) for _, w, h in g.RAGGED_BIG_SPECS] == [1, 129, 2, 1, 257, 3, 1]


@pytest.mark.parametrize("ch", g.UNIFORM_CHANNELS)
def test_modelled_blocks_read_the_rgba16_stream_uniform(ch):
    for w, h in g.BLOCK_GEOS + g.COUNT_GEOS[::9] + g.EDGE_GEOS:
        imgs = g.uniform_images(w, h, ch, 2)
        buf, rs, st = g.embed_uniform(imgs, 1)
        for i in range(2):
            blocks, offs = g.pixel_walk(w, h, ch, rs, 1 + i * st)
            assert len(offs) == w * h and sum(b.bpx for b in blocks) == w * h
            assert g.layout_rgba16(g.gather(buf, offs, ch), ch) == b3.rgba16_bytes(imgs[i]), (w, h, ch, i)


def test_modelled_blocks_read_the_rgba16_stream_ragged():
    specs = g.ragged_block_specs() + g.ragged_count_specs()[::7]
    buf, views, offs, strides = g.embed_ragged(specs)
    for (lay, w, h), v, o, st in zip(specs, views, offs, strides):
        blocks, po = g.pixel_walk(w, h, lay, st, o)
        assert len(po) == w * h and all(b.fast or b.bpx < 8 or b.rows > 1 for b in blocks)
        assert g.layout_rgba16(g.gather(buf, po, lay), lay) == png_util.to_rgba16(v), (lay, w, h)
    assert np.count_nonzero(buf == 0xA5) > len(specs)


def test_walk_by_hand():
    """9 x 15 Luma8 at address 1, stride 10: chunk 0 is rows 0..13 and two pixels of row 14; its first block crosses one row end, no block of
    it is fast (8 pixels never fit the rest of a 9-pixel row but at x = 0 and x = 1)"""
    blocks, offs = g.pixel_walk(9, 15, 1, 10, 1)
    assert [b.chunk for b in blocks] == [0] * 16 + [1] and blocks[16].bpx == 7 and blocks[16].mid_row_chunk
    assert blocks[0].fast and blocks[0].addr3 == 1 and not blocks[0].ends_row and not blocks[1].fast and blocks[1].rows == 2
    assert offs[:10].tolist() == [1, 2, 3, 4, 5, 6, 7, 8, 9, 11]
    b8, _ = g.pixel_walk(8, 17, 3, 25, 0)
    assert all(b.fast and b.ends_row for b in b8) and [b.addr3 for b in b8[:4]] == [0, 1, 2, 3]
    b1, _ = g.pixel_walk(1, 130, 4, 5, 0)
    assert [b.rows for b in b1] == [8] * 16 + [2] and not any(b.fast for b in b1)
    assert g.pixel_groups(0, 5) == [(1, True)] and g.pixel_groups(128, 64) == [(64, True)] and g.pixel_groups(8193, 1) == [(64, False), (1, False)]
