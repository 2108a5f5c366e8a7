"""The CPU oracle of the > 512 px pre-downsample (oracle/resize_ref.c) against the plain restatement of the published algorithm in
tests/resize_util.py, byte for byte: on every geometry x content the GPU tests use (tests/test_resize_gpu.py), and on every source
size from 513 to 4096.  No GPU.  (No input is made up for the clamp to 255: it cannot bite below a window of about 128 taps, see
resize_util.)"""
import numpy as np
import pytest

import resize_util as ru


def test_tables_of_all_outputs_at_once_equal_the_plain_loop():
    for in_size, out_size in [(513, 512), (768, 512), (1024, 512), (1537, 512), (3020, 512), (3328, 512), (6144, 512), (41, 40), (480, 40), (4000, 512), (5, 1), (650, 258),
                              (1285, 512), (120, 39), (777, 512), (4096, 512), (2049, 512), (3, 3)]:
        a, b = ru.build_axis_plain(in_size, out_size), ru.build_axis(in_size, out_size)
        assert (a.window, a.precision) == (b.window, b.precision), (in_size, out_size)
        assert np.array_equal(a.start, b.start) and np.array_equal(a.size, b.size) and np.array_equal(a.coef, b.coef), (in_size, out_size)


def test_restatement_on_hand_derived_cases():
    """2:1 and 4:1 are block means rounded half up, twice (u8 intermediate); luma and target sizes as the reference computes them"""
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (64, 72), dtype=np.uint8)
    for f in (2, 4):
        s = img.astype(np.int64)
        hor = (2 * sum(s[:, k::f] for k in range(f)) + f) // (2 * f)
        ver = (2 * sum(hor[k::f] for k in range(f)) + f) // (2 * f)
        assert np.array_equal(ru.resize_box_u8(img, 72 // f, 64 // f), ver.astype(np.uint8))
    assert ru.axis_info(1024, 512) == (15, 3, 32768, 32768) and ru.axis_info(768, 512) == (14, 3, 16384, 16384)
    assert [ru.target_dimensions(*s) for s in [(4000, 5), (5, 4000), (1285, 650), (513, 513), (1537, 120), (600, 600)]] == \
        [(512, 1), (1, 512), (512, 258), (512, 512), (512, 39), (512, 512)]
    assert ru.to_luma601(np.array([[[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255], [1, 1, 1]]], np.uint8)).tolist() == [[255, 0, 76, 150, 29, 1]]


def test_geometries_reach_what_they_are_for():
    by = {ru.geometry_id(g): g for g in ru.GEOMETRIES}
    assert len(by) == len(ru.GEOMETRIES) == 19
    windows = {k: ru.build_axis(g.w, g.nw).window for k, g in by.items()}
    assert (windows["513x41"], windows["768x60"], windows["1024x80"], windows["1280x100"], windows["1537x120"], windows["3020x236"], windows["3328x260"]) == (3, 3, 3, 5, 5, 7, 9)
    assert (by["4000x5"].nw, by["4000x5"].nh, by["5x4000"].nw, by["5x4000"].nh) == (512, 1, 1, 512)
    assert (by["1285x650"].nw, by["1285x650"].nh) == (512, 258) and by["41x513"].nw == 40 and by["41x513"].nh == 512
    for g in ru.GEOMETRIES:
        if g.nw > 64:
            assert {32, 64}.issubset(g.seams_x) and g.src_x, g
        if g.nh > 32:
            assert {16, 32}.issubset(g.seams_y) and g.src_y, g
        target = ru.target_dimensions(g.w, g.h)
        assert (g.nw, g.nh) == target
    # the content stack holds what its names say, and its lone pixels are lone: at most one per window on either axis
    g = by["1537x120"]
    imgs, names = ru.content_stack(g)
    assert len(imgs) == len(names) >= 25 and not imgs[0].any() and (imgs[1] == 255).all()
    ax, ay = ru.build_axis(g.w, g.nw), ru.build_axis(g.h, g.nh)
    for k, name in enumerate(names):
        if name.startswith("seam pixels") and name.endswith("255 on 0"):
            ys, xs = (v.astype(np.int64) for v in np.nonzero(imgs[k]))
            assert len(xs) >= 8 and np.array_equal(imgs[k + 1], 255 - imgs[k])
            dx, dy = np.abs(xs[:, None] - xs[None, :]), np.abs(ys[:, None] - ys[None, :])
            apart = (dx >= 2 * ax.window) | ((dx == 0) & (dy >= 2 * ay.window)) | np.eye(len(xs), dtype=bool)
            assert apart.all(), name
    lit_x = set()
    for k, name in enumerate(names):
        if name.startswith("seam pixels") and name.endswith("255 on 0"):
            lit_x.update(np.nonzero(imgs[k])[1].tolist())
    for b in (32, 64, 480):  # first and last source column of the outputs on either side
        for o in (b - 1, b):
            assert {int(ax.start[o]), int(ax.start[o] + ax.size[o] - 1)} <= lit_x
    assert {0, g.w - 1} <= lit_x  # (windows the image edge truncates)
    assert len(ay.start) == 39
    c3 = ru.colour(imgs[-2:], 3)
    assert np.array_equal(c3[..., 1], imgs[-2:, :, ::-1]) and np.array_equal(c3[..., 2], imgs[-2:, ::-1, :]) and ru.colour(imgs[-2:], 4).shape[-1] == 4


@pytest.mark.parametrize("g", ru.GEOMETRIES, ids=ru.geometry_id)
def test_oracle_equals_restatement_on_every_geometry_and_content(oracle, g):
    imgs, names = ru.content_stack(g)
    for ch in (1, 3):  # (the colour spread has a luma of its own; Rgba8 has Rgb8's)
        luma = ru.to_luma601(ru.colour(imgs, ch))
        if ch == 3:
            assert np.array_equal(luma[-1], oracle.luma601(ru.colour(imgs[-1:], 3)[0]))
        want = ru.resize_box_u8(luma, g.nw, g.nh)
        got = np.stack([oracle.resize_box_u8(x, g.nw, g.nh) for x in luma])
        diff = ru.first_difference(got, want, names)
        assert diff is None, f"oracle (got) against restatement (want), {ru.geometry_id(g)} channels {ch}: {diff}"
    assert oracle.target_dimensions(g.w, g.h) == (g.nw, g.nh)
    assert oracle.resize_axis_info(g.w, g.nw) == ru.axis_info(g.w, g.nw) and oracle.resize_axis_info(g.h, g.nh) == ru.axis_info(g.h, g.nh)


def test_oracle_equals_restatement_at_every_source_size_from_513_to_4096(oracle):
    rng = np.random.default_rng(513)
    noise = rng.integers(0, 256, (3, 4096), dtype=np.uint8)
    stripes = ((np.arange(4096) & 1) * 255).astype(np.uint8)
    for in_size in range(513, 4097):
        img = noise[:, :in_size].copy()
        img[1] = stripes[:in_size]
        assert oracle.resize_axis_info(in_size, 512) == ru.axis_info(in_size, 512), in_size
        got, want = oracle.resize_box_u8(img, 512, 3), ru.resize_box_u8(img, 512, 3)
        assert np.array_equal(got, want), f"source width {in_size}: {ru.first_difference(got[None], want[None])}"
