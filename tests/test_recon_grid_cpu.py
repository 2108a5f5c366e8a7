"""The grids of recon_grid.py, host half (no GPU).  The GPU tests compare the device with the plain Python decoders of png_util,
tiff_util and webp_util, so those are pinned first: every WebP file against libwebp (Pillow), modes 14 and 15 included, every PNG file
Pillow returns at full precision, every TIFF layout libtiff opens.  Then the host decoders against the references byte for byte on
every file.  (The ASan + UBSan host runs of test_png_cpu, test_tiff_cpu and test_webp_cpu take grid files as further inputs.)

WebP grid 1 is thinned by mode to keep the corpus build short: every mode 0 .. 15 keeps 2 x 66, 64 x 66, 65 x 66, 129 x 66,
65 x 65 and 65 x 129; each of 1 x 66, 3 x 66, 63 x 66, 127 x 66, 128 x 66, 65 x 1, 65 x 2 and 65 x 64 is written for four of the sixteen modes
(recon_grid.WEBP_THINNED)."""
import io

import numpy as np
import pytest

import recon_grid as rg

# PNG layouts Pillow hands back at the file's full precision (it narrows the other 16-bit layouts to 8 bits): layout -> Pillow mode
PNG_PILLOW = {"gray8": "L", "gray1": "L", "gray2": "L", "gray4": "L", "palette8": "RGB", "graya8": "LA", "rgb8": "RGB", "rgba8": "RGBA", "gray16": "I;16"}
# TIFF layouts (sample layout - byte order) not compared with libtiff: Pillow refuses to open them or hands them back at 8 bits
TIFF_NOT_COMPARED = ["graya16-II", "graya16-MM",  # Pillow cannot identify the file
                     "rgb16-II", "rgb16-MM", "rgba16-II", "rgba16-MM"]  # Pillow opens them as 8-bit RGB / RGBA


def _groups(fmt):
    return list(rg.GRIDS[fmt][0]())


def _open(data):
    Image = pytest.importorskip("PIL.Image")
    im = Image.open(io.BytesIO(data))
    im.load()
    return im


def test_grids_are_seeded_and_hold_the_cases():
    png, tiff, webp = rg.png_grid(), rg.tiff_grid(), rg.webp_grid()
    assert png is rg.png_grid() and tiff is rg.tiff_grid() and webp is rg.webp_grid()  # built once
    names = {n for g in (png, tiff, webp) for files in g.values() for n, _ in files}
    assert sum(len(f) for g in (png, tiff, webp) for f in g.values()) == len(names)
    for layout, _, _ in rg.PNG_LAYOUTS:
        for f in range(5):
            assert {f"{layout}-f{f}-{w}x{h}" for w in rg.PNG_WIDTHS for h in rg.PNG_ROWS} <= names
    assert len(png["pairs"]) == 2 * 2 * 25 and len(png["adam7"]) == 3 * 3 * 8 + 2
    for m in range(16):
        assert {f"mode{m}-{w}x{h}" for w, h in rg.WEBP_KEPT} <= names
    for w, h in rg.WEBP_THINNED:
        assert sum(f"mode{m}-{w}x{h}" in names for m in range(16)) == 4
    for w, h in ((65, 1), (65, 2), (65, 64), (65, 65), (65, 129), (1, 66), (2, 66), (3, 66), (63, 66), (64, 66), (65, 66), (127, 66), (128, 66), (129, 66)):
        assert (w, h) in rg.WEBP_KEPT + rg.WEBP_THINNED  # every size of grid 1 is written for some mode
    slots = rg.webp_slot_counts()  # (read from the kernel's sources: the four cache sizes give four slot counts, all below 7 groups)
    assert len(set(slots.values())) == 4 and slots[0] > slots[9] > slots[10] > slots[11] >= 2 and slots[0] < 7
    assert {n for n, _ in webp["slots"]} == {f"slots-groups{g}-cache{cb}" for g in (4, 7, 9) for cb in slots}
    for n_groups in (4, 7, 9):
        for n_slots in slots.values():
            ent = rg.slot_map(n_groups, n_slots, 90)
            assert set(ent) == set(range(n_groups))
            if n_groups > n_slots:  # groups of one slot follow each other, and come back after the slot has held another
                assert sum(a != b and a % n_slots == b % n_slots for a, b in zip(ent, ent[1:])) >= 3 * (n_groups - n_slots)


@pytest.mark.parametrize("group", _groups("webp"))
def test_webp_reference_equals_libwebp(group):
    for name, data, ref, _ in rg.references("webp", group, hashes=False):
        pil = np.asarray(_open(data))
        assert pil.shape == ref.shape and np.array_equal(pil, ref), name


@pytest.mark.parametrize("group", _groups("png"))
def test_png_reference_equals_pillow_where_pillow_keeps_the_precision(group):
    compared = 0
    for name, data, ref, _ in rg.references("png", group, hashes=False):
        mode = PNG_PILLOW.get(name.split("-")[0])
        if mode is None:
            continue
        im = _open(data)
        if im.mode != mode:
            assert im.mode in ("1", "P") or (mode == "I;16" and im.mode.startswith("I;16")), (name, im.mode)
            if not im.mode.startswith("I;16"):
                im = im.convert(mode)
        got = np.asarray(im)
        assert got.shape == ref.shape and np.array_equal(got.astype(np.int64), ref.astype(np.int64)), name
        compared += 1
    assert compared >= len(rg.png_grid()[group]) // 3


@pytest.mark.parametrize("group", _groups("tiff"))
def test_tiff_reference_equals_libtiff_for_every_layout_it_opens(group):
    for name, data, ref, _ in rg.references("tiff", group, hashes=False):
        if rg.tiff_layout(name) in TIFF_NOT_COMPARED:
            try:  # (the list holds only what Pillow cannot open or narrows)
                assert np.asarray(_open(data)).dtype.itemsize < ref.dtype.itemsize, name
            except OSError:
                pass
            continue
        im = _open(data)
        got = np.asarray(im.convert("L") if im.mode == "1" else im)
        assert got.dtype.itemsize == ref.dtype.itemsize, (name, im.mode)
        assert got.shape == ref.shape and np.array_equal(got.astype(np.int64), ref.astype(np.int64)), (name, im.mode)


def test_tiff_not_compared_list_is_short_and_named():
    layouts = {rg.tiff_layout(n) for files in rg.tiff_grid().values() for n, _ in files}
    assert set(TIFF_NOT_COMPARED) <= layouts
    for must in ("gray8", "rgb8", "rgba8", "gray16"):
        for bo in ("II", "MM"):
            assert f"{must}-{bo}" in layouts and f"{must}-{bo}" not in TIFF_NOT_COMPARED


@pytest.mark.parametrize("fmt,group", [(fmt, g) for fmt in rg.GRIDS for g in _groups(fmt)])
def test_host_decoder_equals_reference(fmt, group):
    from rupphash_amd import Engine

    host = getattr(Engine, f"{fmt}_decode_host")
    for name, data, ref, _ in rg.references(fmt, group, hashes=False):
        got = host(data)
        assert got.dtype == ref.dtype and got.shape == ref.shape and np.array_equal(got, ref), name
