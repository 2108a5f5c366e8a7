"""The grids of recon_grid.py on the device (-m gpu): the PNG unfilter kernel, the TIFF expand kernel and the WebP inverse transforms
and table slots at the rows, pixels and units where wave-shaped code goes wrong.  One test per group of files, so that a failure names
the kernel.  Every file: the device decode equals the plain Python reference byte for byte (dtype included) with the entropy /
decompress stage forced to the device and to the host; in a batch call its status is 0 and its pixel hash is the BLAKE3 of
to_rgba16(reference); every 8th of the files of at least 5 x 5 pixels has the oracle's PDQ hash, coefficients and quality on the reference
pixels.  The references (test_recon_grid_cpu.py pins them to libwebp, libpng and libtiff through Pillow) are computed once per file, the hashes of a group's files together."""
import numpy as np
import pytest

import recon_grid as rg
import png_util as pu
import tiff_util as tu

pytestmark = pytest.mark.gpu

HOST, DEVICE, AUTO = 0, 1, 2
SETTER = dict(png="png_set_inflate", tiff="tiff_set_decompress", webp="webp_set_entropy")
HASHER_PIXELS = dict(png=pu.hasher_pixels, tiff=tu.hasher_pixels, webp=lambda img: np.ascontiguousarray(img[:, :, :3]))


@pytest.fixture(scope="module")
def eng():
    from rupphash_amd import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def refs():
    """(format, group) -> [(name, file, reference pixels, BLAKE3 of to_rgba16)], decoded by the Python decoders once"""
    return rg.references


def _check_group(eng, oracle, fmt, items):
    decode, batch, set_mode = getattr(eng, f"{fmt}_decode"), getattr(eng, f"{fmt}_pdq_hash_batch"), getattr(eng, SETTER[fmt])
    files = [data for _, data, _, _ in items]
    outs = {}
    big = [k for k, item in enumerate(items) if min(item[2].shape[:2]) >= 5]
    pdq = set(big[::8])  # every 8th of the files PDQ takes
    assert len(pdq) == -(-len(big) // 8) and (pdq or not big)
    try:
        for mode in (DEVICE, HOST):
            set_mode(mode)
            for name, data, ref, _ in items:
                got = decode(data)
                assert got.dtype == ref.dtype and got.shape == ref.shape and np.array_equal(got, ref), (name, mode)
            out = outs[mode] = batch(files, want_coeffs=True, want_pixel_hash=True)
            assert not out["status"].any(), [items[k][0] for k in np.flatnonzero(out["status"])]
            for k, (name, data, ref, digest) in enumerate(items):
                assert out["pixel_hash"][k].tobytes() == digest, (name, mode)
                if k in pdq:
                    rc, coeffs, q = oracle.pdq_features(HASHER_PIXELS[fmt](ref))
                    assert rc == 0 and out["valid"][k] == 1, (name, mode)
                    assert np.array_equal(out["hash"][k], oracle.to_hash(coeffs)), (name, mode)
                    assert np.array_equal(out["coeffs"][k].view(np.uint32), coeffs.view(np.uint32)), (name, mode)
                    assert out["quality"][k] == np.float32(q), (name, mode)
    finally:
        set_mode(AUTO)
    return outs


@pytest.mark.parametrize("layout", [l[0] for l in rg.PNG_LAYOUTS])
def test_png_unfilter_one_filter_type_on_every_row(eng, oracle, refs, layout):
    """filter types 0 .. 4 x 1, 63, 64, 65 and 129 rows x 1, 3 and 65 pixels, one case per sample layout (units of 1 .. 8 bytes): lane
    0's row above (from memory, all zero for row 0) against every other lane's (from a shuffle)"""
    items = refs("png", "filters", layout=layout)
    assert len(items) >= 75
    _check_group(eng, oracle, "png", items)


def test_png_unfilter_every_pair_of_filter_types_across_rows_63_64_and_127_128(eng, oracle, refs):
    _check_group(eng, oracle, "png", refs("png", "pairs"))


def test_png_unfilter_adam7_passes_of_65_and_33_rows(eng, oracle, refs):
    _check_group(eng, oracle, "png", refs("png", "adam7"))


def test_tiff_expand_predictor_2_in_strips(eng, oracle, refs):
    """1 .. 4 samples x 8 and 16 bits x both byte orders at 1 .. 193 pixels: the scan across the wave and the carry between steps"""
    _check_group(eng, oracle, "tiff", refs("tiff", "pred2_strips"))


def test_tiff_expand_predictor_2_in_tiles(eng, oracle, refs):
    """tiles of 16, 64, 80, 128 and 144 pixels with a cropped edge tile: the carry starts again in every tile row"""
    _check_group(eng, oracle, "tiff", refs("tiff", "pred2_tiles"))


def test_tiff_expand_packed_gray_and_sixteen_bit(eng, oracle, refs):
    _check_group(eng, oracle, "tiff", refs("tiff", "pred1"))


def test_webp_predictor_each_mode_0_to_15(eng, oracle, refs):
    """one mode per file around the 64-pixel window of lane 0 (T, TL, TR; TR of the last column) and the 64-row groups"""
    _check_group(eng, oracle, "webp", refs("webp", "predictor_single"))


def test_webp_predictor_modes_mixed_per_block(eng, oracle, refs):
    """block edges inside, on and across the 64-row and 64-pixel boundaries (block bits 2, 5, 6, 7 and 9)"""
    _check_group(eng, oracle, "webp", refs("webp", "predictor_mixed"))


def test_webp_cross_colour_sign_extremes(eng, oracle, refs):
    _check_group(eng, oracle, "webp", refs("webp", "cross"))


def test_webp_colour_indexing_packed_widths_from_1(eng, oracle, refs):
    _check_group(eng, oracle, "webp", refs("webp", "palette"))


def test_webp_table_slots_shared_by_groups_in_turn(eng, oracle, refs):
    """more groups than LDS table slots, the groups of one slot taking turns, with and without a colour cache; host and device entropy
    decoding give the same outputs"""
    outs = _check_group(eng, oracle, "webp", refs("webp", "slots"))
    for key in ("hash", "quality", "valid", "status", "pixel_hash", "coeffs"):
        assert np.array_equal(outs[HOST][key].view(np.uint8), outs[DEVICE][key].view(np.uint8)), key
