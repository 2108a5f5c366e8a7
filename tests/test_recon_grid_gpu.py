"""The grids of recon_grid.py on the device (-m gpu): the PNG unfilter kernel, the TIFF expand kernel and the WebP inverse transforms
and table slots at the rows, pixels and units where wave-shaped code goes wrong.  One test per group of files, so that a failure names
the kernel.  Every file: the device decode equals the plain Python reference byte for byte (dtype included) with the entropy /
decompress stage forced to the device and to the host; in a batch call its status is 0 and its pixel hash is the BLAKE3 of
to_rgba16(reference); every 8th of the files of at least 5 x 5 pixels has the oracle's PDQ hash, coefficients and quality on the reference
pixels.  The references (test_recon_grid_cpu.py pins them to libwebp, libpng and libtiff through Pillow) are computed once per file, the hashes of a group's files together.

GIF and BMP ride the same check on the seams of their own kernels (gif_expand_kernel, gif_lzw_kernel, bmp_expand_kernel; BMP has no
mode to force, so one pass), and each of their batch calls is made a second time straight after a call on one larger foreign file."""
import functools

import numpy as np
import pytest

import bmp_streams as bs
import gif_streams as gs
import recon_grid as rg
import png_util as pu
import tiff_util as tu

pytestmark = pytest.mark.gpu

HOST, DEVICE, AUTO = 0, 1, 2
SETTER = dict(png="png_set_inflate", tiff="tiff_set_decompress", webp="webp_set_entropy", gif="gif_set_decompress")  # (BMP has no mode: one pass)
_rgb = lambda img: np.ascontiguousarray(img[:, :, :3])
HASHER_PIXELS = dict(png=pu.hasher_pixels, tiff=tu.hasher_pixels, webp=_rgb, gif=_rgb, bmp=_rgb)
KEYS = ("hash", "quality", "valid", "status", "pixel_hash", "coeffs")


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


def _check_group(eng, oracle, fmt, items, foreign=None):
    """foreign: a file larger than the group with other content.  Each mode's batch call is made again straight after a call on it, when
    the buffers the pipeline keeps between calls hold its bytes behind every slot: the outputs must not change"""
    decode, batch = getattr(eng, f"{fmt}_decode"), getattr(eng, f"{fmt}_pdq_hash_batch")
    set_mode = getattr(eng, SETTER[fmt]) if fmt in SETTER else lambda mode: None
    files = [data for _, data, _, _ in items]
    outs = {}
    big = [k for k, item in enumerate(items) if min(item[2].shape[:2]) >= 5]
    pdq = set(big[::8])  # every 8th of the files PDQ takes
    assert len(pdq) == -(-len(big) // 8) and (pdq or not big)
    try:
        for mode in (DEVICE, HOST) if fmt in SETTER else (AUTO,):
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
            if foreign is not None:
                assert batch([foreign], want_coeffs=True, want_pixel_hash=True)["status"][0] == 0
                again = batch(files, want_coeffs=True, want_pixel_hash=True)
                for key in KEYS:
                    assert np.array_equal(again[key].view(np.uint8), out[key].view(np.uint8)), (key, mode)
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
    for key in KEYS:
        assert np.array_equal(outs[HOST][key].view(np.uint8), outs[DEVICE][key].view(np.uint8)), key


# ------------------------------------------------------------------ GIF and BMP
@functools.lru_cache(maxsize=None)
def _foreign(fmt):
    """one file with more decoded bytes than any group of the format's grid holds together, of content no grid file has"""
    most = max(sum(ref.nbytes for _, _, ref, _ in rg.references(fmt, group, hashes=False)) for group in rg.GRIDS[fmt][0]())
    side = int(np.ceil(np.sqrt(most / 4))) + 1
    if fmt == "bmp":
        return bs.make("bf8888a", side, side, seed=99)[0]
    # (a period of 251 x 256 indices, every row different: the encoder's table does the work, a file of a few dozen KiB)
    idx = (np.arange(side * side, dtype=np.int64) * 7 % 251 + np.arange(side * side) // 251 % 256) % 256
    return gs.image_gif(idx.reshape(side, side).astype(np.uint8), gs.colour_palette(256, 98))[0]


def _check_gif_group(eng, oracle, refs, group):
    items = refs("gif", group)
    outs = _check_group(eng, oracle, "gif", items, _foreign("gif"))
    for key in KEYS:  # decompressed on the host and on the device: the same outputs
        assert np.array_equal(outs[HOST][key].view(np.uint8), outs[DEVICE][key].view(np.uint8)), key
    return items, outs


def test_gif_expand_rows_past_one_trip_of_the_grid(eng, oracle, refs):
    """screens of 1023 .. 2049 rows (a wave's row loop takes 1024 rows a trip), plain and interlaced, the frame one row and 1020 rows
    down and clipped at the bottom, interlaced frames of 1024 .. 1031 rows; then the whole group in one call between two 5 x 5 files
    (the tallest screen sizes the grid for all of them) against every file in a call of its own"""
    items, outs = _check_gif_group(eng, oracle, refs, "expand_rows")
    small = items[0]
    assert small[0] == rg.GIF_SMALL and small[2].shape == (5, 5, 4)
    files = [data for _, data, _, _ in items] + [small[1]]
    eng.gif_set_decompress(DEVICE)
    try:
        mixed = eng.gif_pdq_hash_batch(files, want_coeffs=True, want_pixel_hash=True)
        for k, data in enumerate(files):
            alone = eng.gif_pdq_hash_batch([data], want_coeffs=True, want_pixel_hash=True)
            for key in KEYS:
                assert np.array_equal(mixed[key][k], alone[key][0]), ((items + [small])[k][0], key)
    finally:
        eng.gif_set_decompress(AUTO)
    for key in KEYS:
        assert np.array_equal(mixed[key][:-1], outs[DEVICE][key]) and np.array_equal(mixed[key][-1], mixed[key][0]), key


def test_gif_expand_frame_edges_on_and_beside_the_64_pixel_steps(eng, oracle, refs):
    """screens of 127 .. 130 px, the frame's left edge at 0, 1, 63, 64, 65 and its right edge at 63, 64, 65, 128, 129 and past the screen"""
    _check_gif_group(eng, oracle, refs, "expand_cols")


def test_gif_lzw_frames_on_both_sides_of_the_lds_switch(eng, oracle, refs):
    """frames of 16 383, 16 384 and 16 385 indices, of 16 369 .. 16 383 (the last 16-byte store of a frame built in LDS at every
    residue) and of 1 .. 33, noise over 4 and 256 colours with and without Clears"""
    _check_gif_group(eng, oracle, refs, "lzw_switch")


def test_gif_lzw_copies_that_carry_noise(eng, oracle, refs):
    """plain and KwKwK copies of 63 .. 129 bytes of noise in frames built in LDS and in global memory, last strings clipped by the
    frame's end (test_recon_grid_cpu.py shows what a wrong copy would write)"""
    _check_gif_group(eng, oracle, refs, "lzw_copies")


def test_bmp_expand_band_walk(eng, oracle, refs):
    """the sixteen variants in both row orders at the sizes where the band walk changes: eight trips, a last item of one row, the carry
    on every third trip, more groups than threads, more groups than an item holds"""
    _check_group(eng, oracle, "bmp", refs("bmp", "bands"), _foreign("bmp"))
