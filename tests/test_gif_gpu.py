"""The GIF path on the device (-m gpu) on the corpora of tests/gif_streams.py: with decompression forced to the device rph_gif_decode equals
rph_gif_decode_host byte for byte and the statuses of damaged files are the host's; one batch call that mixes good, damaged, unsupported
and below-5-px files gives every file what it gets alone, in the HOST, DEVICE and AUTO modes; PDQ outputs equal rph_pdq_hash_batch and
pixel hashes rph_pixel_hash_batch on the decoded Rgba8 pixels; a GIF of a palette PNG's pixels has that PNG's hashes."""
import functools

import numpy as np
import pytest

import gif_streams as gs
import png_util as pu

pytestmark = pytest.mark.gpu

HOST, DEVICE, AUTO = 0, 1, 2
KEYS = ("hash", "quality", "coeffs", "dihedral", "valid", "status", "pixel_hash")


@pytest.fixture(scope="module")
def eng():
    from rupphash_amd import Engine

    e = Engine(0)
    yield e
    e.gif_set_decompress(AUTO)
    e.close()


@functools.lru_cache(maxsize=None)
def good_files():
    """(name, data) of every valid file: Pillow's, the helper's (frame widths 63, 64, 65, interlaced heights 1 .. 9 and 67 among them)"""
    return list(gs.pillow_files()) + [(n, d) for n, d, _ in gs.valid_files()]


@functools.lru_cache(maxsize=None)
def host_pixels():
    from rupphash_amd import Engine

    return [Engine.gif_decode_host(d) for _, d in good_files()]


def _batch(eng, files, mode):
    eng.gif_set_decompress(mode)
    return eng.gif_pdq_hash_batch(files, want_coeffs=True, want_dihedral=True, want_pixel_hash=True)


def test_device_decode_equals_host_decode_byte_for_byte(eng):
    assert len(good_files()) >= 80
    eng.gif_set_decompress(DEVICE)
    for (name, data), ref in zip(good_files(), host_pixels()):
        got = eng.gif_decode(data)
        assert got.dtype == np.uint8 and got.shape == ref.shape and got.tobytes() == ref.tobytes(), name


def test_load_gif_is_the_device_decode(eng):
    from rupphash_amd import scanner

    name, data = good_files()[0]
    assert np.array_equal(scanner.load_gif("x/" + name + ".GIF", data, engine=eng), host_pixels()[0])


@pytest.mark.parametrize("mode", [HOST, DEVICE, AUTO])
def test_damaged_files_have_the_host_status(eng, mode):
    from rupphash_amd import RphError

    eng.gif_set_decompress(mode)
    for name, data, status in gs.damaged_files():
        with pytest.raises(RphError) as e:
            eng.gif_decode(data)
        assert e.value.status == status, name


@functools.lru_cache(maxsize=None)
def mixed():
    """good (below-5-px ones among them), damaged and unsupported files, interleaved: (name, data, status)"""
    good, bad = good_files(), gs.damaged_files()
    out = []
    for k in range(max(len(good), len(bad))):
        if k < len(good):
            out.append(good[k] + (0,))
        if k < len(bad):
            out.append(bad[k])
    return out


@pytest.fixture(scope="module")
def alone(eng):
    """every file of the mixed call sent alone, decompressed on the device"""
    return [_batch(eng, [data], DEVICE) for _, data, _ in mixed()]


@pytest.mark.parametrize("mode", [HOST, DEVICE, AUTO])
def test_one_mixed_call_gives_every_file_what_it_gets_alone(eng, alone, mode):
    files = mixed()
    assert sum(1 for f in files if f[2] == gs.INVALID) >= 25 and sum(1 for f in files if f[2] == gs.UNSUPPORTED) >= 8
    big = _batch(eng, [d for _, d, _ in files], mode)
    small = 0
    for k, (name, data, status) in enumerate(files):
        assert big["status"][k] == status, name
        for key in KEYS:
            assert np.array_equal(big[key][k], alone[k][key][0]), (name, key)
        if status != 0:  # damaged: zero outputs
            assert big["valid"][k] == 0 and big["quality"][k] == 0, name
            assert not (big["hash"][k].any() or big["pixel_hash"][k].any() or big["coeffs"][k].any() or big["dihedral"][k].any()), name
        else:
            w, h, _, _ = eng.gif_info(data)
            if w < 5 or h < 5:  # valid but small: no PDQ hash, still a pixel hash
                small += 1
                assert big["valid"][k] == 0 and not big["hash"][k].any() and big["pixel_hash"][k].any(), name
            else:
                assert big["valid"][k] == 1, name
    assert small >= 5


def test_hashes_are_those_of_the_decoded_pixels(eng, oracle):
    """hash, quality, coefficients and dihedral = rph_pdq_hash_batch, pixel hashes = rph_pixel_hash_batch, on the Rgba8 pixels; files with
    a side above 512 px (pre-downsampled from Rgba8 rows at the screen's pitch) are held to the CPU oracle on the host-decoded pixels too"""
    out = _batch(eng, [d for _, d in good_files()], DEVICE)
    assert not out["status"].any()
    large = [k for k, px in enumerate(host_pixels()) if max(px.shape[:2]) > 512]
    assert sorted(host_pixels()[k].shape[:2] for k in large) == [(90, 700), (600, 1024), (700, 90)]
    for k in large:
        name = good_files()[k][0]
        rc, coeffs, q = oracle.pdq_features(host_pixels()[k])
        assert rc == 0 and out["valid"][k] == 1, name
        assert out["coeffs"][k].tobytes() == coeffs.tobytes(), name
        assert out["quality"][k].tobytes() == np.float32(q).tobytes(), name
        assert np.array_equal(out["hash"][k], oracle.to_hash(coeffs)) and np.array_equal(out["dihedral"][k], oracle.dihedral_hashes(coeffs)), name
    for k, ((name, _), px) in enumerate(zip(good_files(), host_pixels())):
        assert np.array_equal(out["pixel_hash"][k], eng.pixel_hash_batch(px[None])[0]), name
        ref = eng.pdq_hash_batch(px[None], want_coeffs=True, want_dihedral=True)
        assert out["valid"][k] == ref["valid"][0] == (px.shape[0] >= 5 and px.shape[1] >= 5), name
        if not ref["valid"][0]:
            continue
        assert np.array_equal(out["hash"][k], ref["hash"][0]), name
        assert out["quality"][k].tobytes() == ref["quality"][0].tobytes(), name
        assert out["coeffs"][k].tobytes() == ref["coeffs"][0].tobytes(), name
        assert np.array_equal(out["dihedral"][k], ref["dihedral"][0]), name


@pytest.mark.parametrize("interlace", [False, True])
def test_gif_of_a_palette_png_has_the_pngs_hashes(eng, interlace):
    rng = np.random.default_rng(5)
    pal = gs.colour_palette(64, 77)
    yy, xx = np.mgrid[0:70, 0:90]
    idx = ((xx // 7 + yy // 5 + rng.integers(0, 2, (70, 90))) % 64).astype(np.uint8)
    png = pu.encode(idx, 3, 8, palette=pal)
    gif, px = gs.image_gif(idx, pal, interlace=interlace)
    assert np.array_equal(px[:, :, :3], pal[idx]) and (px[:, :, 3] == 255).all()
    a = eng.png_pdq_hash_batch([png], want_coeffs=True, want_dihedral=True, want_pixel_hash=True)
    for mode in (HOST, DEVICE):
        b = _batch(eng, [gif], mode)
        assert a["status"][0] == 0 and b["status"][0] == 0 and a["valid"][0] == 1
        for key in KEYS:
            assert np.array_equal(a[key], b[key]), key
