"""The BMP path on the device (-m gpu) on the files of tests/bmp_streams.py: rph_bmp_decode equals rph_bmp_decode_host byte for byte at
every depth, row order and the widths where the expand kernel's lanes, dwords and wave passes end; one batch call that mixes all variants,
sizes on both sides of the ragged kernels' 128 px, damaged and below-5-px files gives every file what it gets alone; the hashes are those
of Engine.image_hash_ragged, the CPU oracle and the numpy to_rgba16 + BLAKE3 on the host-decoded pixels; a BMP of a PNG's pixels has that
PNG's hashes."""
import functools

import numpy as np
import pytest

import bmp_streams as bs
import png_util as pu

pytestmark = pytest.mark.gpu

KEYS = ("hash", "quality", "coeffs", "dihedral", "valid", "status", "pixel_hash")
# bmp_kernels.hip: a lane turns PX_PER_LANE = 4 pixels into whole dwords at every depth, so one wave pass covers 64 * 4 pixels
WAVE_PASS_PIXELS = 64 * 4
WIDTHS = (1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, WAVE_PASS_PIXELS - 1, WAVE_PASS_PIXELS, WAVE_PASS_PIXELS + 1)
HEIGHTS = (1, 2, 5)


@pytest.fixture(scope="module")
def eng():
    from rupphash_amd import Engine

    e = Engine(0)
    yield e
    e.close()


def _batch(eng, files):
    return eng.bmp_pdq_hash_batch(files, want_coeffs=True, want_dihedral=True, want_pixel_hash=True)


@pytest.mark.parametrize("variant", bs.VARIANTS)
def test_device_decode_equals_host_decode_byte_for_byte(eng, variant):
    from rupphash_amd import Engine

    for td in bs.ROW_ORDERS:
        if td and variant.startswith("rle"):
            continue
        for h in HEIGHTS:
            for w in WIDTHS:
                data, px = bs.make(variant, w, h, td, seed=4)
                ref = Engine.bmp_decode_host(data)
                assert np.array_equal(ref, px), (variant, w, h, td)
                got = eng.bmp_decode(data)
                assert got.dtype == np.uint8 and got.shape == ref.shape and got.tobytes() == ref.tobytes(), (variant, w, h, td)


def test_every_file_of_the_writer_decodes_on_the_device_as_on_the_host(eng):
    """the header sizes, short palettes, odd mask sets and hand-written RLE streams (skipped pixels with a full palette among them: the
    plane of B G R rows)"""
    for name, data, px in bs.valid_files():
        assert eng.bmp_decode(data).tobytes() == px.tobytes(), name
    # several row bands per image: more rows than one work item covers
    for variant, w, h in (("rgb24", 37, 700), ("pal4", 1100, 9), ("bf565", 258, 70), ("rle8", 300, 40), ("bf8888a", 513, 33)):
        data, px = bs.make(variant, w, h, seed=9)
        assert eng.bmp_decode(data).tobytes() == px.tobytes(), variant


def test_load_bmp_is_the_device_decode(eng):
    from rupphash_amd import scanner

    data, px = bs.make("bf4444a", 21, 9, seed=2)
    got = scanner.load_bmp("x/shot.BMP", data, engine=eng)
    assert got.shape == (9, 21, 4) and np.array_equal(got, px)
    assert scanner.load_bmp("a.bmp", bs.make("pal1", 21, 9)[0], engine=eng).shape == (9, 21, 3)


def test_damaged_files_have_the_host_status(eng):
    from rupphash_amd import RphError

    for name, data, status in bs.damaged_files():
        with pytest.raises(RphError) as e:
            eng.bmp_decode(data)
        assert e.value.status == status, name


@functools.lru_cache(maxsize=None)
def mixed():
    """(name, data, status): every variant at a size the ragged kernels take (both sides >= 128) and at sizes of the per-geometry path,
    below-5-px files and damaged ones, interleaved"""
    big = [(128, 128), (131, 130), (300, 200), (129, 257)]
    small = [(1, 1), (4, 9), (9, 4), (64, 64), (127, 140), (33, 17)]
    out = []
    bad = bs.damaged_files()[::6]
    for k, v in enumerate(bs.VARIANTS):
        w, h = big[k % len(big)]
        out.append((f"{v}_{w}x{h}", bs.make(v, w, h, bool(k & 1), seed=k)[0], 0))
        w, h = small[k % len(small)]
        out.append((f"{v}_{w}x{h}", bs.make(v, w, h, not (k & 1), seed=k)[0], 0))
        if k < len(bad):
            out.append(bad[k])
    for w, h in ((2, 2), (1, 7), (300, 4)):
        out.append((f"rgb24_{w}x{h}", bs.make("rgb24", w, h)[0], 0))
    out.append(("two_of_one_size_a", bs.make("rgb24", 131, 130, seed=90)[0], 0))
    out.append(("two_of_one_size_b", bs.make("rgb24", 131, 130, seed=91)[0], 0))
    return out


def test_one_mixed_call_gives_every_file_what_it_gets_alone(eng):
    files = mixed()
    assert 50 <= len(files) <= 70 and sum(1 for f in files if f[2] != 0) >= 10
    alone = [_batch(eng, [d]) for _, d, _ in files]
    big = _batch(eng, [d for _, d, _ in files])
    small = 0
    for k, (name, data, status) in enumerate(files):
        assert big["status"][k] == status == alone[k]["status"][0], name
        for key in KEYS:
            assert np.array_equal(big[key][k], alone[k][key][0]), (name, key)
        if status != 0:  # damaged: zero outputs
            assert big["valid"][k] == 0 and big["quality"][k] == 0, name
            assert not (big["hash"][k].any() or big["pixel_hash"][k].any() or big["coeffs"][k].any() or big["dihedral"][k].any()), name
        else:
            w, h, _, _ = eng.bmp_info(data)
            if w < 5 or h < 5:  # valid but small: no PDQ hash, still a pixel hash
                small += 1
                assert big["valid"][k] == 0 and not big["hash"][k].any() and big["pixel_hash"][k].any(), name
            else:
                assert big["valid"][k] == 1, name
    assert small >= 5


def test_hashes_are_those_of_the_decoded_pixels(eng, oracle):
    """= Engine.image_hash_ragged on rph_bmp_decode_host's pixels, = the CPU oracle's PDQ, = numpy to_rgba16 + BLAKE3"""
    import blake3_util as b3
    from rupphash_amd import Engine

    good = [(n, d) for n, d, s in mixed() if s == 0]
    out = _batch(eng, [d for _, d in good])
    assert not out["status"].any()
    px = [Engine.bmp_decode_host(d) for _, d in good]
    ref = eng.image_hash_ragged(px, want_coeffs=True, want_dihedral=True, want_pixel_hash=True)
    for key in ("hash", "quality", "coeffs", "dihedral", "valid", "pixel_hash"):
        assert np.array_equal(np.asarray(out[key]).view(np.uint8), np.asarray(ref[key]).view(np.uint8)), key
    for k, ((name, _), p) in enumerate(zip(good, px)):
        assert out["pixel_hash"][k].tobytes() == b3.pixel_hash(p), name
        if p.shape[0] < 5 or p.shape[1] < 5:
            assert out["valid"][k] == 0
            continue
        rc, coeffs, q = oracle.pdq_features(p)
        assert rc == 0 and out["valid"][k] == 1, name
        assert out["coeffs"][k].tobytes() == coeffs.tobytes() and out["quality"][k].tobytes() == np.float32(q).tobytes(), name
        assert np.array_equal(out["hash"][k], oracle.to_hash(coeffs)) and np.array_equal(out["dihedral"][k], oracle.dihedral_hashes(coeffs)), name


@pytest.mark.parametrize("channels", [3, 4])
def test_bmp_of_a_pngs_pixels_has_the_pngs_hashes(eng, channels):
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:150, 0:170]
    px = np.stack([(xx * 3 + yy) % 256, (yy * 2 + xx // 3) % 256, (xx + yy) // 2 % 256, 255 - xx % 200][:channels], axis=-1).astype(np.uint8)
    px ^= rng.integers(0, 4, px.shape).astype(np.uint8)
    png = pu.encode(px, 2 if channels == 3 else 6, 8)
    if channels == 3:
        bmp = bs.bmp_file(40, 170, 150, 24, bs.BI_RGB, bs.pack_rows([r[:, ::-1].tobytes() for r in px], False))
    else:
        bits, masks = bs.MASKS["8888a"]
        v = (px[..., 0].astype(np.uint64) << np.uint64(16)) | (px[..., 1].astype(np.uint64) << np.uint64(8)) | px[..., 2].astype(np.uint64) | (px[..., 3].astype(np.uint64) << np.uint64(24))
        bmp = bs.bmp_file(124, 170, 150, 32, bs.BI_BITFIELDS, bs.pack_rows(bs.value_rows(v, 32), False), masks=masks)
    assert np.array_equal(eng.bmp_decode(bmp), px)
    a = eng.png_pdq_hash_batch([png], want_coeffs=True, want_dihedral=True, want_pixel_hash=True)
    b = _batch(eng, [bmp])
    assert a["status"][0] == 0 and b["status"][0] == 0 and a["valid"][0] == 1
    for key in KEYS:
        assert np.array_equal(a[key], b[key]), key


def test_release_and_empty_calls(eng):
    data = bs.make("rgb24", 140, 130, seed=1)[0]
    first = _batch(eng, [data])
    eng.bmp_release()
    again = _batch(eng, [data])
    for key in KEYS:
        assert np.array_equal(first[key], again[key]), key
    assert eng.L.rph_bmp_pdq_hash_batch(eng.ctx, None, None, 0, 0, None, None, None, None, None, None, None) == 0
    eng.bmp_release()
    eng.bmp_release()
