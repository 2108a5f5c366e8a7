"""TIFF files on the device (-m gpu): decode against the reference decoder of tiff_util, batch PDQ outputs against the CPU oracle on the
reference pixels, pixel hashes against a BLAKE3 of to_rgba16, the same results in every decompress mode and whatever shares a call, a
file of thousands of strips, and the cross-format case (a JPEG, the PNG and the TIFF of its decoded pixels)."""
import os

import numpy as np
import pytest

import blake3_util as b3
import jpeg_util as ju
import png_util as pu
import tiff_util as tu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from rupphash_amd import Engine

    e = Engine(0)
    yield e
    e.close()


def _check_pdq(oracle, out, k, img):
    px = tu.hasher_pixels(img)
    h, w = px.shape[:2]
    assert out["status"][k] == 0
    if w < 5 or h < 5:
        assert out["valid"][k] == 0 and not out["hash"][k].any()
        return
    rc, coeffs, q = oracle.pdq_features(px)
    assert rc == 0 and out["valid"][k] == 1
    assert np.array_equal(out["hash"][k], oracle.to_hash(coeffs))
    assert np.array_equal(out["coeffs"][k].view(np.uint32), coeffs.view(np.uint32))
    assert out["quality"][k] == np.float32(q)
    assert np.array_equal(out["dihedral"][k], oracle.dihedral_hashes(coeffs))


def test_decode_equals_reference_for_every_layout(eng):
    names = set()
    for mode in (1, 0):
        eng.tiff_set_decompress(mode)
        for name, data in tu.valid_corpus():
            st, ref = tu.decode(data)
            got = eng.tiff_decode(data)
            assert got.dtype == ref.dtype and np.array_equal(got, ref), (name, mode)
            names.add(name)
    eng.tiff_set_decompress(2)
    assert {"lzw_table_fills", "lzw_clear_mid_strip", "big_tile", "lzw_runs"} <= names
    assert any("_tile_be_" in n for n in names) and any("_strip_le_" in n for n in names) and any("_b1_" in n for n in names)


def test_batch_outputs_equal_oracle_on_reference_pixels(eng, oracle):
    corpus = tu.valid_corpus(8)
    files = [d for _, d in corpus]
    for mode in (0, 1, 2):
        eng.tiff_set_decompress(mode)
        out = eng.tiff_pdq_hash_batch(files, want_coeffs=True, want_dihedral=True, want_pixel_hash=True)
        for k, (name, data) in enumerate(corpus):
            _, ref = tu.decode(data)
            _check_pdq(oracle, out, k, ref)
            if k % 3 == 0 or ref.size <= 400:
                assert out["pixel_hash"][k].tobytes() == b3.blake3(tu.to_rgba16(ref)), name
    eng.tiff_set_decompress(2)


def test_sixteen_bit_and_photo_sized_images(eng, oracle):
    rng = np.random.default_rng(5)
    files, refs = [], []
    for photo, spp, bps, w, h, comp, pred, kw in [(2, 3, 16, 512, 512, 5, 2, dict(rows_per_strip=2)), (2, 4, 8, 512, 512, 8, 2, dict(tile=(128, 128))),
                                                 (1, 1, 16, 300, 200, 5, 2, dict(tile=(64, 64), bo=">")), (1, 2, 16, 64, 80, 32773, 1, dict(rows_per_strip=7)),
                                                 (0, 1, 4, 700, 90, 5, 1, dict(rows_per_strip=11)), (2, 3, 8, 512, 512, 5, 2, dict(rows_per_strip=5)),
                                                 (2, 3, 8, 512, 512, 1, 1, dict(rows_per_strip=16, bo=">"))]:
        data = tu.make_file(rng, w, h, photo, spp, bps, compression=comp, predictor=pred, **kw)
        files.append(data)
        refs.append(tu.decode(data)[1] if w * h <= 64 * 80 else None)
    for mode in (0, 1):
        eng.tiff_set_decompress(mode)
        out = eng.tiff_pdq_hash_batch(files, want_coeffs=True, want_dihedral=True, want_pixel_hash=True)
        for k, data in enumerate(files):
            img = eng.tiff_decode_host(data)
            assert np.array_equal(eng.tiff_decode(data), img)
            _check_pdq(oracle, out, k, img)
            one = eng.pixel_hash_batch(tu.hasher_pixels(img)[None]) if img.dtype == np.uint8 else None
            if one is not None:
                assert np.array_equal(out["pixel_hash"][k], one[0])
            if refs[k] is not None:
                assert out["pixel_hash"][k].tobytes() == b3.blake3(tu.to_rgba16(refs[k]))
    eng.tiff_set_decompress(2)


def test_scan_of_4000x3000_with_thousands_of_strips(eng, oracle):
    """one file, one call: 3000 strips of one row each (LZW + predictor), and the same pixels in 256x256 Deflate tiles"""
    yy, xx = np.mgrid[0:3000, 0:4000]
    rng = np.random.default_rng(41)
    img = np.stack([(xx // 3 + yy // 5 + 40 * c) % 256 for c in range(3)], axis=-1).astype(np.int64)
    img[::7, ::5] += rng.integers(0, 8, img[::7, ::5].shape)
    img %= 256
    import zlib

    cache = {}  # (the helper's LZW encoder is Python: rows that repeat are encoded once)
    strips = [cache.setdefault(raw, None) or cache.__setitem__(raw, tu.lzw_encode(raw)) or cache[raw] for raw, _ in tu.segment_rows(img, 8, predictor=2, rows_per_strip=1)]
    files = [tu.write(tu.base_tags(4000, 3000, 3, 8, 2, 5, 2, 1), strips)]
    tiles = [zlib.compress(raw, 1) for raw, _ in tu.segment_rows(img, 8, predictor=2, tile=(256, 256))]
    files.append(tu.write(tu.base_tags(4000, 3000, 3, 8, 2, 8, 2, None, (256, 256)), tiles, tiled=True))
    strips8 = [zlib.compress(raw, 1) for raw, _ in tu.segment_rows(img, 8, predictor=2, rows_per_strip=1)]
    files.append(tu.write(tu.base_tags(4000, 3000, 3, 8, 2, 32946, 2, 1), strips8))
    want = img.astype(np.uint8)
    rc, coeffs, q = oracle.pdq_features(want)
    for mode in (1, 0):
        eng.tiff_set_decompress(mode)
        out = eng.tiff_pdq_hash_batch(files, want_pixel_hash=True)
        assert not out["status"].any() and out["valid"].all()
        for k in range(len(files)):
            assert np.array_equal(out["hash"][k], oracle.to_hash(coeffs))
            assert np.array_equal(out["pixel_hash"][k], out["pixel_hash"][0])
        assert np.array_equal(eng.tiff_decode(files[-1]), want)
    eng.tiff_set_decompress(2)
    assert out["pixel_hash"][0].tobytes() == b3.blake3(tu.to_rgba16(want))


def test_modes_agree_on_damaged_files(eng):
    corpus = tu.damaged_corpus(seed=99, n_random=300)
    files = [d for _, d in corpus]
    outs = []
    for mode in (0, 1, 2):
        eng.tiff_set_decompress(mode)
        outs.append(eng.tiff_pdq_hash_batch(files, want_pixel_hash=True))
    eng.tiff_set_decompress(2)
    for k, (name, data) in enumerate(corpus):
        st, _ = tu.decode(data)
        assert outs[0]["status"][k] == st, name
        if st:
            assert not outs[0]["hash"][k].any() and not outs[0]["pixel_hash"][k].any()
    for o in outs[1:]:
        for key in ("hash", "quality", "valid", "status", "pixel_hash"):
            assert np.array_equal(o[key], outs[0][key]), key


def test_each_file_alone_as_in_a_mixed_call_of_3000(eng):
    rng = np.random.default_rng(17)
    valid = tu.valid_corpus(3)
    damaged = tu.damaged_corpus(seed=5, n_random=100)
    pool = [d for _, d in valid] + [d for _, d in damaged]
    files = [pool[int(i)] for i in rng.integers(0, len(pool), 3000)]
    eng.tiff_set_decompress(2)
    big = eng.tiff_pdq_hash_batch(files, want_pixel_hash=True)
    assert (big["status"] != 0).any() and (big["valid"] == 1).any()
    alone = {}
    for data in pool:
        alone[data] = eng.tiff_pdq_hash_batch([data], want_pixel_hash=True)
    for k, data in enumerate(files):
        a = alone[data]
        for key in ("hash", "quality", "valid", "status", "pixel_hash"):
            assert np.array_equal(big[key][k], a[key][0]), (k, key)


def test_call_larger_than_one_chunk(eng):
    rng = np.random.default_rng(23)
    small = [tu.make_file(rng, 6 + k % 5, 7, compression=(1, 5, 8, 32773)[k % 4]) for k in range(40)]
    files = [small[k % 40] for k in range(8192 + 300)]
    out = eng.tiff_pdq_hash_batch(files, want_pixel_hash=True)
    assert eng.debug_file_chunks("tiff")[0] == [8192, 300]
    ref = eng.tiff_pdq_hash_batch(small, want_pixel_hash=True)
    for key in ("hash", "quality", "valid", "status", "pixel_hash"):
        assert out[key].tobytes() == ref[key][np.arange(len(files)) % 40].tobytes(), key
    assert out["valid"].all() and not out["status"].any()


def test_below_five_pixels(eng):
    rng = np.random.default_rng(29)
    files = [tu.make_file(rng, w, h, compression=5) for w, h in [(4, 30), (30, 4), (1, 1), (5, 5)]]
    out = eng.tiff_pdq_hash_batch(files, want_pixel_hash=True)
    assert list(out["valid"]) == [0, 0, 0, 1] and not out["status"].any()
    assert not out["hash"][:3].any()
    for k, data in enumerate(files):
        assert out["pixel_hash"][k].tobytes() == b3.blake3(tu.to_rgba16(tu.decode(data)[1]))


def test_cross_format_pixel_hash_and_pdq_hash(eng):
    from rupphash_amd import scanner

    golden = open(os.path.join(os.path.dirname(__file__), "golden", "bench.jpg"), "rb").read()
    gray = ju.pillow_jpeg(ju.make_image(96, 80, "L", seed=3), quality=85)
    for jpg in (golden, gray):
        px = eng.jpeg_decode(jpg)
        jout = eng.jpeg_pdq_hash_batch([jpg], want_pixel_hash=True)
        assert jout["status"][0] == 0
        png = pu.encode(px, 2 if px.ndim == 3 else 0, 8, filters=1)
        rgb = px if px.ndim == 3 else np.repeat(px[:, :, None], 3, axis=2)
        changed = rgb.astype(np.int64) * 257
        changed[0, 0, 0] ^= 1  # one low byte
        tiffs = [tu.encode(px, compression=5, predictor=2, tile=(64, 48)),
                 tu.encode(px, compression=8, bo=">", rows_per_strip=3),
                 tu.encode(rgb.astype(np.int64) * 257, bps=16, compression=5, predictor=2, bo=">"),
                 tu.encode(changed, bps=16, compression=5, predictor=2)]
        pout = eng.png_pdq_hash_batch([png], want_pixel_hash=True)
        tout = eng.tiff_pdq_hash_batch(tiffs, want_pixel_hash=True)
        assert not tout["status"].any() and not pout["status"].any()
        j = jout["pixel_hash"][0]
        assert np.array_equal(pout["pixel_hash"][0], j)
        assert [np.array_equal(p, j) for p in tout["pixel_hash"]] == [True, True, True, False]
        # the hasher takes the pixels themselves in all three 8-bit files: one PDQ hash
        assert np.array_equal(tout["hash"][0], pout["hash"][0]) and np.array_equal(tout["hash"][1], pout["hash"][0])
        assert np.array_equal(tout["hash"][0], jout["hash"][0])
        content = eng.blake3_batch([jpg, png] + tiffs)
        pixel = [j, pout["pixel_hash"][0]] + list(tout["pixel_hash"])
        assert scanner.identical_duplicates(content, pixel) == [True, True, True, True, True, False]
        assert np.array_equal(eng.tiff_decode(tiffs[0]), px)
        assert np.array_equal(scanner.load_tiff("x.TIF", tiffs[0], engine=eng), px)
        assert np.array_equal(scanner.load_tiff("x.tiff", tiffs[1], engine=eng), px)
        with pytest.raises(ValueError):
            scanner.load_tiff("x.png", tiffs[0], engine=eng)
