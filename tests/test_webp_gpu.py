"""Lossless WebP files on the device (-m gpu): decode against the reference decoder of webp_util, batch PDQ outputs against the CPU
oracle on the reference pixels, pixel hashes against a BLAKE3 of to_rgba16, the same results in every entropy mode and whatever shares
a call, a 4000 x 3000 file, a file of hundreds of entropy groups, and the cross-format case (a JPEG, the PNG, the TIFF and the WebP of
its decoded pixels)."""
import os

import numpy as np
import pytest

import blake3_util as b3
import jpeg_util as ju
import png_util as pu
import tiff_util as tu
import webp_util as wu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from rupphash_amd import Engine

    e = Engine(0)
    yield e
    e.close()


def _check_pdq(oracle, out, k, img):
    h, w = img.shape[:2]
    assert out["status"][k] == 0
    if w < 5 or h < 5:
        assert out["valid"][k] == 0 and not out["hash"][k].any()
        return
    rc, coeffs, q = oracle.pdq_features(np.ascontiguousarray(img[:, :, :3]))
    assert rc == 0 and out["valid"][k] == 1
    assert np.array_equal(out["hash"][k], oracle.to_hash(coeffs))
    assert np.array_equal(out["coeffs"][k].view(np.uint32), coeffs.view(np.uint32))
    assert out["quality"][k] == np.float32(q)
    assert np.array_equal(out["dihedral"][k], oracle.dihedral_hashes(coeffs))


def test_decode_equals_reference_for_every_feature(eng):
    names = set()
    for mode in (1, 0):
        eng.webp_set_entropy(mode)
        for name, data in wu.valid_corpus():
            st, ref = wu.decode(data)
            got = eng.webp_decode(data)
            assert got.dtype == ref.dtype and got.shape == ref.shape and np.array_equal(got, ref), (name, mode)
            names.add(name)
    eng.webp_set_entropy(2)
    assert {"overlap_distance_1_and_below_64", "copy_ends_on_last_pixel", "groups_300", "four_transforms_with_palette", "size_16384x1", "distance_code_120"} <= names


def test_batch_outputs_equal_oracle_on_reference_pixels(eng, oracle):
    corpus = wu.valid_corpus(3)
    files = [d for _, d in corpus]
    for mode in (0, 1, 2):
        eng.webp_set_entropy(mode)
        out = eng.webp_pdq_hash_batch(files, want_coeffs=True, want_dihedral=True, want_pixel_hash=True)
        for k, (name, data) in enumerate(corpus):
            _, ref = wu.decode(data)
            _check_pdq(oracle, out, k, ref)
            assert out["pixel_hash"][k].tobytes() == b3.blake3(wu.to_rgba16(ref)), name
    eng.webp_set_entropy(2)


def test_4000x3000_and_hundreds_of_groups(eng, oracle):
    """one photo-sized file through subtract-green with a colour cache, 300 groups and copies of 4096 pixels from 256000
    pixels back (its rows repeat every 64, so the helper's writer finds them), and one 1024 x 700 file through predictor, cross-colour and subtract-green, whose rows
    are wider than one wave's reach"""
    yy, xx = np.mgrid[0:64, 0:4000]
    band = np.stack([(xx // 3 + yy // 5 + 40 * c + (xx * yy) % 7) % 256 for c in range(3)], axis=-1).astype(np.uint8)
    img = np.ascontiguousarray(np.tile(band, (47, 1, 1))[:3000])
    big = wu.encode(img, [("green",)], cache_bits=5, refs="lz", meta_bits=7, n_groups=300, seed=9)
    rng = np.random.default_rng(3)
    wide = wu.photo(rng, 1024, 700)
    files, want = [big, wu.encode(wide, [("predictor", 4, "mixed"), ("cross", 5), ("green",)], seed=10)], [img, wide]
    for mode in (1, 0):
        eng.webp_set_entropy(mode)
        out = eng.webp_pdq_hash_batch(files, want_pixel_hash=True)
        for k in range(2):
            rc, coeffs, q = oracle.pdq_features(want[k])
            assert out["status"][k] == 0 and out["valid"][k] == 1
            assert np.array_equal(out["hash"][k], oracle.to_hash(coeffs))
            assert out["pixel_hash"][k].tobytes() == b3.blake3(wu.to_rgba16(want[k]))
            assert np.array_equal(eng.webp_decode(files[k]), want[k])
    eng.webp_set_entropy(2)


def test_modes_agree_on_damaged_files(eng):
    corpus = wu.damaged_corpus(seed=99, n_random=300)
    files = [d for _, d in corpus]
    outs = []
    for mode in (0, 1, 2):
        eng.webp_set_entropy(mode)
        outs.append(eng.webp_pdq_hash_batch(files, want_pixel_hash=True))
    eng.webp_set_entropy(2)
    for k, (name, data) in enumerate(corpus):
        st, _ = wu.decode(data)
        assert outs[0]["status"][k] == st, name
        if st:
            assert not outs[0]["hash"][k].any() and not outs[0]["pixel_hash"][k].any()
    for o in outs[1:]:
        for key in ("hash", "quality", "valid", "status", "pixel_hash"):
            assert np.array_equal(o[key], outs[0][key]), key


def test_each_file_alone_as_in_a_mixed_call_of_3000(eng):
    rng = np.random.default_rng(17)
    valid = wu.valid_corpus(3)
    damaged = wu.damaged_corpus(seed=5, n_random=100)
    pool = [d for _, d in valid] + [d for _, d in damaged]
    files = [pool[int(i)] for i in rng.integers(0, len(pool), 3000)]
    alone = {}
    for mode in (2, 1):
        eng.webp_set_entropy(mode)
        big = eng.webp_pdq_hash_batch(files, want_pixel_hash=True)
        assert (big["status"] != 0).any() and (big["valid"] == 1).any()
        for data in pool:
            if data not in alone:
                alone[data] = eng.webp_pdq_hash_batch([data], want_pixel_hash=True)
        for k, data in enumerate(files):
            a = alone[data]
            for key in ("hash", "quality", "valid", "status", "pixel_hash"):
                assert np.array_equal(big[key][k], a[key][0]), (k, key, mode)
    eng.webp_set_entropy(2)


def test_below_five_pixels(eng):
    files = [d for n, d in wu.valid_corpus() if n in ("size_1x1", "size_4x4", "size_5x5")]
    out = eng.webp_pdq_hash_batch(files, want_pixel_hash=True)
    assert list(out["valid"]) == [0, 0, 1] and not out["status"].any()
    for k, data in enumerate(files):
        assert out["pixel_hash"][k].tobytes() == b3.blake3(wu.to_rgba16(wu.decode(data)[1]))


def test_cross_format_pixel_hash_and_pdq_hash(eng):
    golden = open(os.path.join(os.path.dirname(__file__), "golden", "bench.jpg"), "rb").read()
    px = eng.jpeg_decode(golden)
    assert px.ndim == 3
    jout = eng.jpeg_pdq_hash_batch([golden], want_pixel_hash=True)
    pout = eng.png_pdq_hash_batch([pu.encode(px, 2, 8, filters=1)], want_pixel_hash=True)
    tout = eng.tiff_pdq_hash_batch([tu.encode(px, compression=5, predictor=2, tile=(64, 48))], want_pixel_hash=True)
    changed = px.copy()
    changed[0, 0, 0] ^= 1
    webps = [wu.encode(px, [("green",), ("predictor", 4, "mixed")], refs="lz", cache_bits=6), wu.encode(px, form="vp8x"), wu.encode(changed)]
    for mode in (1, 0):
        eng.webp_set_entropy(mode)
        wout = eng.webp_pdq_hash_batch(webps, want_pixel_hash=True)
        assert not wout["status"].any() and jout["status"][0] == 0 and pout["status"][0] == 0 and tout["status"][0] == 0
        j = jout["pixel_hash"][0]
        assert np.array_equal(pout["pixel_hash"][0], j) and np.array_equal(tout["pixel_hash"][0], j)
        assert [np.array_equal(p, j) for p in wout["pixel_hash"]] == [True, True, False]
        for other in (jout, pout, tout):
            assert np.array_equal(wout["hash"][0], other["hash"][0]) and np.array_equal(wout["hash"][1], other["hash"][0])
        assert np.array_equal(eng.webp_decode(webps[0]), px)
    eng.webp_set_entropy(2)
