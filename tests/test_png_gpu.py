"""PNG files on the device (-m gpu): decode against the reference decoder of png_util, batch PDQ outputs against the CPU oracle on the
reference pixels, pixel hashes against a BLAKE3 of to_rgba16, the same results in every inflate mode and whatever shares a call, and the
cross-format case of the pixel hash (a JPEG and the PNG of its decoded pixels)."""
import io

import numpy as np
import pytest

import blake3_util as b3
import jpeg_util as ju
import png_util as pu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from rupphash_amd import Engine

    e = Engine(0)
    yield e
    e.close()


def _check_pdq(oracle, out, k, img):
    px = pu.hasher_pixels(img)
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
    for name, data in pu.valid_corpus():
        st, ref = pu.decode(data)
        got = eng.png_decode(data)
        assert got.dtype == ref.dtype and np.array_equal(got, ref), name
        names.add(name)
    assert {"adam7_1x1", "adam7_3x7", "adam7_9x1"} <= names


def test_batch_outputs_equal_oracle_on_reference_pixels(eng, oracle):
    corpus = pu.valid_corpus(8)
    files = [d for _, d in corpus]
    for mode in (0, 1, 2):
        eng.png_set_inflate(mode)
        out = eng.png_pdq_hash_batch(files, want_coeffs=True, want_dihedral=True, want_pixel_hash=True)
        for k, (name, data) in enumerate(corpus):
            _, ref = pu.decode(data)
            _check_pdq(oracle, out, k, ref)
            if k % 3 == 0 or ref.size <= 400:
                assert out["pixel_hash"][k].tobytes() == b3.blake3(pu.to_rgba16(ref)), name
    eng.png_set_inflate(2)


def test_sixteen_bit_and_photo_sized_images(eng, oracle):
    rng = np.random.default_rng(5)
    files, refs = [], []
    for ct, d, w, h in [(2, 16, 512, 512), (6, 8, 512, 512), (0, 16, 300, 200), (4, 16, 64, 80), (3, 8, 700, 90), (2, 8, 512, 512)]:
        s = pu.random_samples(rng, h, w, ct, d)
        pal = rng.integers(0, 256, (256, 3)) if ct == 3 else None
        data = pu.encode(s, ct, d, palette=pal, filters=[0, 1, 2, 3, 4], level=6)
        files.append(data)
        refs.append(pu.decode(data)[1] if w * h <= 64 * 80 else None)
    for mode in (0, 1):
        eng.png_set_inflate(mode)
        out = eng.png_pdq_hash_batch(files, want_coeffs=True, want_dihedral=True, want_pixel_hash=True)
        for k, data in enumerate(files):
            img = eng.png_decode_host(data)
            assert np.array_equal(eng.png_decode(data), img)
            _check_pdq(oracle, out, k, img)
            one = eng.pixel_hash_batch(pu.hasher_pixels(img)[None]) if img.dtype == np.uint8 else None
            if one is not None:
                assert np.array_equal(out["pixel_hash"][k], one[0])
            if refs[k] is not None:
                assert out["pixel_hash"][k].tobytes() == b3.blake3(pu.to_rgba16(refs[k]))
    eng.png_set_inflate(2)


def test_modes_agree_on_damaged_files(eng):
    corpus = pu.damaged_corpus(seed=99, n_random=300)
    files = [d for _, d in corpus]
    outs = []
    for mode in (0, 1, 2):
        eng.png_set_inflate(mode)
        outs.append(eng.png_pdq_hash_batch(files, want_pixel_hash=True))
    eng.png_set_inflate(2)
    for k, (name, data) in enumerate(corpus):
        st, _ = pu.decode(data)
        assert outs[0]["status"][k] == st, name
        if st:
            assert not outs[0]["hash"][k].any() and not outs[0]["pixel_hash"][k].any()
    for o in outs[1:]:
        for key in ("hash", "quality", "valid", "status", "pixel_hash"):
            assert np.array_equal(o[key], outs[0][key]), key


def test_each_file_alone_as_in_a_mixed_call_of_3000(eng):
    rng = np.random.default_rng(17)
    valid = pu.valid_corpus(3)
    damaged = pu.damaged_corpus(seed=5, n_random=100)
    pool = [d for _, d in valid] + [d for _, d in damaged]
    files = [pool[int(i)] for i in rng.integers(0, len(pool), 3000)]
    eng.png_set_inflate(2)
    big = eng.png_pdq_hash_batch(files, want_pixel_hash=True)
    assert (big["status"] != 0).any() and (big["valid"] == 1).any()
    alone = {}
    for data in pool:
        alone[data] = eng.png_pdq_hash_batch([data], want_pixel_hash=True)
    for k, data in enumerate(files):
        a = alone[data]
        for key in ("hash", "quality", "valid", "status", "pixel_hash"):
            assert np.array_equal(big[key][k], a[key][0]), (k, key)


def test_call_larger_than_one_chunk(eng):
    rng = np.random.default_rng(23)
    small = [pu.make_file(rng, 6 + k % 5, 7, 2, 8, False) for k in range(40)]
    files = [small[k % 40] for k in range(8192 + 300)]
    out = eng.png_pdq_hash_batch(files, want_pixel_hash=True)
    assert eng.debug_file_chunks("png")[0] == [8192, 300]
    ref = eng.png_pdq_hash_batch(small, want_pixel_hash=True)
    for key in ("hash", "quality", "valid", "status", "pixel_hash"):
        assert out[key].tobytes() == ref[key][np.arange(len(files)) % 40].tobytes(), key
    assert out["valid"].all() and not out["status"].any()


def test_below_five_pixels(eng):
    rng = np.random.default_rng(29)
    files = [pu.make_file(rng, w, h, 2, 8, False) for w, h in [(4, 30), (30, 4), (1, 1), (5, 5)]]
    out = eng.png_pdq_hash_batch(files, want_pixel_hash=True)
    assert list(out["valid"]) == [0, 0, 0, 1] and not out["status"].any()
    assert not out["hash"][:3].any()
    for k, data in enumerate(files):
        assert out["pixel_hash"][k].tobytes() == b3.blake3(pu.to_rgba16(pu.decode(data)[1]))


def test_cross_format_pixel_hash(eng):
    from rupphash_amd import scanner

    golden = open(__import__("os").path.join(__import__("os").path.dirname(__file__), "golden", "bench.jpg"), "rb").read()
    gray = ju.pillow_jpeg(ju.make_image(96, 80, "L", seed=3), quality=85)
    for jpg in (golden, gray):
        px = eng.jpeg_decode(jpg)
        jout = eng.jpeg_pdq_hash_batch([jpg], want_pixel_hash=True)
        assert jout["status"][0] == 0
        rgb = px if px.ndim == 3 else np.repeat(px[:, :, None], 3, axis=2)
        a16 = rgb.astype(np.int64) * 257
        changed = a16.copy()
        changed[0, 0, 0] ^= 1  # one low byte
        pngs = [pu.encode(px, 2 if px.ndim == 3 else 0, 8, filters=1),
                pu.encode(np.concatenate([rgb, np.full(rgb.shape[:2] + (1,), 255)], axis=2), 6, 8, filters=2),
                pu.encode(a16, 2, 16, filters=0),
                pu.encode(changed, 2, 16, filters=0)]
        pout = eng.png_pdq_hash_batch(pngs, want_pixel_hash=True)
        assert not pout["status"].any()
        j = jout["pixel_hash"][0]
        assert [np.array_equal(p, j) for p in pout["pixel_hash"]] == [True, True, True, False]
        files = [jpg] + pngs
        content = eng.blake3_batch(files)
        pixel = [j] + list(pout["pixel_hash"])
        assert scanner.identical_duplicates(content, pixel) == [True, True, True, True, False]
        assert np.array_equal(eng.png_decode(pngs[0]), px)
        assert np.array_equal(scanner.load_png("x.png", pngs[0], engine=eng), px)
