"""BLAKE3 identity hashes on the GPU: rph_blake3_batch(_dev) on byte strings, rph_pixel_hash_batch(_dev) on decoded pixels and
rph_jpeg_pdq_pixel_hash_batch on JPEG files, each against the numpy restatement of the specification in tests/blake3_util.py."""
import io
import os

import numpy as np
import pytest

import blake3_util as b3
import jpeg_util as ju

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEY = b"whats the Elvish word for friend"
LENGTHS = sorted({0, 1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 16384, 31744, 102400}
                 | {k * 1024 + d for k in range(1, 10) for d in (-1, 1)})


@pytest.fixture(scope="module")
def eng():
    from rupphash_amd import Engine

    e = Engine(0)
    yield e
    e.jpeg_set_entropy(2)
    e.close()


def _hex(rows):
    return [bytes(r).hex() for r in rows]


@pytest.mark.parametrize("key", [None, KEY], ids=["hash", "keyed"])
def test_byte_strings_of_every_length_in_one_call(eng, key):
    rng = np.random.default_rng(11)
    lens = LENGTHS + [1 << 20, (1 << 20) + 1] + [int(x) for x in rng.integers(0, 3_000_000, 4)]
    strings = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lens]
    got = eng.blake3_batch(strings, key)
    assert _hex(got) == [b3.blake3(s, key).hex() for s in strings]


@pytest.mark.parametrize("key", [None, KEY], ids=["hash", "keyed"])
def test_ten_thousand_short_strings(eng, key):
    from rupphash_amd import Engine

    rng = np.random.default_rng(12)
    strings = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in rng.integers(0, 4097, 10_000)]
    got = eng.blake3_batch(strings, key)
    assert _hex(got) == [Engine.blake3_host(s, key).hex() for s in strings]  # host scalar: pinned to the helper by the CPU tests
    for i in rng.choice(len(strings), 100, replace=False):
        assert bytes(got[i]) == b3.blake3(strings[i], key)


def test_dev_form_with_offsets(eng):
    rng = np.random.default_rng(13)
    lens = [0, 5, 1024, 70000, 3, 131072, 131073, 0, 4096 * 64 + 17]
    blob = rng.integers(0, 256, 7 + sum(lens), dtype=np.uint8)
    off = np.concatenate([[7], 7 + np.cumsum(lens)]).astype(np.uint64)  # strings start at odd byte addresses
    d_data, d_off, d_dig = eng.dev_alloc(blob.nbytes), eng.dev_alloc(off.nbytes), eng.dev_alloc(32 * len(lens))
    try:
        eng.dev_upload(d_data, blob)
        eng.dev_upload(d_off, off)
        for key in (None, KEY):
            eng.blake3_batch_dev(d_data, d_off, len(lens), d_dig, key)
            eng.stream_synchronize()
            got = np.zeros((len(lens), 32), np.uint8)
            eng.dev_download(got, d_dig)
            want = [b3.blake3(blob[int(off[i]):int(off[i + 1])].tobytes(), key).hex() for i in range(len(lens))]
            assert _hex(got) == want
    finally:
        for p in (d_data, d_off, d_dig):
            eng.dev_free(p)


SIZES = [(1, 1), (5, 5), (128, 1), (129, 1), (127, 3), (513, 257), (512, 512), (1265, 850)]


@pytest.mark.parametrize("ch", [1, 3, 4], ids=["luma8", "rgb8", "rgba8"])
def test_pixel_hash_of_raw_pixels_with_padded_rows(eng, ch):
    rng = np.random.default_rng(20 + ch)
    for w, h in SIZES:
        n = 2
        pad = 5 + (w % 3)  # padded rows (odd stride) and a gap between images
        big = rng.integers(0, 256, (n, h + 1, w + pad, ch), dtype=np.uint8)
        view = big[:, :h, :w, :] if ch > 1 else big[:, :h, :w, 0]
        got = eng.pixel_hash_batch(view)
        for k in range(n):
            assert bytes(got[k]) == b3.pixel_hash(view[k]), (w, h, ch, k)
        packed = np.ascontiguousarray(view)
        assert np.array_equal(eng.pixel_hash_batch(packed), got)


def test_pixel_hash_dev_form(eng):
    rng = np.random.default_rng(30)
    w, h, ch, n, row, img = 300, 200, 3, 3, 300 * 3 + 12, (300 * 3 + 12) * 201
    buf = rng.integers(0, 256, n * img, dtype=np.uint8)
    d_px, d_h = eng.dev_alloc(buf.nbytes), eng.dev_alloc(32 * n)
    try:
        eng.dev_upload(d_px, buf)
        eng.pixel_hash_batch_dev(d_px, n, w, h, ch, d_h, row_stride=row, image_stride=img)
        eng.stream_synchronize()
        got = np.zeros((n, 32), np.uint8)
        eng.dev_download(got, d_h)
    finally:
        eng.dev_free(d_px)
        eng.dev_free(d_h)
    for k in range(n):
        im = np.lib.stride_tricks.as_strided(buf[k * img:], (h, w, ch), (row, ch, 1))
        assert bytes(got[k]) == b3.pixel_hash(im)


def test_pixel_hash_dev_on_two_caller_streams():
    """Images above 8192 px keep their group values in one scratch per context, shared by every caller stream.  On a fresh context
    the second geometry needs more of it, so it grows while the other stream may still be using it."""
    from rupphash_amd import Engine

    eng = Engine(0)
    rng = np.random.default_rng(35)
    sets = [rng.integers(0, 256, (4, 100, 120, 3), dtype=np.uint8), rng.integers(0, 256, (6, 130, 160, 4), dtype=np.uint8)]
    streams = [eng.stream_create(), eng.stream_create()]
    d_px = [eng.dev_alloc(s.nbytes) for s in sets]
    d_h = [eng.dev_alloc(len(s) * 32) for s in sets]
    try:
        for k in range(2):
            eng.dev_upload(d_px[k], sets[k])
        eng.synchronize()
        for rep in range(20):  # no host synchronisation between the launches
            for k in range(2):
                n, h, w, ch = sets[k].shape
                eng.pixel_hash_batch_dev(d_px[k], n, w, h, ch, d_h[k], stream=streams[k])
        for st in streams:
            eng.stream_synchronize(st)
        for k in range(2):
            got = np.zeros((len(sets[k]), 32), np.uint8)
            eng.dev_download(got, d_h[k])
            for i in range(len(sets[k])):
                assert bytes(got[i]) == b3.pixel_hash(sets[k][i]), (k, i)
    finally:
        for p in d_px + d_h:
            eng.dev_free(p)
        for st in streams:
            eng.stream_destroy(st)
        eng.close()


def test_scanner_pixel_hash(eng):
    from rupphash_amd import scanner

    im = np.random.default_rng(31).integers(0, 256, (40, 70, 3), dtype=np.uint8)
    assert scanner.pixel_hash(im, eng) == b3.pixel_hash(im)


def _jpeg_files():
    from PIL import Image

    files = [open(os.path.join(GOLDEN, n), "rb").read() for n in sorted(os.listdir(GOLDEN)) if n.endswith(".jpg")]
    for i, ss in enumerate([2, 1, 0]):  # 4:2:0, 4:2:2, 4:4:4
        files.append(ju.pillow_jpeg(ju.make_image(97 + 8 * i, 61, seed=100 + i), quality=85, subsampling=ss))
        files.append(ju.pillow_jpeg(ju.make_image(130, 90 + i, seed=110 + i), quality=80, subsampling=ss, progressive=True))
    files.append(ju.encode_baseline(np.array(ju.make_image(120, 64, seed=120)), ((1, 2), (1, 1), (1, 1)), 1.0, 0))  # 4:4:0
    files.append(ju.pillow_jpeg(ju.make_image(77, 45, "L", seed=121), quality=90))                                   # grey
    files.append(ju.pillow_jpeg(ju.make_image(90, 70, "L", seed=122), quality=90, progressive=True))
    files.append(ju.pillow_jpeg(ju.make_image(160, 90, seed=123), quality=60, restart_marker_blocks=2))              # restart intervals
    files.append(ju.encode_baseline(np.array(ju.make_image(97, 61, seed=124)), ((2, 2), (1, 1), (1, 1)), 0.7, 3))
    files.append(ju.pillow_jpeg(Image.fromarray(np.asarray(ju.make_image(512, 512, seed=125))), quality=90, subsampling=2))  # fused-kernel geometry
    files.append(ju.pillow_jpeg(ju.make_image(1265, 850, seed=126), quality=90, subsampling=2))                       # photo, pre-downsampled
    files.append(ju.pillow_jpeg(ju.make_image(3, 3, seed=127), quality=90))                                           # below 5 px
    files.append(b"\xff\xd8 this is not a JPEG")                                                                       # corrupt
    return files


@pytest.mark.parametrize("flavour", [0, 1], ids=["zune", "libjpeg"])
def test_jpeg_pixel_hash_in_every_entropy_mode(eng, flavour):
    files = _jpeg_files()
    i_tiny, i_bad = len(files) - 2, len(files) - 1
    want = {}
    for i, data in enumerate(files[:i_bad]):
        px = eng.jpeg_decode(data, flavour)
        want[i] = b3.pixel_hash(px)
        if flavour == 1:
            assert want[i] == b3.pixel_hash(ju.pillow_decode(data)), i  # independent of the project's decoder
    kw = dict(flavour=flavour, threads=4, want_quality=True, want_coeffs=True, want_dihedral=True)
    for mode in (0, 1, 2, 3):
        eng.jpeg_set_entropy(mode)
        plain = eng.jpeg_pdq_hash_batch(files, **kw)
        out = eng.jpeg_pdq_hash_batch(files, want_pixel_hash=True, **kw)
        assert "pixel_hash" not in plain
        for k in ("hash", "quality", "coeffs", "dihedral", "valid", "status"):
            assert out[k].tobytes() == plain[k].tobytes(), (mode, k)
        for i in range(i_bad):
            assert out["status"][i] == 0 and bytes(out["pixel_hash"][i]) == want[i], (mode, i)
        assert out["status"][i_bad] != 0 and not out["pixel_hash"][i_bad].any()
        assert out["valid"][i_tiny] == 0 and out["status"][i_tiny] == 0
    eng.jpeg_set_entropy(2)


def test_jpeg_pixel_hash_large_call(eng):
    from PIL import Image

    rng = np.random.default_rng(40)
    base = []
    for k in range(200):
        w, h = int(rng.integers(8, 160)), int(rng.integers(8, 120))
        im = Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) if k % 5 == 0 else ju.make_image(w, h, "L" if k % 7 == 0 else "RGB", seed=k)
        base.append(ju.pillow_jpeg(im, quality=70 + k % 25, subsampling=k % 3 if im.mode == "RGB" else 0, progressive=k % 9 == 4))
    files = base * 100  # 20 000 files: host chunks (4096 files) and device sub-batches turn over
    lst = eng.jpeg_file_list(files)
    for mode in (2, 0):
        eng.jpeg_set_entropy(mode)
        plain = eng.jpeg_pdq_hash_batch(lst, want_quality=True)
        out = eng.jpeg_pdq_hash_batch(lst, want_quality=True, want_pixel_hash=True)
        for k in ("hash", "quality", "valid", "status"):
            assert out[k].tobytes() == plain[k].tobytes(), (mode, k)
        assert (out["status"] == 0).all()
        ph = out["pixel_hash"].reshape(100, 200, 32)
        assert (ph == ph[0][None]).all()  # every copy of a file has its hash, wherever it fell in the call
        for i in rng.choice(200, 25, replace=False):
            assert bytes(ph[0][i]) == b3.pixel_hash(eng.jpeg_decode(base[i])), (mode, i)
    eng.jpeg_set_entropy(2)
