"""The fused 512x512 PDQ kernel (rupphash_amd/csrc/pdq_fused512.hip) requests pixels long before it uses them: the whole image head
in one go (rows 0..3, the edge pixels of band 0, the first tile) and the edge pixels of band b + 1 while band b's column chain runs.
A request that delivered another band's or another image's pixels would go unnoticed on images whose frame columns are uniform, so
these batches give every band and every image its own frame columns and head rows.  Every output must be the oracle's, bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FRAME = np.r_[0:8, 504:512]  # the columns the edge pre-pass reads


@pytest.fixture(scope="module")
def eng():
    from rupphash_amd import Engine

    e = Engine(0)
    yield e
    e.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _band_distinct_images(rng):
    """3 images whose frame columns are random per row around a level that depends on the band (30 x band + 0..29); the interior is
    constant in the first image and random bytes in the other two"""
    imgs = np.empty((3, 512, 512, 3), np.uint8)
    imgs[0] = 128
    imgs[1:] = rng.integers(0, 256, (2, 512, 512, 3), dtype=np.uint8)
    level = (np.arange(512) // 64 * 30).astype(np.uint8)
    for k in range(3):
        imgs[k][:, FRAME] = level[:, None, None] + rng.integers(0, 30, (512, FRAME.size, 3), dtype=np.uint8)
    return imgs


def _head_distinct_images(rng):
    """6 images that share one random interior and differ only in rows 0..7 and in the frame columns (level 40 x image + 0..39)"""
    base = rng.integers(0, 256, (512, 512, 3), dtype=np.uint8)
    imgs = np.repeat(base[None], 6, axis=0)
    for k in range(6):
        imgs[k][:8] = 40 * k + rng.integers(0, 40, (8, 512, 3), dtype=np.uint8)
        imgs[k][:, FRAME] = 40 * k + rng.integers(0, 40, (512, FRAME.size, 3), dtype=np.uint8)
    return imgs


@pytest.fixture(scope="module")
def batches(oracle):
    """name -> (rgb images, gray images, oracle features of each); computed once, never modified"""
    rng = np.random.default_rng(20261018)
    out = {}
    for name, rgb in (("bands", _band_distinct_images(rng)), ("heads", _head_distinct_images(rng))):
        gray = np.ascontiguousarray(rgb[..., 1])
        out[name] = (rgb, gray, [oracle.pdq_features(im) for im in rgb], [oracle.pdq_features(im) for im in gray])
    # the batches tell a wrong band or a wrong image apart only if the right and the wrong pixels give different results
    feats = out["heads"][2]
    assert len({oracle.to_hash(c).tobytes() for _, c, _ in feats}) == len(feats)
    return out


def _check(oracle, out, feats, everything):
    for k, (rc, coeffs, q) in enumerate(feats):
        assert rc == 0 and out["valid"][k] == 1, k
        assert np.array_equal(out["hash"][k], oracle.to_hash(coeffs)), f"hash differs for image {k}"
        if everything:
            assert np.array_equal(bits(out["coeffs"][k]), bits(coeffs)), f"coefficients differ for image {k}"
            assert bits(out["quality"][k:k + 1])[0] == bits(np.float32(q))[()], k
            assert np.array_equal(out["dihedral"][k], oracle.dihedral_hashes(coeffs)), k


@pytest.mark.parametrize("name", ["bands", "heads"])
@pytest.mark.parametrize("which", [1, 2, 3])  # one wave per image (64- / 128-px strips), eight waves per image
def test_rgb8_matches_oracle(eng, oracle, batches, which, name):
    rgb, _, feats, _ = batches[name]
    everything = which == 1
    eng.set_pdq_kernel(which)
    try:
        out = eng.pdq_hash_batch(rgb, want_quality=everything, want_coeffs=everything, want_dihedral=everything)
    finally:
        eng.set_pdq_kernel(4)
    _check(oracle, out, feats, everything)


@pytest.mark.parametrize("name", ["bands", "heads"])
def test_luma8_matches_oracle(eng, oracle, batches, name):
    _, gray, _, feats = batches[name]
    eng.set_pdq_kernel(1)
    try:
        out = eng.pdq_hash_batch(gray, want_quality=True, want_coeffs=True, want_dihedral=True)
    finally:
        eng.set_pdq_kernel(4)
    _check(oracle, out, feats, True)


@pytest.mark.parametrize("which", [1, 2])
def test_padded_layout_matches_oracle(eng, oracle, batches, which):
    """the band-distinct images at row_stride 1540 (4 bytes of padding per row) with a gap between the images, everything around
    the pixels filled with 255: an early request formed from the wrong stride, or one that reads outside a row, changes a sum"""
    from rupphash_amd._lib import check

    rgb, _, feats, _ = batches["bands"]
    n = len(rgb)
    row_stride = 1540
    image_stride = row_stride * 512 + 4096
    buf = np.full(image_stride * n, 255, np.uint8)
    for k in range(n):
        rows = buf[k * image_stride: k * image_stride + 512 * row_stride].reshape(512, row_stride)
        rows[:, :1536] = rgb[k].reshape(512, 1536)
    out = {"hash": np.zeros((n, 32), np.uint8), "valid": np.zeros(n, np.uint8)}
    eng.set_pdq_kernel(which)
    try:
        check(eng.L.rph_pdq_hash_batch(eng.ctx, buf.ctypes.data, n, 512, 512, 3, row_stride, image_stride, out["hash"].ctypes.data,
                                       None, None, None, out["valid"].ctypes.data), "rph_pdq_hash_batch")
    finally:
        eng.set_pdq_kernel(4)
    _check(oracle, out, feats, False)


# ---- batch sizes around the number of waves the device holds at once (8 per CU): one, two, one less, exactly, one more, two rounds and a bit
FIRST_K = 77_000


@pytest.fixture(scope="module")
def resident(eng, oracle):
    """2 G + 5 device-synthesised images (G = 8 x CUs; 3.2 GB at 256 CUs) and their hashes by the generic kernel, computed once"""
    _, cus, _ = eng.device_info()
    g = 8 * cus
    n_max = 2 * g + 5
    d_img = eng.dev_alloc(n_max * 512 * 512 * 3)
    d_hash = eng.dev_alloc(n_max * 32)
    generic = np.zeros((n_max, 32), np.uint8)
    try:
        eng.synth_images_dev(d_img, FIRST_K, n_max)
        eng.set_pdq_kernel(0)
        try:
            eng.pdq_hash_batch_dev(d_img, n_max, 512, 512, 3, d_hash)
            eng.synchronize()
        finally:
            eng.set_pdq_kernel(4)
        eng.dev_download(generic, d_hash)
        yield {"g": g, "n_max": n_max, "d_img": d_img, "d_hash": d_hash, "generic": generic, "oracle": {}}
    finally:
        eng.dev_free(d_img)
        eng.dev_free(d_hash)


def _oracle_hash(oracle, cache, k):
    if k not in cache:
        cache[k] = oracle.pdq_batch_rgb(oracle.synth_images(FIRST_K + k, 1))[0][0]
    return cache[k]


@pytest.mark.parametrize("case", ["1", "2", "G-1", "G", "G+1", "2G+5"])
def test_grid_boundaries(eng, oracle, resident, case):
    g = resident["g"]
    n = {"1": 1, "2": 2, "G-1": g - 1, "G": g, "G+1": g + 1, "2G+5": 2 * g + 5}[case]
    n_max = resident["n_max"]
    eng.dev_memset(resident["d_hash"], 0xEE, n_max * 32)
    eng.set_pdq_kernel(1)
    try:
        eng.pdq_hash_batch_dev(resident["d_img"], n, 512, 512, 3, resident["d_hash"])
        eng.synchronize()
    finally:
        eng.set_pdq_kernel(4)
    got = np.zeros((n_max, 32), np.uint8)
    eng.dev_download(got, resident["d_hash"])
    assert np.array_equal(got[:n], resident["generic"][:n]), "fused and generic kernels disagree"
    assert (got[n:] == 0xEE).all(), "a hash was written beyond the batch"
    for k in sorted(set(range(min(32, n))) | set(range(max(0, n - 32), n))):
        assert np.array_equal(got[k], _oracle_hash(oracle, resident["oracle"], k)), f"hash of image {k} differs from the oracle"
