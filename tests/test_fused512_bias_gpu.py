"""The fused 512x512 PDQ kernels carry their luma rows biased (f16 1024 + y), run the edge pre-pass on the packed f16 pairs and
fold the factor 8 into the frame bands' division constants (rupphash_amd/csrc/pdq_fused512.hip).  Every output must still be the
oracle's, bit for bit, on the contents that reach the limits of that arithmetic: V = 2040 (the f16 limit), the extremes of
v - hist_b in the window slide, the frame rows and columns, the zero rows beyond the image, and padded layouts."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 5  # images per batch: the geometry is fixed, what can go wrong is content and layout


@pytest.fixture(scope="module")
def eng():
    from rupphash_amd import Engine

    e = Engine(0)
    yield e
    e.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _pattern_images():
    """all 0, all 255, rows alternating 0 / 255 with periods 1 and 8, and a 255 frame (rows 0-3, 508-511, columns 0-7, 504-511) on 0"""
    y = np.arange(512)
    black = np.zeros((512, 512, 3), np.uint8)
    white = np.full((512, 512, 3), 255, np.uint8)
    alt1 = np.broadcast_to(((y & 1) * 255).astype(np.uint8)[:, None, None], (512, 512, 3)).copy()
    alt8 = np.broadcast_to((((y >> 3) & 1) * 255).astype(np.uint8)[:, None, None], (512, 512, 3)).copy()
    frame = np.zeros((512, 512, 3), np.uint8)
    frame[:4] = 255
    frame[508:] = 255
    frame[:, :8] = 255
    frame[:, 504:] = 255
    return np.stack([black, white, alt1, alt8, frame])


@pytest.fixture(scope="module")
def batches(oracle):
    """name -> (rgb images, gray images, oracle features of each); computed once, never modified"""
    rng = np.random.default_rng(20261017)
    noise = rng.integers(0, 256, (2, 512, 512, 3), dtype=np.uint8)
    mixed = np.concatenate([noise, oracle.synth_images(0, 3)])  # random bytes + the first images of the synthetic sequence
    out = {}
    for name, rgb in (("patterns", _pattern_images()), ("mixed", mixed)):
        assert rgb.shape == (N, 512, 512, 3)
        gray = np.ascontiguousarray(rgb[..., 1])
        out[name] = (rgb, gray, [oracle.pdq_features(im) for im in rgb], [oracle.pdq_features(im) for im in gray])
    return out


def _check(oracle, out, feats, everything):
    for k, (rc, coeffs, q) in enumerate(feats):
        assert rc == 0 and out["valid"][k] == 1, k
        assert np.array_equal(out["hash"][k], oracle.to_hash(coeffs)), f"hash differs for image {k}"
        if everything:
            assert np.array_equal(bits(out["coeffs"][k]), bits(coeffs)), f"coefficients differ for image {k}"
            assert bits(out["quality"][k:k + 1])[0] == bits(np.float32(q))[()], k
            assert np.array_equal(out["dihedral"][k], oracle.dihedral_hashes(coeffs)), k


@pytest.mark.parametrize("name", ["patterns", "mixed"])
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


@pytest.mark.parametrize("name", ["patterns", "mixed"])
def test_luma8_matches_oracle(eng, oracle, batches, name):
    _, gray, _, feats = batches[name]
    eng.set_pdq_kernel(1)
    try:
        out = eng.pdq_hash_batch(gray, want_quality=True, want_coeffs=True, want_dihedral=True)
    finally:
        eng.set_pdq_kernel(4)
    _check(oracle, out, feats, True)


@pytest.mark.parametrize("name", ["patterns", "mixed"])
def test_padded_layout_matches_oracle(eng, oracle, batches, name):
    """row_stride 1540 (4 bytes of padding per row) and a gap between the images, everything around the pixels filled with 255:
    a read outside a row would change a sum"""
    from rupphash_amd._lib import check

    rgb, _, feats, _ = batches[name]
    row_stride = 1540
    image_stride = row_stride * 512 + 4096
    buf = np.full(image_stride * N, 255, np.uint8)
    for k in range(N):
        rows = buf[k * image_stride: k * image_stride + 512 * row_stride].reshape(512, row_stride)
        rows[:, :1536] = rgb[k].reshape(512, 1536)
    out = {"hash": np.zeros((N, 32), np.uint8), "valid": np.zeros(N, np.uint8)}
    eng.set_pdq_kernel(1)
    try:
        check(eng.L.rph_pdq_hash_batch(eng.ctx, buf.ctypes.data, N, 512, 512, 3, row_stride, image_stride, out["hash"].ctypes.data,
                                       None, None, None, out["valid"].ctypes.data), "rph_pdq_hash_batch")
    finally:
        eng.set_pdq_kernel(4)
    _check(oracle, out, feats, False)
