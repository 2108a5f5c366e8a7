"""The frame rows of the fused 512x512 PDQ kernels (rupphash_amd/csrc/pdq_fused512.hip).  In bands 0 and 7 the scan divides the window
sums of rows 0..2 and 508..511 by their clipped window heights, and the 64-px kernels form that quotient for two neighbouring columns
per instruction.  The pictures here put full-range noise into exactly those rows -- neighbouring columns differ, so a pair whose halves
were swapped or duplicated changes the coefficients -- and keep the rows next to them (3 and 507) constant, where a quotient applied
to a row that has none would show.  One picture's frame is dark except in the first and last octet of every strip, where the scan
takes its first-octet and its last-columns paths.  Hash, quality and all 256 coefficient bit patterns must be the oracle's, for the
three kernels that share the scan (64-px strips, 128-px strips, eight waves per image) and for Luma8 input, at batch sizes 1, 3, 4."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FRAME_ROWS = np.r_[0:3, 508:512]
NEXT_ROWS = np.array([3, 507])


@pytest.fixture(scope="module")
def eng():
    from rupphash_amd import Engine

    e = Engine(0)
    yield e
    e.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _images(rng):
    """4 RGB pictures:
    0  noise everywhere, rows 3 and 507 constant
    1  flat interior (128), noisy frame rows, rows 3 and 507 constant at another level
    2  noise interior, frame rows dark except in the first and the last octet of every 64-px strip (and so of every 128-px strip)
    3  frame rows alternate 0 / 255 from column to column with the phase flipped from row to row, smooth interior"""
    imgs = np.empty((4, 512, 512, 3), np.uint8)
    imgs[0] = rng.integers(0, 256, (512, 512, 3), dtype=np.uint8)
    imgs[0][NEXT_ROWS] = 90
    imgs[1] = 128
    imgs[1][FRAME_ROWS] = rng.integers(0, 256, (FRAME_ROWS.size, 512, 3), dtype=np.uint8)
    imgs[1][NEXT_ROWS] = 201
    imgs[2] = rng.integers(0, 256, (512, 512, 3), dtype=np.uint8)
    x = np.arange(512)
    octet_ends = ((x % 64) < 8) | ((x % 64) >= 56)
    frame = rng.integers(128, 256, (FRAME_ROWS.size, 512, 3), dtype=np.uint8)
    frame[:, ~octet_ends] = 0
    imgs[2][FRAME_ROWS] = frame
    imgs[2][NEXT_ROWS] = 17
    yy, xx = np.mgrid[0:512, 0:512]
    imgs[3] = ((xx + 2 * yy) // 5 % 256).astype(np.uint8)[..., None]
    imgs[3][FRAME_ROWS] = (((xx[FRAME_ROWS] + yy[FRAME_ROWS]) & 1) * 255).astype(np.uint8)[..., None]
    imgs[3][NEXT_ROWS] = 64
    return imgs


@pytest.fixture(scope="module")
def pictures(oracle):
    """(rgb, gray, oracle features of each rgb picture, of each gray picture); computed once, never modified"""
    rng = np.random.default_rng(20261020)
    rgb = _images(rng)
    gray = np.ascontiguousarray(rgb[..., 1])
    for k, im in list(enumerate(rgb)) + list(enumerate(gray)):
        fr = im[FRAME_ROWS].reshape(FRAME_ROWS.size, 512, -1).astype(int)
        if k != 2:  # (picture 2's frame is dark between the octets at the strips' ends)
            assert (np.abs(np.diff(fr, axis=1)).sum(axis=2) > 0).mean() > 0.95, "neighbouring frame columns must differ"
        assert (im[NEXT_ROWS].reshape(2, -1) == im[NEXT_ROWS].reshape(2, -1)[:, :1]).all()
    f_rgb = [oracle.pdq_features(im) for im in rgb]
    f_gray = [oracle.pdq_features(im) for im in gray]
    # the frame rows reach the result: two neighbouring columns of a pair swapped in the frame rows alone change the coefficients
    for im, (_, c, _) in ((rgb[0], f_rgb[0]), (rgb[1], f_rgb[1]), (gray[3], f_gray[3])):
        sw = im.copy()
        sw[FRAME_ROWS, 22], sw[FRAME_ROWS, 23] = im[FRAME_ROWS, 23], im[FRAME_ROWS, 22]
        assert not np.array_equal(bits(oracle.pdq_features(sw)[1]), bits(c))
    for feats in (f_rgb, f_gray):
        assert len({bits(c).tobytes() for _, c, _ in feats}) == 4
    rgb.setflags(write=False)
    gray.setflags(write=False)
    return rgb, gray, f_rgb, f_gray


def _check(oracle, out, feats):
    for k, (rc, coeffs, q) in enumerate(feats):
        assert rc == 0 and out["valid"][k] == 1, k
        bad = np.nonzero(bits(out["coeffs"][k]) != bits(coeffs))[0]
        assert bad.size == 0, f"picture {k}: {bad.size} coefficients differ, the first at (row, column) {divmod(int(bad[0]), 16)}"
        assert np.array_equal(out["hash"][k], oracle.to_hash(coeffs)), f"hash differs for picture {k}"
        assert bits(out["quality"][k:k + 1])[0] == bits(np.float32(q))[()], f"quality differs for picture {k}"
        assert np.array_equal(out["dihedral"][k], oracle.dihedral_hashes(coeffs)), f"dihedral hashes differ for picture {k}"


def _run(eng, which, imgs):
    eng.set_pdq_kernel(which)
    try:
        return eng.pdq_hash_batch(imgs, want_quality=True, want_coeffs=True, want_dihedral=True)
    finally:
        eng.set_pdq_kernel(4)


SLICES = {"1": slice(0, 1), "3": slice(1, 4), "4": slice(0, 4)}


@pytest.mark.parametrize("batch", ["1", "3", "4"])
@pytest.mark.parametrize("which", [1, 2, 3])  # one wave per image with 64-px / 128-px strips, eight waves per image
def test_rgb8_frame_rows_match_oracle(eng, oracle, pictures, which, batch):
    rgb, _, feats, _ = pictures
    sl = SLICES[batch]
    _check(oracle, _run(eng, which, np.ascontiguousarray(rgb[sl])), feats[sl])


@pytest.mark.parametrize("batch", ["1", "3", "4"])
def test_luma8_frame_rows_match_oracle(eng, oracle, pictures, batch):
    _, gray, _, feats = pictures
    sl = SLICES[batch]
    _check(oracle, _run(eng, 1, np.ascontiguousarray(gray[sl])), feats[sl])


def test_single_pictures_one_by_one(eng, oracle, pictures):
    """every picture as a batch of its own through the default kernel choice"""
    rgb, gray, f_rgb, f_gray = pictures
    for k in range(4):
        _check(oracle, _run(eng, 4, np.ascontiguousarray(rgb[k:k + 1])), f_rgb[k:k + 1])
        _check(oracle, _run(eng, 4, np.ascontiguousarray(gray[k:k + 1])), f_gray[k:k + 1])
