"""The multi-pass PDQ kernels (csrc/pdq_kernels.hip: box_rows_tiled_kernel -> box_cols_kernel -> box_rows_tiled_kernel<0, true> ->
tail_sampled_kernel, and their plain one-thread-per-line form) at their tile, window and sample seams: the geometries and contents of
tests/box_grid.py, bit for bit against the CPU oracle -- hash, quality, all 256 coefficients, the 8 dihedral hashes and `valid`."""
import ctypes as C

import numpy as np
import pytest

import box_grid as bg

pytestmark = pytest.mark.gpu

KEYS = ("hash", "quality", "coeffs", "dihedral", "valid")


@pytest.fixture(scope="module")
def eng():
    from rupphash_amd import Engine

    e = Engine(0)
    yield e
    e.set_pdq_kernel(4)
    e.close()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def reference(oracle, imgs):
    """the oracle's five outputs for every image of `imgs` (any size the library takes: the oracle resizes above 512 px as the reference does)"""
    n = len(imgs)
    ref = {"hash": np.zeros((n, 32), np.uint8), "quality": np.zeros(n, np.float32), "coeffs": np.zeros((n, 256), np.float32),
           "dihedral": np.zeros((n, 8, 32), np.uint8), "valid": np.ones(n, np.uint8)}
    for k in range(n):
        rc, c, q = oracle.pdq_features(imgs[k])
        assert rc == 0
        ref["coeffs"][k], ref["quality"][k] = c, np.float32(q)
        ref["hash"][k], ref["dihedral"][k] = oracle.to_hash(c), oracle.dihedral_hashes(c)
    return ref


def take(ref, idx):
    return {k: v[idx] for k, v in ref.items()}


def hold(out, ref, what):
    """every output array identical to the reference's, bit for bit; names the first image that differs"""
    for key in KEYS:
        a, b = bits(out[key]), bits(ref[key])
        if not np.array_equal(a, b):
            bad = np.nonzero((a != b).reshape(len(a), -1).any(axis=1))[0]
            pytest.fail(f"{what}: {key} differs for images {bad[:16].tolist()} ({len(bad)} of {len(a)})")


def hash_host(eng, buf, n, w, h, ch, row_stride, image_stride, full=True):
    """rph_pdq_hash_batch on a caller's byte buffer; full = False: every optional output pointer null"""
    from rupphash_amd._lib import check

    out = {"hash": np.zeros((n, 32), np.uint8), "quality": np.zeros(n, np.float32), "coeffs": np.zeros((n, 256), np.float32),
           "dihedral": np.zeros((n, 8, 32), np.uint8), "valid": np.zeros(n, np.uint8)}
    opt = [out[k].ctypes.data if full else None for k in KEYS[1:]]
    check(eng.L.rph_pdq_hash_batch(eng.ctx, buf.ctypes.data, n, w, h, ch, row_stride, image_stride, out["hash"].ctypes.data, *opt), "rph_pdq_hash_batch")
    return out


def hash_packed(eng, imgs, full=True):
    n, h, w = imgs.shape[:3]
    ch = 1 if imgs.ndim == 3 else imgs.shape[3]
    return hash_host(eng, np.ascontiguousarray(imgs), n, w, h, ch, w * ch, w * h * ch, full)


def hash_dev(eng, buf, lead, n, w, h, ch, row_stride, image_stride):
    """rph_pdq_hash_batch_dev on the uploaded bytes, `lead` bytes into the allocation; all five outputs"""
    sizes = {"hash": 32, "quality": 4, "coeffs": 1024, "dihedral": 256, "valid": 1}
    out = {"hash": np.zeros((n, 32), np.uint8), "quality": np.zeros(n, np.float32), "coeffs": np.zeros((n, 256), np.float32),
           "dihedral": np.zeros((n, 8, 32), np.uint8), "valid": np.zeros(n, np.uint8)}
    d_px, d_out = eng.dev_alloc(buf.nbytes), eng.dev_alloc(n * 2048)
    try:
        eng.dev_upload(d_px, buf)
        ptr, at = {}, 0
        for k in ("coeffs", "dihedral", "hash", "quality", "valid"):  # (descending alignment)
            ptr[k], at = d_out + at, at + n * sizes[k]
        eng.pdq_hash_batch_dev(d_px + lead, n, w, h, ch, ptr["hash"], ptr["quality"], ptr["coeffs"], ptr["dihedral"], ptr["valid"], row_stride=row_stride,
                               image_stride=image_stride)
        eng.synchronize()
        for k in KEYS:
            eng.dev_download(out[k], ptr[k])
    finally:
        eng.dev_free(d_px)
        eng.dev_free(d_out)
    return out


# ---- 2. the grid --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", bg.GRID_WIDTHS)
def test_grid_matches_oracle(eng, oracle, w):
    """every height the grid pairs with this width, 8 contents each: the tiled form (5) and the plain form (0) against the oracle, each once
    more with every optional output pointer null, and the default (4) against the tiled form"""
    try:
        for h in bg.grid_heights(w):
            imgs = bg.contents(np.random.default_rng(w * 1009 + h), h, w)
            ref = reference(oracle, imgs)
            got = {}
            for which in (5, 0):
                eng.set_pdq_kernel(which)
                got[which] = hash_packed(eng, imgs)
                hold(got[which], ref, f"{w}x{h} under rph_pdq_set_kernel {which}")
                bare = hash_packed(eng, imgs, full=False)
                assert np.array_equal(bare["hash"], ref["hash"]), f"{w}x{h} under {which}, hash only"
            eng.set_pdq_kernel(4)
            hold(hash_packed(eng, imgs), got[5], f"{w}x{h}: the default against the tiled form")
    finally:
        eng.set_pdq_kernel(4)


@pytest.mark.parametrize("ch", [3, 4])
@pytest.mark.parametrize("i", range(len(bg.COLOUR_GRID)), ids=[f"{w}x{h}" for w, h in bg.COLOUR_GRID])
def test_colour_grid_matches_oracle(eng, oracle, i, ch):
    """SRC = 3: Rgb8 / Rgba8 with rows padded by 1..3 bytes and an odd gap between images (no dword alignment survives), the luma residue
    image among the contents; the host entry point under 5 and 0, and the device entry point on the same bytes one byte into an allocation"""
    w, h = bg.COLOUR_GRID[i]
    imgs = bg.colour_contents(np.random.default_rng(w * 31 + h + ch), h, w, ch)
    n = len(imgs)
    buf, row_stride, image_stride = bg.embed(imgs, row_pad=1 + i % 3, image_gap=1 + 2 * (i % 4), lead=1)
    ref = reference(oracle, imgs)
    try:
        for which in (5, 0):
            eng.set_pdq_kernel(which)
            hold(hash_host(eng, buf[1:], n, w, h, ch, row_stride, image_stride), ref, f"{w}x{h}x{ch} host form under {which}")
            hold(hash_dev(eng, buf, 1, n, w, h, ch, row_stride, image_stride), ref, f"{w}x{h}x{ch} device form under {which}")
    finally:
        eng.set_pdq_kernel(4)


# ---- 3. batch seams -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", bg.BATCH_W)
@pytest.mark.parametrize("h", bg.BATCH_H)
def test_workgroups_that_straddle_images(eng, oracle, w, h):
    """workgroups take 64 consecutive lines of n * h: 8 distinct images cycled, every image of every call held to the oracle"""
    imgs = bg.contents(np.random.default_rng(h * 1009 + w), h, w)
    ref = reference(oracle, imgs)
    try:
        for n in bg.BATCH_N:
            idx = np.arange(n) % 8
            for which in (5, 4):
                eng.set_pdq_kernel(which)
                hold(hash_packed(eng, imgs[idx]), take(ref, idx), f"{n} images of {w}x{h} under {which}")
        # Rgb8 with more than a line of slack between images: the per-lane source offsets of one workgroup are no arithmetic sequence
        cimgs = bg.colour_contents(np.random.default_rng(h * 31 + w), h, w, 3)
        cref = reference(oracle, cimgs)
        eng.set_pdq_kernel(5)
        for n in bg.BATCH_COLOUR_N:
            idx = np.arange(n) % len(cimgs)
            buf, row_stride, image_stride = bg.embed(cimgs[idx], row_pad=1, image_gap=3 * (3 * w + 1) + 1)
            hold(hash_host(eng, buf, n, w, h, 3, row_stride, image_stride), take(cref, idx), f"{n} Rgb8 images of {w}x{h} with slack")
    finally:
        eng.set_pdq_kernel(4)


@pytest.mark.parametrize("w,h", [(200, 150), (100, 150)])
def test_automatic_dispatch_seam(eng, oracle, w, h):
    """RPH_STREAM_MIN_IMAGES (csrc/rph_internal.h; include/rupphash.h documents it under rph_pdq_set_kernel): one image below it a 200x150
    Luma8 call stays on the multi-pass kernels, from it on the streaming kernel takes it; 100x150 stays on them either way"""
    t = bg.stream_min_images()
    rng = np.random.default_rng(w + h)
    try:
        for n in (t - 1, t):
            imgs = rng.integers(0, 256, (n, h, w), dtype=np.uint8)
            imgs[:8] = bg.contents(rng, h, w)
            eng.set_pdq_kernel(4)
            auto = hash_packed(eng, imgs)
            eng.set_pdq_kernel(5)
            hold(auto, hash_packed(eng, imgs), f"{n} images of {w}x{h}: automatic against the multi-pass kernels")
            idx = np.unique(np.concatenate([np.arange(8), np.linspace(8, n - 1, 8).astype(int)]))
            assert len(idx) == 16
            hold(take(auto, idx), reference(oracle, imgs[idx]), f"{n} images of {w}x{h}, images {idx.tolist()}")
    finally:
        eng.set_pdq_kernel(4)


# ---- 4. thumbnails no caller can pass -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("src", sorted(bg.THUMBS), ids=lambda s: f"{s[0]}x{s[1]}")
def test_thumbnails_thinner_than_any_image(eng, oracle, src, ch):
    """sources whose thumbnail behind the pre-downsample has a side of 1..5, 63..65 or 127 beside 512: the multi-pass hasher at w = 512 with
    h = 1..4 (and its transpose), rows of align16(nw) bytes"""
    w, h = src
    nw, nh = C.c_uint32(), C.c_uint32()
    eng.L.rph_pdq_target_dimensions(w, h, 512, C.byref(nw), C.byref(nh))
    assert (nw.value, nh.value) == bg.THUMBS[src]
    rng = np.random.default_rng(w * 7 + h + ch)
    imgs = rng.integers(0, 256, (3, h, w) if ch == 1 else (3, h, w, ch), dtype=np.uint8)
    imgs[1] = 0
    npts = (w * h) // 12
    imgs[1].reshape(-1)[rng.integers(0, imgs[1].size, npts)] = rng.integers(1, 256, npts, dtype=np.uint8)
    ref = reference(oracle, imgs)
    try:
        for which in (0, 4, 5):
            eng.set_pdq_kernel(which)
            hold(hash_packed(eng, imgs), ref, f"{w}x{h}x{ch} -> {nw.value}x{nh.value} under {which}")
    finally:
        eng.set_pdq_kernel(4)


# ---- 5. images more than 4 GiB apart ------------------------------------------------------------------------------------------------
FAR_STRIDE = (1 << 31) + 64   # twice this is past 2^32: a 32-bit product lands 128 bytes into image 0, a sign-extended one in the zeros in front
FAR_FRONT = 1 << 31           # zeroed bytes in front of d_px, so that such a read stays inside the allocation


@pytest.fixture(scope="module")
def far_buffer(eng):
    nbytes = FAR_FRONT + 2 * FAR_STRIDE + 512 * 512 * 4
    try:
        base = eng.dev_alloc(nbytes)
    except Exception as e:  # the only reason to skip: the device cannot give 6 GiB
        pytest.skip(f"rph_dev_alloc of {nbytes} bytes failed: {e}")
    d_out = None
    try:
        d_out = eng.dev_alloc(3 * 2048)
        yield base, nbytes, d_out
    finally:
        eng.synchronize()
        eng.dev_free(base)
        if d_out:
            eng.dev_free(d_out)


@pytest.mark.parametrize("w,h,ch,which", [(100, 37, 3, 0), (100, 37, 3, 5), (200, 150, 1, 0), (200, 150, 1, 5), (200, 150, 1, 6), (512, 512, 1, 1), (512, 512, 1, 3)])
def test_images_more_than_4_gib_apart(eng, oracle, far_buffer, w, h, ch, which):
    """three distinct noise images at d_px + k (2^31 + 64) in a zeroed allocation that starts 2 GiB in front of d_px: an image offset cut to
    32 bits, or sign-extended, reads zeros or another image -- inside the allocation -- and shows as a wrong hash"""
    base, nbytes, d_out = far_buffer
    n = 3
    d_px = base + FAR_FRONT
    assert d_px + (n - 1) * FAR_STRIDE + w * h * ch <= base + nbytes
    imgs = np.random.default_rng(w + h + ch + which).integers(0, 256, (n, h, w) if ch == 1 else (n, h, w, ch), dtype=np.uint8)
    ref = reference(oracle, imgs)
    out = {"hash": np.zeros((n, 32), np.uint8), "quality": np.zeros(n, np.float32), "coeffs": np.zeros((n, 256), np.float32),
           "dihedral": np.zeros((n, 8, 32), np.uint8), "valid": np.zeros(n, np.uint8)}
    ptr, at = {}, 0
    for k in ("coeffs", "dihedral", "hash", "quality", "valid"):
        ptr[k], at = d_out + at, at + out[k].nbytes
    try:
        eng.dev_memset(base, 0, nbytes)
        eng.dev_memset(d_out, 0, n * 2048)
        eng.synchronize()
        for k in range(n):
            eng.dev_upload(d_px + k * FAR_STRIDE, imgs[k])
        eng.set_pdq_kernel(which)
        eng.pdq_hash_batch_dev(d_px, n, w, h, ch, ptr["hash"], ptr["quality"], ptr["coeffs"], ptr["dihedral"], ptr["valid"], image_stride=FAR_STRIDE)
        eng.synchronize()
        for k in KEYS:
            eng.dev_download(out[k], ptr[k])
    finally:
        eng.set_pdq_kernel(4)
    hold(out, ref, f"{w}x{h}x{ch} under {which}, images {FAR_STRIDE} bytes apart")
