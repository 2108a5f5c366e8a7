"""The device forms of the > 512 px pre-downsample (csrc/resize_kernels.hip) held to the CPU oracle at the THUMBNAIL, byte for byte (-m gpu):
the two-pass kernels, the LDS kernel with its unrolled and general windows, the matrix-pipe kernel, and the fallbacks between them.  The
thumbnails are read back with Engine.debug_thumbnails; a failure names the image, row and column.  The features behind them (coefficients,
quality, hash, dihedral) are compared bit for bit as everywhere else.  Geometries and contents: tests/resize_util.py, which
tests/test_resize_cpu.py pins to the published algorithm.  Nothing here has a tolerance.  (No input is made up for the clamp to 255 after
the shift: it cannot bite below a window of about 128 taps, see resize_util.)"""
import functools

import numpy as np
import pytest

import resize_util as ru

pytestmark = pytest.mark.gpu

KEYS = (("hash", np.uint8, 32), ("quality", np.float32, 1), ("coeffs", np.float32, 256), ("dihedral", np.uint8, 256), ("valid", np.uint8, 1))


@pytest.fixture(scope="module")
def eng():
    from rupphash_amd import Engine

    e = Engine(0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def _oracle():
    import oracle

    oracle.lib()
    return oracle


@functools.lru_cache(maxsize=None)
def reference(g, coloured):
    """(thumbnails (n, nh, nw), coefficients, quality, hash, dihedral) of a geometry's content stack from the CPU oracle: computed once,
    shared by every kernel selection, never written to.  Rgba8 has the luma of Rgb8."""
    o = _oracle()
    imgs = ru.colour(ru.content_stack(g)[0], 3 if coloured else 1)
    luma = np.stack([o.luma601(x) for x in imgs]) if coloured else imgs
    thumbs = np.stack([o.resize_box_u8(x, g.nw, g.nh) for x in luma])
    feats = [o.pdq_features(x) for x in imgs]
    assert all(f[0] == 0 for f in feats)
    coeffs = np.stack([f[1] for f in feats])
    out = (thumbs, coeffs, np.array([f[2] for f in feats], np.float32), np.stack([o.to_hash(c) for c in coeffs]), np.stack([o.dihedral_hashes(c) for c in coeffs]))
    for a in out:
        a.setflags(write=False)
    return out


def embed(imgs, ch, offset=0, row_pad=0, image_gap=0, fill=0):
    """the images at `offset` into one byte buffer with padded rows and a gap between images, every other byte = fill"""
    n, h, w = imgs.shape[:3]
    row_stride = w * ch + row_pad
    image_stride = row_stride * h + image_gap
    buf = np.full(offset + image_stride * n + 16, fill, np.uint8)
    rows = np.lib.stride_tricks.as_strided(buf[offset:], (n, h, w * ch), (image_stride, row_stride, 1))
    rows[...] = imgs.reshape(n, h, w * ch)
    return buf, row_stride, image_stride


def run_dev(eng, buf, offset, n, w, h, ch, row_stride, image_stride, nw, nh, stream=None):
    """one rph_pdq_hash_batch_dev call on the buffer's bytes: (outputs, thumbnails read back)"""
    d_px = eng.dev_alloc(buf.nbytes)
    d_out = {k: eng.dev_alloc(n * width * np.dtype(dt).itemsize) for k, dt, width in KEYS}
    try:
        eng.dev_upload(d_px, buf)
        eng.pdq_hash_batch_dev(d_px + offset, n, w, h, ch, d_out["hash"], d_out["quality"], d_out["coeffs"], d_out["dihedral"], d_out["valid"],
                               row_stride=row_stride, image_stride=image_stride, stream=stream)
        eng.synchronize()
        thumbs = eng.debug_thumbnails(n, nw, nh)
        out = {}
        for k, dt, width in KEYS:
            out[k] = np.zeros((n, width), dt)
            eng.dev_download(out[k], d_out[k])
    finally:
        eng.dev_free(d_px)
        for p in d_out.values():
            eng.dev_free(p)
    return out, thumbs


def run_host(eng, buf, offset, n, w, h, ch, row_stride, image_stride, nw, nh):
    """the same through rph_pdq_hash_batch (host pointers; the test calls stay below its 64 MiB chunk)"""
    from rupphash_amd._lib import check as rc_check

    assert image_stride * n <= 64 << 20
    out = {k: np.zeros((n, width), dt) for k, dt, width in KEYS}
    rc_check(eng.L.rph_pdq_hash_batch(eng.ctx, buf.ctypes.data + offset, n, w, h, ch, row_stride, image_stride, out["hash"].ctypes.data, out["quality"].ctypes.data,
                                      out["coeffs"].ctypes.data, out["dihedral"].ctypes.data, out["valid"].ctypes.data), "rph_pdq_hash_batch")
    return out, eng.debug_thumbnails(n, nw, nh)


def hold_to_oracle(g, ch, out, thumbs, what):
    want_thumbs, coeffs, quality, hashes, dihedral = reference(g, ch > 1)
    names = ru.content_stack(g)[1]
    diff = ru.first_difference(thumbs, want_thumbs, names)
    assert diff is None, f"{what}: thumbnail differs from the oracle's at {diff}"
    # the read-back shows THIS call's thumbnails, not what an earlier call left in the scratch: flat black and flat white are exactly that
    assert names[:2] == ["all 0", "all 255"] and not thumbs[0].any() and (thumbs[1] == 255).all(), what
    assert out["valid"].all(), what
    for k in range(len(names)):
        assert out["coeffs"][k].tobytes() == coeffs[k].tobytes(), f"{what}: coefficients differ for image {k} ({names[k]})"
        assert out["quality"][k].tobytes() == quality[k].tobytes(), f"{what}: quality differs for image {k} ({names[k]})"
        assert np.array_equal(out["hash"][k], hashes[k]), f"{what}: hash differs for image {k} ({names[k]})"
        assert np.array_equal(out["dihedral"][k].reshape(8, 32), dihedral[k]), f"{what}: dihedral hashes differ for image {k} ({names[k]})"


def _selections():
    """pdq_kernel 0: luma plane + the two plain resize kernels + the plain hasher; 4 (default): Luma8 on the matrix pipe, colour through the
    LDS kernel (6144 px wide Rgba8: staged row above 8 x 256 bytes, two-pass), tiled hasher; 5: Luma8 through the LDS kernel as well; 6: the
    streaming hasher behind the same resize.  Left out, because the form cannot differ from a selection that is run:
      5 with colour      -- colour sources take the LDS kernel under 4 already, and 4 hashes calls this small with 5's tiled kernels
      6 unless 1285x650  -- the streaming hasher takes thumbnails of 128 .. 512 px a side; every other thumbnail here has a side of at
                            most 40 px and goes to the kernels of 4, behind the resize of 4"""
    out = []
    for g in ru.GEOMETRIES:
        for ch in (1, 3, 4):
            for which in (0, 4, 5, 6):
                if which == 5 and ch > 1:
                    continue
                if which == 6 and min(g.nw, g.nh) < 128:
                    continue
                out.append(pytest.param(g, ch, which, id=f"{ru.geometry_id(g)}-ch{ch}-kernel{which}"))
    return out


@pytest.mark.parametrize("g,ch,which", _selections())
def test_thumbnails_and_features_equal_the_oracle(eng, g, ch, which):
    """one call carries the whole content stack (neighbouring images differ, so image indexing is tested too)"""
    imgs = ru.colour(ru.content_stack(g)[0], ch)
    n = len(imgs)
    buf = np.ascontiguousarray(imgs).reshape(-1)
    eng.set_pdq_kernel(which)
    try:
        out, thumbs = run_dev(eng, buf, 0, n, g.w, g.h, ch, g.w * ch, g.w * g.h * ch, g.nw, g.nh)
    finally:
        eng.set_pdq_kernel(4)
    hold_to_oracle(g, ch, out, thumbs, f"{ru.geometry_id(g)} ({g.note}), {ch} channels, pdq_kernel {which}")


LAYOUTS = [pytest.param(g, ch, which, id=f"{ru.geometry_id(g)}-ch{ch}-kernel{which}") for g in ru.GEOMETRIES if (g.w, g.h) in ((1537, 120), (768, 60))
           for ch, which in ((1, 4), (1, 5), (3, 4))]  # (Rgb8 takes the LDS kernel under 4 already: 5 is the same form)


@pytest.mark.parametrize("g,ch,which", LAYOUTS)
def test_layouts_and_pad_bytes(eng, g, ch, which):
    """Base addresses 1, 2, 3 bytes off, rows padded by 1, 2, 3, 5 bytes and a gap between images, through the host and the device entry
    point, once with every pad byte 0x00 and once with 0xFF: no pad byte may reach a thumbnail (a stray read shows as a difference between
    the two fills; nothing is placed at the end of an allocation), and every thumbnail equals the oracle's.  1537x120 has window 5 and
    768x60 window 3, the unrolled forms of the LDS kernel, which Luma8 takes under 5 and Rgb8 under 4; under 4 Luma8 takes the
    matrix-pipe kernel's path for rows off dword boundaries."""
    assert len(LAYOUTS) == 6
    imgs = ru.colour(ru.content_stack(g)[0], ch)
    n = len(imgs)
    eng.set_pdq_kernel(which)
    try:
        for offset in (1, 2, 3):
            for row_pad in (1, 2, 3, 5):
                got = {}
                for fill in (0x00, 0xFF):
                    buf, row_stride, image_stride = embed(imgs, ch, offset, row_pad, 7 + offset, fill)
                    for entry, run in (("host", run_host), ("dev", run_dev)):
                        out, thumbs = run(eng, buf, offset, n, g.w, g.h, ch, row_stride, image_stride, g.nw, g.nh)
                        what = f"{ru.geometry_id(g)} {ch} channels pdq_kernel {which} {entry} entry, base + {offset}, row_stride = w * ch + {row_pad}, pad bytes {fill:#04x}"
                        hold_to_oracle(g, ch, out, thumbs, what)
                        got[fill, entry] = thumbs
                for entry in ("host", "dev"):
                    diff = ru.first_difference(got[0x00, entry], got[0xFF, entry])
                    assert diff is None, f"pad bytes reach the thumbnail ({entry} entry, base + {offset}, row pad {row_pad}): {diff}"
    finally:
        eng.set_pdq_kernel(4)


# ---------------------------------------------------------------- the axis cache past its limit
CACHE_MAX = 256  # kAxisCacheMax of resize_kernels.hip


class CacheModel:
    """what device_axis keeps: a lookup of a new (in, out) pair when CACHE_MAX are cached drops every table first; a call looks both of its
    axes up and then both again"""

    def __init__(self):
        self.axes, self.drops, self.second_lookup_dropped_the_first = set(), 0, 0

    def call(self, w, h):
        nw, nh = ru.target_dimensions(w, h)
        for turn in range(2):
            for k, key in enumerate(((w, nw), (h, nh))):
                if key not in self.axes:
                    if len(self.axes) >= CACHE_MAX:
                        self.axes.clear()
                        self.drops += 1
                        if turn == 0 and k == 1:
                            self.second_lookup_dropped_the_first += 1
                    self.axes.add(key)


def _turnover_images(k):
    w = 513 + k
    rng = np.random.default_rng(7000 + k)
    imgs = rng.integers(0, 256, (2, 6, w), dtype=np.uint8)
    imgs[1] = ((np.arange(w)[None, :] // 3 + np.arange(6)[:, None]) & 1) * 255
    return imgs


@functools.lru_cache(maxsize=None)
def _turnover_reference(k):
    o = _oracle()
    feats = [o.pdq_features(x) for x in _turnover_images(k)]
    return np.stack([f[1] for f in feats]), np.array([f[2] for f in feats], np.float32), np.stack([o.to_hash(f[1]) for f in feats])


def _hold_turnover(k, out, what):
    coeffs, quality, hashes = _turnover_reference(k)
    assert out["valid"].all(), (what, k)
    assert out["coeffs"].tobytes() == coeffs.tobytes(), f"{what}: coefficients of source width {513 + k} differ from the oracle's"
    assert out["quality"].tobytes() == quality.tobytes() and np.array_equal(out["hash"], hashes), f"{what}: width {513 + k}"


def test_axis_cache_turnover():
    """300 new width axes through one fresh context, in ascending order: the 256-entry cache is dropped on the way, every result equals
    the oracle's, and the first three, hashed again after the drop, are unchanged"""
    from rupphash_amd import Engine

    model = CacheModel()
    eng = Engine(0)
    try:
        first = {}
        for k in range(300):
            imgs = _turnover_images(k)
            model.call(513 + k, 6)
            out = eng.pdq_hash_batch(imgs, want_quality=True, want_coeffs=True)
            _hold_turnover(k, out, "ascending")
            if k < 3:
                first[k] = out
        assert model.drops == 1 and all((513 + k, 512) not in model.axes for k in range(3))
        for k in range(3):
            out = eng.pdq_hash_batch(_turnover_images(k), want_quality=True, want_coeffs=True)
            _hold_turnover(k, out, "after the drop")
            for key in ("hash", "coeffs", "quality"):
                assert out[key].tobytes() == first[k][key].tobytes()
    finally:
        eng.close()


def test_axis_cache_second_lookup_drops_the_first(oracle):
    """a geometry whose two axes are both new arrives when 255 are cached: its first lookup fills the cache, its second drops every
    table, the first one's among them, and the call looks both up again"""
    from rupphash_amd import Engine

    model = CacheModel()
    eng = Engine(0)
    try:
        k = 0
        while len(model.axes) < CACHE_MAX - 1:
            model.call(513 + k, 6)
            _hold_turnover(k, eng.pdq_hash_batch(_turnover_images(k), want_quality=True, want_coeffs=True), "filling")
            k += 1
        assert len(model.axes) == CACHE_MAX - 1 and model.drops == 0
        w, h = 1000, 900
        assert (w, 512) not in model.axes and (h, ru.target_dimensions(w, h)[1]) not in model.axes
        model.call(w, h)
        assert model.second_lookup_dropped_the_first == 1 and len(model.axes) == 2
        rng = np.random.default_rng(1000900)
        imgs = np.stack([rng.integers(0, 256, (h, w), dtype=np.uint8), ru.contents(rng, h, w)[0][-1]])
        out = eng.pdq_hash_batch(imgs, want_quality=True, want_coeffs=True)
        nw, nh = ru.target_dimensions(w, h)
        thumbs = eng.debug_thumbnails(2, nw, nh)
        diff = ru.first_difference(thumbs, np.stack([oracle.resize_box_u8(x, nw, nh) for x in imgs]))
        assert diff is None, f"thumbnail of the call whose second lookup dropped the first: {diff}"
        for i in range(2):
            rc, c, q = oracle.pdq_features(imgs[i])
            assert rc == 0 and out["coeffs"][i].tobytes() == c.tobytes() and out["quality"][i].tobytes() == np.float32(q).tobytes()
            assert np.array_equal(out["hash"][i], oracle.to_hash(c))
        # and the geometries from before the drop are built again
        _hold_turnover(0, eng.pdq_hash_batch(_turnover_images(0), want_quality=True, want_coeffs=True), "after the drop")
    finally:
        eng.close()


def test_axis_cache_turnover_on_two_caller_streams():
    """the same 300 geometries alternating between two caller streams, nothing synchronised on the host inside a stream: the tables are
    dropped while the other stream's work may still be reading them"""
    from rupphash_amd import Engine

    eng = Engine(0)
    streams = [eng.stream_create(), eng.stream_create()]
    n_geo = 300
    sets = [_turnover_images(k) for k in range(n_geo)] + [_turnover_images(k) for k in range(3)]
    offs = np.cumsum([0] + [s.nbytes for s in sets])
    d_px = eng.dev_alloc(int(offs[-1]))
    d_out = {k: eng.dev_alloc(len(sets) * 2 * width * np.dtype(dt).itemsize) for k, dt, width in KEYS}
    try:
        eng.dev_upload(d_px, np.concatenate([s.reshape(-1) for s in sets]))
        eng.synchronize()
        for i, s in enumerate(sets):
            at = {k: d_out[k] + i * 2 * width * np.dtype(dt).itemsize for k, dt, width in KEYS}
            eng.pdq_hash_batch_dev(d_px + int(offs[i]), 2, s.shape[2], 6, 1, at["hash"], at["quality"], at["coeffs"], None, at["valid"], stream=streams[i & 1])
        for st in streams:
            eng.stream_synchronize(st)
        got = {}
        for k, dt, width in KEYS:
            got[k] = np.zeros((len(sets), 2, width), dt)
            eng.dev_download(got[k], d_out[k])
        for i in range(len(sets)):
            _hold_turnover(i if i < n_geo else i - n_geo, {k: got[k][i] for k in got}, f"two streams, call {i}")
    finally:
        eng.dev_free(d_px)
        for p in d_out.values():
            eng.dev_free(p)
        for st in streams:
            eng.stream_destroy(st)
        eng.close()
