"""rph_image_hash_ragged / rph_image_hash_ragged_dev on the device (-m gpu): decoded images of any mix of sizes and of the eight layouts
(Luma, LumaA, Rgb, Rgba with u8 or u16 samples) in ONE call, PDQ outputs and pixel hashes from one upload (csrc/pdq_ragged.hip:
ragged_luma_kernel's quads for the five layouts the hasher does not read; csrc/blake3_kernels.hip: b3_pixels_ragged_kernel).

Yardsticks, all bit for bit (nothing here has a tolerance):
  PDQ         oracle.pdq_features of png_util.hasher_pixels(image) -- (v + 128) // 257 per u16 sample, L replicated, alpha dropped by the
              oracle's luma -- hash, quality and the 256 coefficients as uint32, the 8 dihedral hashes
  pixel hash  blake3_util.blake3 of png_util.to_rgba16(image) (numpy, astype('<u2')); for images of more than one 64-chunk group
              rph_blake3_host of the same bytes (tests/test_blake3_cpu.py holds it to the published vectors)
Images come from a seeded numpy generator (smooth + noise; u16 images carry noise in their low bytes, so a truncation to 8 bits hashes
something else); each image and each reference is made once and never written to."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import blake3_util
import png_util

pytestmark = pytest.mark.gpu

LAYOUTS = (1, 2, 3, 4, 17, 18, 19, 20)
# (w, h) by pixel count: 0; 1; the chunk edge 127, 128, 129; widths 5, 7, 9 (blocks of 8 pixels cross row ends); the group edge 8191, 8192,
# 8193; 3 groups; 5 groups + 1 pixel (the fold carries an odd node)
PIXEL_SIZES = ((7, 0), (1, 1), (127, 1), (64, 2), (43, 3), (5, 26), (7, 19), (9, 15), (8191, 1), (128, 64), (2731, 3), (256, 96), (40961, 1))
# too small (valid 0); class F (a side < 128); class S at both corners; class R twice (513 wide: the smallest; 1030x520)
PDQ_SIZES = ((4, 9), (127, 200), (128, 128), (512, 512), (513, 300), (1030, 520))


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
def image(layout, w, h, seed=0):
    ch, wide = layout & 15, layout > 16
    rng = np.random.default_rng([layout, w, h, seed])
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    planes = []
    for k in range(ch):
        a, b, c = rng.uniform(-1, 1, 3)
        fx, fy = rng.uniform(1, 6, 2)
        p = 128 + 50 * a * (x / max(w - 1, 1) - 0.5) + 50 * b * (y / max(h - 1, 1) - 0.5) + 40 * c * np.sin(fx * x / max(w, 1) * 6.283 + fy * y / max(h, 1) * 6.283)
        p = np.clip(p + rng.normal(0, 12, (h, w)), 0, 255)
        planes.append((np.clip(p * 257 + rng.integers(-128, 129, (h, w)), 0, 65535).astype(np.uint16)) if wide else p.astype(np.uint8))
    out = np.ascontiguousarray(planes[0] if ch == 1 else np.stack(planes, axis=2))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def pdq_reference(layout, w, h, seed=0):
    """(valid, hash, quality, coeffs, dihedral) from the CPU oracle on the hasher's pixels"""
    o = _oracle()
    rc, coeffs, q = o.pdq_features(np.ascontiguousarray(png_util.hasher_pixels(image(layout, w, h, seed))))
    if rc != 0:
        assert w < 5 or h < 5
        out = (0, np.zeros(32, np.uint8), np.zeros(1, np.float32), np.zeros(256, np.float32), np.zeros((8, 32), np.uint8))
    else:
        out = (1, o.to_hash(coeffs), np.array([q], np.float32), coeffs, o.dihedral_hashes(coeffs))
    for a in out[1:]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def pixel_reference(layout, w, h, seed=0):
    from rupphash_amd import _lib

    data = png_util.to_rgba16(image(layout, w, h, seed))
    assert len(data) == 8 * w * h
    if w * h <= 8192:
        return blake3_util.blake3(data)
    out = np.zeros(32, np.uint8)
    _lib.load().rph_blake3_host(data, len(data), None, out.ctypes.data)
    return out.tobytes()


def check_pdq(out, specs, what=""):
    assert len(out["valid"]) == len(specs)
    for i, s in enumerate(specs):
        valid, hsh, q, coeffs, dih = pdq_reference(*s)
        tag = f"{what} image {i} {s}"
        assert out["valid"][i] == valid, tag
        assert np.array_equal(out["hash"][i], hsh), tag
        if out["quality"] is not None:
            assert out["quality"][i:i + 1].view(np.uint32) == q.view(np.uint32), tag
        if out["coeffs"] is not None:
            bad = np.flatnonzero(out["coeffs"][i].view(np.uint32) != coeffs.view(np.uint32))
            assert bad.size == 0, f"{tag}: {bad.size} coefficients differ, first {bad[:4]}"
        if out["dihedral"] is not None:
            assert np.array_equal(out["dihedral"][i].reshape(8, 32), dih), tag
        if valid and min(s[1], s[2]) >= 64:
            assert q[0] > 0, tag


def check_pixel(out, specs, what=""):
    assert out["pixel_hash"].shape == (len(specs), 32)
    for i, s in enumerate(specs):
        assert out["pixel_hash"][i].tobytes() == pixel_reference(*s), f"{what} image {i} {s}"


def embedded(specs, fill):
    """every image as a slice of one byte buffer, the rest `fill`: u8 images at odd addresses with rows padded by 1, 2, 3, 1 .. bytes, u16
    images at offsets = 2 mod 4 with rows padded by 2 bytes.  Returns (buffer, [views], offsets, row strides)."""
    offs, strides, at = [], [], 1
    for k, (layout, w, h, *_) in enumerate(specs):
        bps = 2 if layout > 16 else 1
        row = w * (layout & 15) * bps
        strides.append(row + (2 if bps == 2 else 1 + k % 3))
        at = (-(-at // 4) * 4 + 2) if bps == 2 else at | 1
        offs.append(at)
        at += strides[-1] * h + 5
    buf = np.full(at + 16, fill, np.uint8)
    assert buf.ctypes.data % 4 == 0
    views = []
    for (layout, w, h, *rest), o, st in zip(specs, offs, strides):
        ch, dt = layout & 15, np.dtype(np.uint16 if layout > 16 else np.uint8)
        v = np.ndarray((h, w, ch), dt, buffer=buf, offset=o, strides=(st, ch * dt.itemsize, dt.itemsize))
        v[...] = image(layout, w, h, *rest).reshape(h, w, ch)
        views.append(v[:, :, 0] if ch == 1 else v)
    return buf, views, offs, strides


SIZES = {"hash": 32, "quality": 4, "coeffs": 1024, "dihedral": 256, "valid": 1, "pixel_hash": 32}
SHAPES = (("hash", np.uint8, (32,)), ("quality", np.float32, ()), ("coeffs", np.float32, (256,)), ("dihedral", np.uint8, (8, 32)), ("valid", np.uint8, ()),
          ("pixel_hash", np.uint8, (32,)))


def dev_call(eng, buf, offs, specs, strides, want=("hash", "quality", "coeffs", "dihedral", "valid", "pixel_hash")):
    """rph_image_hash_ragged_dev on an uploaded buffer; the dict has None for outputs not asked for"""
    n = len(specs)
    d_px = eng.dev_alloc(len(buf))
    d = {k: eng.dev_alloc(max(n, 1) * b) if k in want else None for k, b in SIZES.items()}
    try:
        eng.dev_upload(d_px, buf)
        eng.image_hash_ragged_dev(d_px, offs, [s[1] for s in specs], [s[2] for s in specs], [s[0] for s in specs], strides, d["hash"], d["quality"], d["coeffs"],
                                  d["dihedral"], d["valid"], d["pixel_hash"])
        eng.synchronize()
        out = {}
        for k, dt, shape in SHAPES:
            out[k] = None
            if d[k] is not None:
                out[k] = np.zeros((n,) + shape, dt)
                if n:
                    eng.dev_download(out[k], d[k])
        return out
    finally:
        eng.synchronize()
        for p in [d_px] + list(d.values()):
            if p is not None:
                eng.dev_free(p)


def same(a, b):
    for k in a:
        assert (a[k] is None) == (b[k] is None), k
        if a[k] is not None:
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


def permuted(specs, seed):
    return [specs[k] for k in np.random.default_rng(seed).permutation(len(specs))]


# ---- pixel hash

def test_pixel_hash_every_layout_at_every_edge(eng):
    """every layout at every pixel count of the list in one call, in a permuted order; images at odd addresses (u8) and at offsets = 2 mod 4
    (u16), padded rows, 0x00 and 0xFF around the pixels; the host form and the device form"""
    specs = permuted([(lay, w, h) for w, h in PIXEL_SIZES for lay in LAYOUTS], 3)
    assert len(specs) == 104
    outs = []
    for fill in (0x00, 0xFF):
        buf, views, offs, strides = embedded(specs, fill)
        assert all(v.ctypes.data % 4 == 2 for v, s in zip(views, specs) if s[0] > 16 and s[2])
        assert all(v.ctypes.data % 2 == 1 for v, s in zip(views, specs) if s[0] < 16 and s[2])
        host = eng.image_hash_ragged(views, want_pdq=False)
        assert host["hash"] is None and host["valid"] is None
        check_pixel(host, specs, f"host form, fill {fill:#x}")
        dev = dev_call(eng, buf, offs, specs, strides, want=("pixel_hash",))
        check_pixel(dev, specs, f"device form, fill {fill:#x}")
        outs.append(host)
    same(outs[0], outs[1])


def test_pixel_hash_of_nothing_is_the_hash_of_the_empty_string(eng):
    out = eng.image_hash_ragged([np.zeros((0, 7, 3), np.uint16), np.zeros((5, 0), np.uint8)], want_pdq=False)
    empty = blake3_util.blake3(b"")
    assert out["pixel_hash"][0].tobytes() == empty and out["pixel_hash"][1].tobytes() == empty


# ---- PDQ (+ pixel hash from the same upload)

def pdq_specs():
    return permuted([(lay, w, h) for w, h in PDQ_SIZES for lay in LAYOUTS], 4)


def test_every_layout_and_class_in_one_call(eng):
    """all eight layouts and the three classes (S, R, F; too small among the F) interleaved: every output against the oracle, the pixel hash
    of every image (the 4x9 ones too); for the layouts the older calls take, their results as well"""
    specs = pdq_specs()
    imgs = [image(*s) for s in specs]
    out = eng.image_hash_ragged(imgs, want_coeffs=True, want_dihedral=True)
    check_pdq(out, specs)
    check_pixel(out, specs)
    assert [int(v) for v, s in zip(out["valid"], specs) if s[1] == 4] == [0] * 8
    old = [i for i, s in enumerate(specs) if s[0] in (1, 3, 4)]
    ref = eng.pdq_hash_ragged([imgs[i] for i in old], want_quality=True, want_coeffs=True, want_dihedral=True)
    for k in ("hash", "quality", "coeffs", "dihedral", "valid"):
        assert np.array_equal(out[k][old].view(np.uint8), ref[k].view(np.uint8)), k
    for i in old:
        assert np.array_equal(out["pixel_hash"][i], eng.pixel_hash_batch(imgs[i][None])[0]), specs[i]


def test_device_form_embedded_and_packed(eng):
    """the device form on images embedded at odd / 2 mod 4 offsets with padded rows, and on Engine's packing (16-byte aligned, dword pitches)"""
    from rupphash_amd.engine import image_pack

    specs = [s for s in pdq_specs() if s[1:] != (512, 512)]
    outs = []
    for fill in (0x00, 0xFF):
        buf, views, offs, strides = embedded(specs, fill)
        outs.append(dev_call(eng, buf, offs, specs, strides))
        check_pdq(outs[-1], specs, f"fill {fill:#x}")
        check_pixel(outs[-1], specs, f"fill {fill:#x}")
    same(outs[0], outs[1])
    buf, off, w, h, lay, rs = image_pack([image(*s) for s in specs], fill=0xFF)
    assert lay.tolist() == [s[0] for s in specs]
    packed = dev_call(eng, buf, off, specs, rs)
    same(outs[0], packed)


# ---- edges of the interface

def test_no_images(eng):
    out = eng.image_hash_ragged([])
    assert out["hash"].shape == (0, 32) and out["pixel_hash"].shape == (0, 32)
    assert dev_call(eng, np.zeros(16, np.uint8), [], [], [])["hash"].shape == (0, 32)


EDGE = [(19, 200, 150), (2, 513, 300), (17, 127, 200), (4, 4, 9), (20, 128, 128), (18, 129, 131), (3, 300, 200), (1, 130, 140)]


@pytest.mark.parametrize("missing", ["quality", "coeffs", "dihedral", "valid", "pixel_hash", "pdq"])
def test_every_nullable_output_null_in_turn(eng, missing):
    buf, views, offs, strides = embedded(EDGE, 0)
    want = [k for k in SIZES if k != missing] if missing != "pdq" else ["pixel_hash"]
    out = dev_call(eng, buf, offs, EDGE, strides, want=want)
    assert all((out[k] is None) == (k not in want) for k in SIZES)
    host = eng.image_hash_ragged(views, want_pdq=missing != "pdq", want_pixel_hash=missing != "pixel_hash", want_quality=missing != "quality",
                                 want_coeffs=missing != "coeffs", want_dihedral=missing != "dihedral")
    for o, what in ((out, "device"), (host, "host")):
        if o["pixel_hash"] is not None:
            check_pixel(o, EDGE, what)
        if o["hash"] is not None:
            if o["valid"] is None:
                o["valid"] = np.array([pdq_reference(*s)[0] for s in EDGE], np.uint8)
            check_pdq(o, EDGE, what)


def test_no_output_and_pdq_outputs_without_the_hash_are_refused(eng):
    from rupphash_amd._lib import RPH_ERR_INVALID_ARG

    buf, views, offs, strides = embedded(EDGE[:2], 0)
    n = 2
    px = (C.c_void_p * n)(*[v.ctypes.data for v in views])
    w, h, lay = (np.array([s[k] for s in EDGE[:2]], np.uint32) for k in (1, 2, 0))
    rs = (C.c_size_t * n)(*strides)
    q = np.full(n, 7.0, np.float32)
    f = eng.L.rph_image_hash_ragged
    assert f(eng.ctx, px, w.ctypes.data, h.ctypes.data, lay.ctypes.data, rs, n, None, None, None, None, None, None) == RPH_ERR_INVALID_ARG
    assert f(eng.ctx, px, w.ctypes.data, h.ctypes.data, lay.ctypes.data, rs, n, None, q.ctypes.data, None, None, None, q.ctypes.data) == RPH_ERR_INVALID_ARG
    assert f(eng.ctx, px, w.ctypes.data, None, lay.ctypes.data, rs, n, q.ctypes.data, None, None, None, None, None) == RPH_ERR_INVALID_ARG
    assert np.all(q == 7.0)


FAULTS = {"layout 5": ("layout", 5), "layout 21": ("layout", 21), "odd stride, 16-bit": ("stride", "odd"), "short stride": ("stride", "short"),
          "odd address, 16-bit": ("offset", 1)}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_invalid_descriptor_refuses_the_whole_call(eng, fault):
    """nothing is launched and no output is touched, in both forms"""
    from rupphash_amd import RphError
    from rupphash_amd._lib import RPH_ERR_INVALID_ARG

    specs = [(3, 193, 157), (19, 130, 140), (1, 129, 128)]
    buf, views, offs, strides = embedded(specs, 0)
    lay, w, h = ([s[k] for s in specs] for k in range(3))
    ptrs = [v.ctypes.data for v in views]
    kind, arg = FAULTS[fault]
    if kind == "layout":
        lay[1] = arg
    elif kind == "offset":
        offs[1] += 1
        ptrs[1] += 1
    elif arg == "odd":
        strides[1] += 1
    else:
        strides[1] = w[1] * 6 - 2
    n = len(specs)
    d_px = eng.dev_alloc(len(buf))
    d_out = eng.dev_alloc(n * 1024)
    try:
        eng.dev_upload(d_px, buf)
        eng.dev_memset(d_out, 0xA5, n * 1024)
        with pytest.raises(RphError) as e:
            eng.image_hash_ragged_dev(d_px, offs, w, h, lay, strides, d_out, d_out, d_out, d_out, d_out, d_out)
        assert e.value.status == RPH_ERR_INVALID_ARG
        eng.synchronize()
        back = np.zeros(n * 1024, np.uint8)
        eng.dev_download(back, d_out)
        assert np.all(back == 0xA5)
    finally:
        eng.dev_free(d_px)
        eng.dev_free(d_out)
    px = (C.c_void_p * n)(*ptrs)
    aw, ah, al = (np.array(a, np.uint32) for a in (w, h, lay))
    rs = (C.c_size_t * n)(*strides)
    hsh, q, valid, ph = np.full((n, 32), 0xA5, np.uint8), np.full(n, 7.0, np.float32), np.full(n, 0xA5, np.uint8), np.full((n, 32), 0xA5, np.uint8)
    rc = eng.L.rph_image_hash_ragged(eng.ctx, px, aw.ctypes.data, ah.ctypes.data, al.ctypes.data, rs, n, hsh.ctypes.data, q.ctypes.data, None, None,
                                     valid.ctypes.data, ph.ctypes.data)
    assert rc == RPH_ERR_INVALID_ARG
    assert np.all(hsh == 0xA5) and np.all(q == 7.0) and np.all(valid == 0xA5) and np.all(ph == 0xA5)


def test_older_calls_still_refuse_what_they_refused(eng):
    from rupphash_amd import RphError

    with pytest.raises(ValueError):
        eng.pdq_hash_ragged([np.zeros((8, 8, 2), np.uint8)])
    d = eng.dev_alloc(4096)
    try:
        with pytest.raises(RphError):
            eng.pdq_hash_ragged_dev(d, [0], [8], [8], [2], [16], d)
        with pytest.raises(RphError):
            eng.pdq_hash_ragged_dev(d, [0], [8], [8], [19], [48], d)
    finally:
        eng.dev_free(d)


# ---- kernel selection, staging chunks

MODE_SPECS = [(lay, w, h) for (w, h), lays in (((200, 150), LAYOUTS), ((513, 300), (2, 3, 17, 20)), ((127, 200), (1, 18, 19))) for lay in lays]


@pytest.mark.parametrize("mode", [5, 0, 6, 4], ids=["mode5-all-F", "mode0-all-F", "mode6", "default"])
def test_kernel_modes(eng, mode):
    """rph_pdq_set_kernel 0 and 5: every image goes through the uniform path, the five other layouts as Luma8 planes; 6 and the default
    take the descriptor kernels.  The oracle does not care."""
    specs = permuted(MODE_SPECS, mode)
    eng.set_pdq_kernel(mode)
    try:
        out = eng.image_hash_ragged([image(*s) for s in specs], want_coeffs=True, want_dihedral=True)
    finally:
        eng.set_pdq_kernel(4)
    check_pdq(out, specs, f"mode {mode}")
    check_pixel(out, specs, f"mode {mode}")


def test_runs_of_one_size_among_the_fallback_images(eng):
    """class-F images of the other layouts go through the uniform path in runs of one size whatever their layouts: three of 100x90 in a row
    (LumaA8, Rgb16, Luma16), an image of the hasher's own layout between two runs, an empty and a too-small image inside a run"""
    specs = [(2, 100, 90), (19, 100, 90), (17, 100, 90, 1), (3, 100, 90), (18, 100, 90), (20, 7, 0), (20, 7, 0, 1), (2, 3, 40), (17, 3, 40), (19, 64, 600)]
    out = eng.image_hash_ragged([image(*s) for s in specs], want_coeffs=True, want_dihedral=True)
    check_pdq(out, specs)
    check_pixel(out, specs)


def test_three_staging_chunks():
    """RPH_RAGGED_CHUNK_BYTES (read once, when the context is made) cuts a 12-image call into three staging chunks: both pinned sets are
    used, the first one twice; both hashes of a chunk come from its one upload and land in the images' own slots"""
    from rupphash_amd import Engine

    specs = [(LAYOUTS[k % 8], 128 + 7 * k, 160 - 3 * k) for k in range(10)] + [(17, 513, 300), (2, 100, 64)]
    sizes = [-(-(w * (lay & 15) * (2 if lay > 16 else 1)) // 4) * 4 * h for lay, w, h in specs]
    limit = 400000
    chunks, fill = 1, 0
    for s in sizes:  # the rule of the host form: an image that does not fit opens the next chunk
        at = -(-fill // 16) * 16
        if fill and at + s > limit:
            chunks, at = chunks + 1, 0
        fill = at + s
    assert chunks == 3
    os.environ["RPH_RAGGED_CHUNK_BYTES"] = str(limit)
    try:
        e = Engine(0)
    finally:
        del os.environ["RPH_RAGGED_CHUNK_BYTES"]
    try:
        out = e.image_hash_ragged([image(*s) for s in specs], want_coeffs=True, want_dihedral=True)
    finally:
        e.close()
    check_pdq(out, specs)
    check_pixel(out, specs)


# ---- the layers above, and closing the loop with the library's own decoders

def test_pdqhash_and_scanner_take_what_the_loaders_return(eng):
    from rupphash_amd import pdqhash, scanner

    specs = [(19, 200, 150), (2, 130, 140), (17, 4, 9), (3, 193, 157), (20, 513, 300)]
    imgs = [image(*s) for s in specs]
    many = pdqhash.generate_pdq_features_many(imgs, engine=eng)
    both = scanner.hash_images(imgs, engine=eng)
    assert many[2] is None and both[2][:3] == (None, None, None)
    for s, im, m, b in zip(specs, imgs, many, both):
        valid, hsh, q, coeffs, _ = pdq_reference(*s)
        assert b[3] == pixel_reference(*s) and scanner.pixel_hash(im, engine=eng) == pixel_reference(*s)
        if not valid:
            continue
        one = pdqhash.generate_pdq_features(im, engine=eng)
        gp = pdqhash.generate_pdq(im, engine=eng)
        for feats, quality in (m, one, (b[2], b[1])):
            assert np.array_equal(feats.coefficients.view(np.uint32), coeffs.view(np.uint32)) and np.float32(quality).view(np.uint32) == q.view(np.uint32)[0]
        assert b[0] == hsh.tobytes() and np.array_equal(gp[0], hsh) and np.float32(gp[1]).view(np.uint32) == q.view(np.uint32)[0]
    assert scanner.hash_images(imgs[:2], pixel_hash=False, engine=eng)[0][3] is None


def test_png_decode_then_hash_is_the_png_pipeline(eng):
    """16-bit gray, gray + alpha, RGB and RGBA files and an 8-bit gray + alpha one: Engine.png_decode -> image_hash_ragged gives the hash,
    quality and pixel hash of png_pdq_hash_batch(want_pixel_hash=True)"""
    rng = np.random.default_rng(2026)
    files = [png_util.encode(png_util.random_samples(rng, h, w, ct, d), ct, d) for ct, d, w, h in
             ((0, 16, 150, 140), (4, 16, 131, 129), (2, 16, 200, 150), (6, 16, 160, 130), (4, 8, 513, 300), (2, 16, 4, 9))]
    decoded = [eng.png_decode(f) for f in files]
    assert [(a.dtype.itemsize, a.ndim == 3 and a.shape[2]) for a in decoded] == [(2, False), (2, 2), (2, 3), (2, 4), (1, 2), (2, 3)]
    out = eng.image_hash_ragged(decoded)
    ref = eng.png_pdq_hash_batch(files, want_pixel_hash=True)
    assert np.all(ref["status"] == 0) and ref["valid"].tolist() == [1, 1, 1, 1, 1, 0]
    for k in ("hash", "quality", "valid", "pixel_hash"):
        assert np.array_equal(out[k].view(np.uint8), ref[k].view(np.uint8)), k
