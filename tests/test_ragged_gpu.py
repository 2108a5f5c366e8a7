"""The ragged PDQ call on the device (-m gpu): images of any mix of sizes and channel counts in ONE call of rph_pdq_hash_ragged /
rph_pdq_hash_ragged_dev (csrc/pdq_ragged.hip: descriptor-driven luma, pre-downsample and streaming kernels).

The yardstick is the CPU oracle (oracle.pdq_features): every result must equal it bit for bit -- hash bytes, quality and all 256
coefficients as uint32 views of the floats, the 8 dihedral hashes -- and must additionally equal what Engine.pdq_hash_batch returns for
that image alone.  Float-bit equality of the coefficients is what pins the thumbnails of the pre-downsample: every thumbnail pixel lies
under some Jarosz window that reaches a decimated sample.  Nothing here has a tolerance.

Images: smooth gradients plus noise from a seeded numpy generator (quality is not 0).  About 80 distinct images in all, the largest
1265x850; each reference is computed once, shared by the tests and never written to."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIDES = (128, 129, 191, 192, 193, 256, 257, 320, 384, 385, 448, 449, 511, 512)  # win = ceil(side / 64) changes at each multiple of 64, + 1


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
def image(w, h, ch, seed=0):
    """(h, w) or (h, w, ch) uint8: two gradients and a low-frequency wave + noise, per channel"""
    rng = np.random.default_rng([w, h, ch, seed])
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    planes = []
    for _ in range(ch):
        a, b, c = rng.uniform(-1, 1, 3)
        fx, fy = rng.uniform(1, 6, 2)
        p = 128 + 50 * a * (x / max(w - 1, 1) - 0.5) + 50 * b * (y / max(h - 1, 1) - 0.5) + 40 * c * np.sin(fx * x / max(w, 1) * 6.283 + fy * y / max(h, 1) * 6.283)
        planes.append(np.clip(p + rng.normal(0, 12, (h, w)), 0, 255).astype(np.uint8))
    out = planes[0] if ch == 1 else np.stack(planes, axis=2)
    out = np.ascontiguousarray(out)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(w, h, ch, seed=0):
    """(valid, hash, quality, coeffs, dihedral) of image(w, h, ch, seed) from the CPU oracle; an image the reference refuses (a side < 5):
    valid 0 and zeros"""
    o = _oracle()
    rc, coeffs, q = o.pdq_features(image(w, h, ch, seed))
    if rc != 0:
        assert w < 5 or h < 5
        out = (0, np.zeros(32, np.uint8), np.zeros(1, np.float32), np.zeros(256, np.float32), np.zeros((8, 32), np.uint8))
    else:
        out = (1, o.to_hash(coeffs), np.array([q], np.float32), coeffs, o.dihedral_hashes(coeffs))
    for a in out[1:]:
        a.setflags(write=False)
    return out


def check(out, specs, what=""):
    """the dict of a ragged call against the oracle, image by image, bit for bit"""
    assert len(out["valid"]) == len(specs)
    for i, s in enumerate(specs):
        valid, hsh, q, coeffs, dih = reference(*s)
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
        if valid and min(s[0], s[1]) >= 64:  # (the generator's images are no flat fields: a quality of 0 would compare nothing)
            assert q[0] > 0, tag


def ragged(eng, specs, **kw):
    kw = {"want_quality": True, "want_coeffs": True, "want_dihedral": True, **kw}
    return eng.pdq_hash_ragged([image(*s) for s in specs], **kw)


_ALONE = {}


def alone(eng, spec):
    """Engine.pdq_hash_batch of the one image (its default kernel selection), once per image"""
    if spec not in _ALONE:
        _ALONE[spec] = eng.pdq_hash_batch(image(*spec)[None], want_quality=True, want_coeffs=True, want_dihedral=True)
    return _ALONE[spec]


def check_against_alone(eng, out, specs):
    for i, s in enumerate(specs):
        one = alone(eng, s)
        for k in ("hash", "dihedral", "valid"):
            assert np.array_equal(out[k][i].reshape(-1), one[k][0].reshape(-1)), (k, i, s)
        for k in ("quality", "coeffs"):
            assert np.array_equal(out[k][i:i + 1].view(np.uint32).reshape(-1), one[k][0:1].view(np.uint32).reshape(-1)), (k, i, s)


def stream_specs():
    """32 (w, h) pairs over the window boundaries of the streaming kernel: the four corners inside the list, widths not divisible by 4,
    Luma8 / Rgb8 / Rgba8 interleaved so that neighbours in the work list differ in window, band count and channel count"""
    pairs = [(SIDES[k % 14], SIDES[(5 * k + 3 + 7 * (k // 14)) % 14]) for k in range(28)]
    pairs[3:3] = [(128, 128)]
    pairs[9:9] = [(128, 512)]
    pairs[17:17] = [(512, 128)]
    pairs[26:26] = [(512, 512)]
    return [(w, h, (1, 3, 4)[k % 3]) for k, (w, h) in enumerate(pairs)]


def resize_specs():
    """sources with a side > 512 as Luma8 and Rgb8; 2048x513 has the thinnest thumbnail (512x128) the descriptor kernels take; 700x1024
    twice with different pixels (one pair of axis tables)"""
    geos = [(513, 512), (512, 513), (700, 1024), (1024, 700), (1265, 850), (850, 1265), (2048, 513)]
    specs = [(w, h, ch) for w, h in geos for ch in (1, 3)]
    return specs + [(700, 1024, 1, 1), (700, 1024, 3, 1)]


FALLBACK = [(4, 100, 3), (100, 4, 1), (5, 5, 3), (64, 64, 1), (127, 300, 3), (2048, 511, 1), (4000, 5, 3), (600, 5, 1)]


def test_stream_window_boundaries_mixed(eng):
    specs = stream_specs()
    assert len(set(s[:2] for s in specs)) >= 30 and any(s[0] % 4 for s in specs)
    out = ragged(eng, specs)
    check(out, specs)
    check_against_alone(eng, out, specs)


def test_predownsample_mixed(eng):
    specs = resize_specs()
    out = ragged(eng, specs)
    check(out, specs)
    check_against_alone(eng, out, specs)


def test_fallback_classes_beside_the_others(eng):
    s, r = stream_specs(), resize_specs()
    specs = [s[0], FALLBACK[0], r[0], FALLBACK[1], FALLBACK[2], s[1], FALLBACK[3], FALLBACK[4], r[3], FALLBACK[5], FALLBACK[6], s[2], FALLBACK[7]]
    out = ragged(eng, specs)
    check(out, specs)
    check_against_alone(eng, out, specs)
    assert out["valid"].tolist() == [1, 0, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1]


def test_order_follows_the_list(eng):
    specs = stream_specs()
    perm = np.random.default_rng(5).permutation(len(specs))
    check(ragged(eng, [specs[k] for k in perm]), [specs[k] for k in perm])


# ---- layout

LAYOUT = [(191, 129, 1), (257, 193, 3), (130, 131, 4), (513, 512, 1), (700, 1024, 3), (127, 300, 3), (449, 128, 1), (600, 5, 1)]


def embedded(specs, fill):
    """every image as a slice of one byte buffer: rows padded by 1, 2, 3, 1 .. bytes, first pixels at odd addresses, the rest `fill`.
    Returns (buffer, [views], offsets, row strides)."""
    offs, strides, at = [], [], 1
    for k, (w, h, ch, *_) in enumerate(specs):
        strides.append(w * ch + 1 + k % 3)
        at |= 1
        offs.append(at)
        at += strides[-1] * h + 5
    buf = np.full(at + 16, fill, np.uint8)
    views = []
    for (w, h, ch, *rest), o, st in zip(specs, offs, strides):
        rows = np.lib.stride_tricks.as_strided(buf[o:], (h, w * ch), (st, 1))
        rows[...] = image(w, h, ch, *rest).reshape(h, w * ch)
        views.append(rows if ch == 1 else np.lib.stride_tricks.as_strided(buf[o:], (h, w, ch), (st, ch, 1)))
    return buf, views, offs, strides


def dev_call(eng, buf, offs, specs, strides, wants=(True, True, True, True), sentinel=None):
    """rph_pdq_hash_ragged_dev on an uploaded buffer; returns the dict (None for outputs not asked for)"""
    n = len(specs)
    sizes = {"hash": 32, "quality": 4, "coeffs": 1024, "dihedral": 256, "valid": 1}
    want = dict(zip(("quality", "coeffs", "dihedral", "valid"), wants), hash=True)
    d_px = eng.dev_alloc(len(buf))
    d = {k: eng.dev_alloc(max(n, 1) * b) if want[k] else None for k, b in sizes.items()}
    try:
        eng.dev_upload(d_px, buf)
        for k, p in d.items():
            if p is not None and sentinel is not None:
                eng.dev_memset(p, sentinel, max(n, 1) * sizes[k])
        eng.pdq_hash_ragged_dev(d_px, offs, [s[0] for s in specs], [s[1] for s in specs], [s[2] for s in specs], strides, d["hash"], d["quality"], d["coeffs"],
                                d["dihedral"], d["valid"])
        eng.synchronize()
        out = {}
        for k, dt, shape in (("hash", np.uint8, (n, 32)), ("quality", np.float32, (n,)), ("coeffs", np.float32, (n, 256)), ("dihedral", np.uint8, (n, 8, 32)),
                             ("valid", np.uint8, (n,))):
            out[k] = None
            if d[k] is not None:
                out[k] = np.zeros(shape, dt)
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
        assert (a[k] is None) == (b[k] is None)
        if a[k] is not None:
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


def test_row_padding_and_odd_addresses_host_form(eng):
    outs = []
    for fill in (0x00, 0xFF):
        buf, views, _, _ = embedded(LAYOUT, fill)
        assert all(v.ctypes.data % 2 == 1 for v in views)
        outs.append(eng.pdq_hash_ragged(views, want_quality=True, want_coeffs=True, want_dihedral=True))
        check(outs[-1], LAYOUT, f"fill {fill:#x}")
    same(outs[0], outs[1])


def test_row_padding_and_odd_offsets_device_form(eng):
    outs = []
    for fill in (0x00, 0xFF):
        buf, _, offs, strides = embedded(LAYOUT, fill)
        assert all(o % 2 == 1 for o in offs)
        outs.append(dev_call(eng, buf, offs, LAYOUT, strides))
        check(outs[-1], LAYOUT, f"fill {fill:#x}")
    same(outs[0], outs[1])


def test_device_form_packed(eng):
    """the packing Engine offers for the device form: 16-byte aligned images, rows on dword boundaries (Luma8 of 128..512 is read in place)"""
    from rupphash_amd.engine import ragged_pack

    specs = stream_specs()[:9] + resize_specs()[:4] + FALLBACK[:4]
    buf, off, w, h, ch, rs = ragged_pack([image(*s) for s in specs], fill=0xFF)
    check(dev_call(eng, buf, off, specs, rs), specs)


# ---- edges of the interface

def test_no_images(eng):
    out = eng.pdq_hash_ragged([])
    assert out["hash"].shape == (0, 32) and out["valid"].shape == (0,)
    assert dev_call(eng, np.zeros(16, np.uint8), [], [], [])["hash"].shape == (0, 32)


@pytest.mark.parametrize("spec", [(193, 257, 3), (1024, 700, 1), (127, 300, 3), (4, 100, 3)], ids=["S", "R", "F", "too-small"])
def test_one_image_of_each_class(eng, spec):
    check(ragged(eng, [spec]), [spec])


def test_uniform_call_is_forwarded(eng):
    specs = [(320, 257, 3, k) for k in range(5)]
    out = ragged(eng, specs)
    check(out, specs)
    ref = eng.pdq_hash_batch(np.stack([image(*s) for s in specs]), want_quality=True, want_coeffs=True, want_dihedral=True)
    same(out, ref)


@pytest.mark.parametrize("missing", ["quality", "coeffs", "dihedral", "valid"])
def test_every_nullable_output_null_in_turn(eng, missing):
    specs = [stream_specs()[4], resize_specs()[2], FALLBACK[3], FALLBACK[0], stream_specs()[5]]
    buf, views, offs, strides = embedded(specs, 0)
    wants = tuple(k != missing for k in ("quality", "coeffs", "dihedral", "valid"))
    out = dev_call(eng, buf, offs, specs, strides, wants=wants)
    assert out[missing] is None
    if out["valid"] is None:
        out["valid"] = np.array([reference(*s)[0] for s in specs], np.uint8)
    check(out, specs)
    if missing != "valid":  # the host form has the same nullable outputs; Engine always asks for valid
        host = eng.pdq_hash_ragged(views, **{f"want_{k}": k != missing for k in ("quality", "coeffs", "dihedral")})
        assert host[missing] is None
        check(host, specs)


@pytest.mark.parametrize("fault", ["channels", "row_stride"])
def test_invalid_descriptor_refuses_the_whole_call(eng, fault):
    from rupphash_amd import RphError
    from rupphash_amd._lib import RPH_ERR_INVALID_ARG

    specs = [(193, 257, 3), (1024, 700, 1), (129, 128, 1)]
    buf, views, offs, strides = embedded(specs, 0)
    w, h, ch = ([s[k] for s in specs] for k in range(3))
    if fault == "channels":
        ch[1] = 2
    else:
        strides[2] = w[2] * ch[2] - 1
    # device form: sentinel-filled outputs stay as they are
    n = len(specs)
    d_px = eng.dev_alloc(len(buf))
    d_out = eng.dev_alloc(n * 1024)
    try:
        eng.dev_upload(d_px, buf)
        eng.dev_memset(d_out, 0xA5, n * 1024)
        with pytest.raises(RphError) as e:
            eng.pdq_hash_ragged_dev(d_px, offs, w, h, ch, strides, d_out, d_out, d_out, d_out, d_out)
        assert e.value.status == RPH_ERR_INVALID_ARG
        eng.synchronize()
        back = np.zeros(n * 1024, np.uint8)
        eng.dev_download(back, d_out)
        assert np.all(back == 0xA5)
    finally:
        eng.dev_free(d_px)
        eng.dev_free(d_out)
    # host form
    px = (C.c_void_p * n)(*[v.ctypes.data for v in views])
    aw, ah, ach = (np.array(a, np.uint32) for a in (w, h, ch))
    rs = (C.c_size_t * n)(*strides)
    hsh, q, valid = np.full((n, 32), 0xA5, np.uint8), np.full(n, 7.0, np.float32), np.full(n, 0xA5, np.uint8)
    rc = eng.L.rph_pdq_hash_ragged(eng.ctx, px, aw.ctypes.data, ah.ctypes.data, ach.ctypes.data, rs, n, hsh.ctypes.data, q.ctypes.data, None, None, valid.ctypes.data)
    assert rc == RPH_ERR_INVALID_ARG
    assert np.all(hsh == 0xA5) and np.all(q == 7.0) and np.all(valid == 0xA5)
    # a null required pointer
    assert eng.L.rph_pdq_hash_ragged(eng.ctx, px, aw.ctypes.data, None, ach.ctypes.data, rs, n, hsh.ctypes.data, None, None, None, None) == RPH_ERR_INVALID_ARG
    assert eng.L.rph_pdq_hash_ragged(eng.ctx, px, aw.ctypes.data, ah.ctypes.data, ach.ctypes.data, rs, n, None, None, None, None, None) == RPH_ERR_INVALID_ARG
    assert np.all(hsh == 0xA5)


# ---- kernel selection

@pytest.mark.parametrize("mode", [5, 0, 6, 4], ids=["mode5-all-F", "mode0-all-F", "mode6", "default"])
def test_kernel_modes(eng, mode):
    """rph_pdq_set_kernel 0 and 5 ask for no single-pass kernel: every image goes through the uniform path's multi-pass kernels; 6 and the
    default (4) take the descriptor kernels.  The oracle does not care."""
    specs = stream_specs() + resize_specs()
    eng.set_pdq_kernel(mode)
    try:
        out = ragged(eng, specs)
    finally:
        eng.set_pdq_kernel(4)
    check(out, specs, f"mode {mode}")


# ---- staging chunks of the host form

def test_three_staging_chunks():
    """RPH_RAGGED_CHUNK_BYTES (read once, when the context is made) cuts a 12-image call into three staging chunks: both pinned sets are
    used, the first one twice"""
    from rupphash_amd import Engine

    specs = [(128 + 7 * k, 160 - 3 * k, (1, 3, 4)[k % 3]) for k in range(10)] + [(513, 512, 1), (100, 64, 1)]
    sizes = [-(-(w * ch) // 4) * 4 * h for w, h, ch in specs]
    limit = 300000
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
        out = ragged(e, specs)
    finally:
        e.close()
    check(out, specs)


def test_features_many(eng):
    from rupphash_amd import pdqhash

    specs = [(193, 257, 3), (4, 100, 3), (700, 1024, 1), (64, 64, 1)]
    res = pdqhash.generate_pdq_features_many([image(*s) for s in specs], engine=eng)
    assert res[1] is None
    for r, s in zip((res[0], res[2], res[3]), (specs[0], specs[2], specs[3])):
        _, hsh, q, coeffs, _ = reference(*s)
        assert np.array_equal(r[0].coefficients.view(np.uint32), coeffs.view(np.uint32)) and np.float32(r[1]).view(np.uint32) == q.view(np.uint32)[0]
        assert np.array_equal(r[0].to_hash(), hsh)
