"""rph_image_hash_ragged / rph_image_hash_ragged_dev (decoded images of any mix of sizes and of the eight layouts Luma/LumaA/Rgb/Rgba x
8/16 bit in one call: PDQ outputs and the pixel hash) as far as they can be held without a GPU: the symbols, the layout codes, the
bindings and layers above them, the Python packing, and the two context-free host restatements rph_image_luma601_host and
rph_image_pixel_hash_host against the numpy restatements of tests/png_util.py and the CPU oracle.  The kernels: tests/test_image_layouts_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import blake3_util
import oracle
import png_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rph_image_hash_ragged", "rph_image_hash_ragged_dev", "rph_image_luma601_host", "rph_image_pixel_hash_host")
LAYOUTS = {"RPH_LAYOUT_LUMA8": 1, "RPH_LAYOUT_LUMAA8": 2, "RPH_LAYOUT_RGB8": 3, "RPH_LAYOUT_RGBA8": 4,
           "RPH_LAYOUT_LUMA16": 17, "RPH_LAYOUT_LUMAA16": 18, "RPH_LAYOUT_RGB16": 19, "RPH_LAYOUT_RGBA16": 20}
SIZES = [(0, 7), (1, 1), (3, 5), (129, 67)]  # (h, w)


def _prototype(name):
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "rupphash.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", header, flags=re.S)
    assert m, f"{name} is not declared in include/rupphash.h"
    return [a.strip() for a in m.group(1).split(",")]


def image_of(rng, layout, h, w):
    """a random image of a layout code: uint8 / uint16, (h, w) or (h, w, channels)"""
    ch, dt = layout & 15, (np.uint16 if layout > 16 else np.uint8)
    return rng.integers(0, np.iinfo(dt).max + 1, (h, w) if ch == 1 else (h, w, ch), dtype=dt)


def luma_of(img):
    """the Luma8 plane the hasher sees, in numpy: hasher_pixels, then the 601 luma (Luma8 borrowed)"""
    p = png_util.hasher_pixels(img)
    return np.ascontiguousarray(p) if p.ndim == 2 else oracle.luma601(np.ascontiguousarray(p))


def padded(img, pad_bytes, fill):
    """the same pixels as a view into a buffer whose rows carry pad_bytes more bytes, all other bytes `fill`"""
    h, w = img.shape[:2]
    row = (img.size // h if h else w * (img.shape[2] if img.ndim == 3 else 1)) * img.dtype.itemsize
    buf = np.full((h, row + pad_bytes), fill, np.uint8)
    buf[:, :row] = np.ascontiguousarray(img).view(np.uint8).reshape(h, row)
    v = buf[:, :row].view(img.dtype)  # rows row + pad_bytes apart
    return v if img.ndim == 2 else np.lib.stride_tricks.as_strided(v, img.shape, (row + pad_bytes,) + img.strides[1:])


@pytest.mark.parametrize("name", NAMES)
def test_symbols_are_exported_and_bound(name):
    from rupphash_amd import _lib

    L = _lib.load()
    assert name in _lib.SIGNATURES
    res, args = _lib.SIGNATURES[name]
    assert res is C.c_int and len(args) == len(_prototype(name))
    assert getattr(L, name).argtypes == args


def test_prototypes_layout_codes_and_abi_version():
    from rupphash_amd import _lib

    host, dev = _prototype(NAMES[0]), _prototype(NAMES[1])
    assert host[1].replace(" ", "") == "constvoid*const*px" and host[4].replace(" ", "") == "constuint32_t*layout" and host[6] == "uint32_t n"
    assert host[-1].replace(" ", "") == "uint8_t*pixel_hash32_out" and len(host) == 13
    assert dev[1].replace(" ", "") == "constvoid*d_px" and dev[2].replace(" ", "") == "constuint64_t*offset" and len(dev) == 15
    assert dev[-2].replace(" ", "") == "void*d_pixel_hash32" and dev[-1].replace(" ", "") == "void*stream"
    header = open(os.path.join(ROOT, "include", "rupphash.h")).read()
    assert re.search(r"#define\s+RPH_ABI_VERSION\s+1\b", header), "additive: the ABI version stays 1"
    for name, code in LAYOUTS.items():
        assert re.search(r"#define\s+" + name + r"\s+" + str(code) + r"\b", header), name
        assert getattr(_lib, name) == code
        assert code == (code & 15) + (16 if name.endswith("16") else 0)


def test_rust_binding_declares_them():
    rs = open(os.path.join(ROOT, "rust", "rph_ffi.rs")).read()
    m = re.search(r"pub fn rph_image_hash_ragged\((.*?)\) -> c_int;", rs)
    assert m and "px: *const *const c_void" in m.group(1) and "layout: *const u32" in m.group(1) and len(m.group(1).split(",")) == 13
    m = re.search(r"pub fn rph_image_hash_ragged_dev\((.*?)\) -> c_int;", rs)
    assert m and "offset: *const u64" in m.group(1) and "d_pixel_hash32: *mut c_void" in m.group(1) and len(m.group(1).split(",")) == 15
    assert "pub const RPH_LAYOUT_RGBA16: i32 = 20;" in rs
    wrapper = open(os.path.join(ROOT, "rust", "pdqhash.rs")).read()
    assert "ImageRgb16" in wrapper and "rph_image_hash_ragged" in wrapper


def test_python_and_cpp_layers_exist():
    from rupphash_amd import Engine, engine, pdqhash, scanner

    assert callable(Engine.image_hash_ragged) and callable(Engine.image_hash_ragged_dev) and callable(engine.image_pack)
    assert callable(scanner.hash_images) and callable(pdqhash.generate_pdq_features_many)
    hpp = open(os.path.join(ROOT, "include", "rupphash.hpp")).read()
    assert "uint32_t bit_depth = 8;" in hpp and "hash_images" in hpp and "rph_image_hash_ragged(" in hpp


def test_packing_of_a_hand_written_list():
    """offsets on 16-byte boundaries in list order (so even for 16-bit images), rows at their bytes rounded up to 4, every sample where the
    descriptor says in native byte order, the rest fill"""
    from rupphash_amd.engine import image_pack

    rng = np.random.default_rng(11)
    #        3x5 L8   2x7 LA8    2x3 L16    1x1 Rgba8  3x3 Rgb16  0x9 LA16   2x5 Rgb8   2x1 Rgba16  1x3 LA16
    specs = [(1, 3, 5), (2, 2, 7), (17, 2, 3), (4, 1, 1), (19, 3, 3), (18, 0, 9), (3, 2, 5), (20, 2, 1), (18, 1, 3)]
    imgs = [image_of(rng, lay, h, w) for lay, h, w in specs]
    buf, off, w, h, lay, rs = image_pack(imgs, fill=0xEE)
    assert (off.dtype, w.dtype, h.dtype, lay.dtype, rs.dtype) == (np.uint64, np.uint32, np.uint32, np.uint32, np.uintp)
    assert lay.tolist() == [s[0] for s in specs] and h.tolist() == [s[1] for s in specs] and w.tolist() == [s[2] for s in specs]
    assert rs.tolist() == [8, 16, 8, 4, 20, 36, 16, 8, 12]
    assert off.tolist() == [0, 32, 64, 80, 96, 160, 160, 192, 208]
    assert len(buf) == 208 + 12
    assert all(int(o) % 2 == 0 and int(r) % 2 == 0 for o, r, l in zip(off, rs, lay) if l > 16)
    seen = np.zeros(len(buf), bool)
    for i, im in enumerate(imgs):
        row = int(w[i]) * (int(lay[i]) & 15) * im.dtype.itemsize
        for y in range(int(h[i])):
            at = int(off[i]) + y * int(rs[i])
            assert np.array_equal(buf[at:at + row].view(im.dtype), im[y].reshape(-1)), (i, y)
            seen[at:at + row] = True
    assert np.all(buf[~seen] == 0xEE)
    # an unaligned packing for the device tests: 16-bit images stay at even offsets with even pitches
    buf, off, w, h, lay, rs = image_pack(imgs, align=1, pitch_align=1)
    assert all(int(o) % 2 == 0 and int(r) % 2 == 0 for o, r, l in zip(off, rs, lay) if l > 16)
    assert rs.tolist() == [5, 14, 6, 4, 18, 36, 15, 8, 12]


def test_views_of_every_layout_are_taken_as_they_are():
    from rupphash_amd.engine import _image_view

    big = np.zeros((10, 40), np.uint16)
    a, h, w, lay, stride = _image_view(big[1:7, 3:20])
    assert (h, w, lay, stride) == (6, 17, 17, 80) and a.ctypes.data == big.ctypes.data + 86
    la = np.zeros((6, 9, 2), np.uint8)
    a, h, w, lay, stride = _image_view(la[:, 1:8])
    assert (h, w, lay, stride) == (6, 7, 2, 18) and a.ctypes.data == la.ctypes.data + 2
    rgba = np.zeros((4, 5, 4), np.uint16)
    a, h, w, lay, stride = _image_view(rgba[::-1])  # rows backwards: a copy
    assert (lay, stride) == (20, 40) and a.flags.c_contiguous
    assert _image_view(np.zeros((3, 3), ">u2"))[0].dtype == np.uint16  # foreign byte order: converted
    with pytest.raises(ValueError):
        _image_view(np.zeros((4, 4, 5), np.uint8))


@pytest.mark.parametrize("layout", sorted(LAYOUTS.values()))
def test_host_restatements_against_numpy(layout):
    """every size of the list, packed rows and rows with padding (0xFF and 0x00 around the pixels)"""
    from rupphash_amd import Engine

    rng = np.random.default_rng(100 + layout)
    bps = 2 if layout > 16 else 1
    for h, w in SIZES:
        img = image_of(rng, layout, h, w)
        for pad, fill in ((0, 0), (bps, 0xFF), (3 * bps, 0x00)):
            view = padded(img, pad, fill) if h else img
            assert np.array_equal(Engine.image_luma601_host(view), luma_of(img)), (layout, h, w, pad)
            want = blake3_util.blake3(png_util.to_rgba16(img))
            assert Engine.image_pixel_hash_host(view) == want, (layout, h, w, pad)


@pytest.mark.parametrize("layout", [17, 18, 19, 20])
def test_all_65536_sample_values_once(layout):
    """every u16 value in every channel position: the rounding (v + 128) / 257 and the RGBA16 stream"""
    from rupphash_amd import Engine

    ch = layout & 15
    v = np.arange(65536, dtype=np.uint16)
    img = np.stack([np.roll(v, 7919 * k) for k in range(ch)], axis=-1).reshape(256, 256, ch)
    img = img[:, :, 0] if ch == 1 else img
    assert np.array_equal(Engine.image_luma601_host(img), luma_of(img))
    assert Engine.image_pixel_hash_host(img) == blake3_util.blake3(png_util.to_rgba16(img))


@pytest.mark.parametrize("layout", [1, 2, 3, 4])
def test_all_256_sample_values_once(layout):
    from rupphash_amd import Engine

    ch = layout & 15
    v = np.arange(256, dtype=np.uint8)
    img = np.stack([np.roll(v, 37 * k) for k in range(ch)], axis=-1).reshape(16, 16, ch)
    img = img[:, :, 0] if ch == 1 else img
    assert np.array_equal(Engine.image_luma601_host(img), luma_of(img))
    assert Engine.image_pixel_hash_host(img) == blake3_util.blake3(png_util.to_rgba16(img))


@pytest.mark.parametrize("layout", [2, 17, 18, 19, 20])
def test_host_luma_as_luma8_is_the_oracle_on_to_rgb8(layout):
    """the reference does everything behind to_luma601 from the luma plane: the host luma fed to the oracle as Luma8 gives the features the
    oracle gives for the numpy to_rgb8 conversion"""
    from rupphash_amd import Engine

    rng = np.random.default_rng(layout)
    yy, xx = np.mgrid[0:150, 0:131]
    ch, top = layout & 15, (65535 if layout > 16 else 255)
    base = ((np.sin(xx / 9.0) + np.cos(yy / 13.0) + 2) / 4 * top)[:, :, None] * np.linspace(1.0, 0.6, ch)[None, None, :]
    img = np.clip(base + rng.integers(0, top // 16, base.shape), 0, top).astype(np.uint16 if layout > 16 else np.uint8)
    img = img[:, :, 0] if ch == 1 else img
    rc_a, coeffs_a, q_a = oracle.pdq_features(Engine.image_luma601_host(img))
    rc_b, coeffs_b, q_b = oracle.pdq_features(np.ascontiguousarray(png_util.hasher_pixels(img)))
    assert rc_a == rc_b == oracle.REF_OK
    assert np.array_equal(coeffs_a.view(np.uint32), coeffs_b.view(np.uint32)) and q_a == q_b


def test_sixteen_bit_input_is_no_longer_truncated():
    """np.asarray(image, np.uint8) wraps a uint16 image to its low bytes; the hasher's pixels are (v + 128) / 257.  pdqhash routes such an
    array to the call that knows its layout (checked here with the host functions alone)."""
    from rupphash_amd import Engine, pdqhash

    rng = np.random.default_rng(5)
    img = rng.integers(0, 65536, (40, 33, 3), dtype=np.uint16)
    assert pdqhash._other_layout(img) and pdqhash._other_layout(np.zeros((4, 4, 2), np.uint8))
    assert not pdqhash._other_layout(np.zeros((4, 4, 3), np.uint8)) and not pdqhash._other_layout(np.zeros((4, 4), np.uint8))
    right = Engine.image_luma601_host(img)
    assert np.array_equal(right, oracle.luma601(((img.astype(np.uint32) + 128) // 257).astype(np.uint8)))
    assert not np.array_equal(right, oracle.luma601(img.astype(np.uint8)))


def test_refused_descriptors_on_the_host():
    from rupphash_amd import _lib

    L = _lib.load()
    px = np.zeros(64, np.uint16)
    out = np.full(64, 0xAB, np.uint8)
    p, o = C.c_void_p(px.ctypes.data), C.c_void_p(out.ctypes.data)
    for fn in (L.rph_image_luma601_host, L.rph_image_pixel_hash_host):
        assert fn(p, 2, 2, 5, 16, o) == _lib.RPH_ERR_INVALID_ARG       # no such layout
        assert fn(p, 2, 2, 21, 16, o) == _lib.RPH_ERR_INVALID_ARG
        assert fn(p, 2, 2, 0, 16, o) == _lib.RPH_ERR_INVALID_ARG
        assert fn(p, 2, 2, 19, 11, o) == _lib.RPH_ERR_INVALID_ARG      # row_stride below the row's 12 bytes
        assert fn(p, 2, 2, 19, 13, o) == _lib.RPH_ERR_INVALID_ARG      # odd row_stride of a 16-bit image
        assert fn(C.c_void_p(px.ctypes.data + 1), 2, 2, 17, 4, o) == _lib.RPH_ERR_INVALID_ARG  # odd address of a 16-bit image
        assert fn(p, 1 << 21, 1 << 20, 1, 1 << 21, o) == _lib.RPH_ERR_INVALID_ARG  # more than 2^40 pixels
        assert np.all(out == 0xAB)
