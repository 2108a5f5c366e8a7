"""The ragged PDQ call (rph_pdq_hash_ragged / rph_pdq_hash_ragged_dev: images of any mix of sizes in one call) as far as it can be held
without a GPU: the two symbols are exported by the built library and bound with the header's arity, the generated Rust binding declares
them, the Python layers above them exist, and the Python packing of a list of images (offsets, pitches, descriptor arrays) is what the
device form is documented to take.  The kernels themselves: tests/test_ragged_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rph_pdq_hash_ragged", "rph_pdq_hash_ragged_dev")


def _prototype(name):
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "rupphash.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", header, flags=re.S)
    assert m, f"{name} is not declared in include/rupphash.h"
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", NAMES)
def test_symbols_are_exported_and_bound(name):
    from rupphash_amd import _lib

    L = _lib.load()  # without a device too: loading binds every entry of SIGNATURES and raises on a missing export
    assert name in _lib.SIGNATURES
    res, args = _lib.SIGNATURES[name]
    assert res is C.c_int and len(args) == len(_prototype(name))
    assert getattr(L, name).argtypes == args


def test_prototypes_are_the_documented_ones():
    host, dev = _prototype(NAMES[0]), _prototype(NAMES[1])
    assert host[1].replace(" ", "") == "constuint8_t*const*px" and host[5].replace(" ", "") == "constsize_t*row_stride" and host[6] == "uint32_t n"
    assert dev[1].replace(" ", "") == "constvoid*d_px" and dev[2].replace(" ", "") == "constuint64_t*offset" and dev[-1].replace(" ", "") == "void*stream"
    header = open(os.path.join(ROOT, "include", "rupphash.h")).read()
    assert re.search(r"#define\s+RPH_ABI_VERSION\s+1\b", header), "additive: the ABI version stays 1"


def test_rust_binding_declares_them():
    rs = open(os.path.join(ROOT, "rust", "rph_ffi.rs")).read()
    m = re.search(r"pub fn rph_pdq_hash_ragged\((.*?)\) -> c_int;", rs)
    assert m and "px: *const *const u8" in m.group(1) and "row_stride: *const usize" in m.group(1) and len(m.group(1).split(",")) == 12
    m = re.search(r"pub fn rph_pdq_hash_ragged_dev\((.*?)\) -> c_int;", rs)
    assert m and "offset: *const u64" in m.group(1) and "stream: *mut c_void" in m.group(1) and len(m.group(1).split(",")) == 14


def test_python_and_cpp_layers_exist():
    from rupphash_amd import Engine, engine, pdqhash

    assert callable(Engine.pdq_hash_ragged) and callable(Engine.pdq_hash_ragged_dev)
    assert callable(pdqhash.generate_pdq_features_many) and callable(engine.ragged_pack)
    hpp = open(os.path.join(ROOT, "include", "rupphash.hpp")).read()
    assert "generate_pdq_features_many" in hpp and "rph_pdq_hash_ragged(" in hpp


def test_packing_of_a_hand_written_list():
    """offsets on 16-byte boundaries in list order, rows at w * channels rounded up to 4, every pixel where the descriptor says, the rest fill"""
    from rupphash_amd.engine import ragged_pack

    rng = np.random.default_rng(7)
    shapes = [(3, 5), (2, 7, 3), (1, 1, 4), (4, 16), (5, 3, 3), (0, 9), (2, 6, 4)]  # (h, w[, ch])
    imgs = [rng.integers(1, 255, s, dtype=np.uint8) for s in shapes]
    buf, off, w, h, ch, rs = ragged_pack(imgs, fill=0xEE)
    assert (off.dtype, w.dtype, h.dtype, ch.dtype, rs.dtype) == (np.uint64, np.uint32, np.uint32, np.uint32, np.uintp)
    #            3x5 L8   2x7 Rgb8   1x1 Rgba8   4x16 L8   5x3 Rgb8   0x9   2x6 Rgba8
    assert rs.tolist() == [8, 24, 4, 16, 12, 12, 24]
    assert off.tolist() == [0, 32, 80, 96, 160, 224, 224]
    assert w.tolist() == [5, 7, 1, 16, 3, 9, 6] and h.tolist() == [3, 2, 1, 4, 5, 0, 2] and ch.tolist() == [1, 3, 4, 1, 3, 1, 4]
    assert len(buf) == 224 + 2 * 24
    seen = np.zeros(len(buf), bool)
    for i, im in enumerate(imgs):
        row = int(w[i] * ch[i])
        for y in range(int(h[i])):
            at = int(off[i]) + y * int(rs[i])
            assert np.array_equal(buf[at:at + row], im[y].reshape(-1)), (i, y)
            seen[at:at + row] = True
    assert np.all(buf[~seen] == 0xEE)


def test_views_of_larger_arrays_are_taken_as_they_are():
    """a slice with padded rows is passed where it lies (pointer and row stride), anything else is copied"""
    from rupphash_amd.engine import _ragged_view

    big = np.zeros((10, 40), np.uint8)
    a, h, w, ch, stride = _ragged_view(big[1:7, 3:20])
    assert (h, w, ch, stride) == (6, 17, 1, 40) and a.ctypes.data == big.ctypes.data + 43
    rgb = np.zeros((6, 9, 3), np.uint8)
    a, h, w, ch, stride = _ragged_view(rgb[:, 1:8])
    assert (h, w, ch, stride) == (6, 7, 3, 27) and a.ctypes.data == rgb.ctypes.data + 3
    a, h, w, ch, stride = _ragged_view(big[:, ::2])  # pixels not adjacent: a copy
    assert (h, w, ch, stride) == (10, 20, 1, 20) and a.flags.c_contiguous
    a, h, w, ch, stride = _ragged_view(big[::-1])  # rows backwards: a copy
    assert stride == 40 and a.flags.c_contiguous
    with pytest.raises(ValueError):
        _ragged_view(np.zeros((4, 4, 2), np.uint8))
