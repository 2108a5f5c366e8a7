"""The host-only entry points of the five file pipelines (rph_<fmt>_info, rph_<fmt>_decode_host) held to one contract through the C ABI,
on one small valid file per format from tests/file_chunks.py (no GPU): which out-pointers may be null, what a null argument and a
capacity one byte short return, and that exact capacity gives the array Engine.<fmt>_decode_host gives."""
import ctypes as C
import itertools

import numpy as np
import pytest

import file_chunks as fc


def small_file(fmt):
    """the pool's first valid file of more than one pixel (its byte count then differs from the capacity of no other argument)"""
    from rupphash_amd import Engine

    return next(f.data for f in fc.of_kind(fmt, "ok") if np.prod(getattr(Engine, fmt + "_info")(f.data)[:2]) > 1)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("fmt", fc.FORMATS)
def test_info_takes_any_subset_of_its_out_pointers(fmt):
    from rupphash_amd import Engine, _lib

    info = getattr(_lib.load(), f"rph_{fmt}_info")
    data = small_file(fmt)
    want = getattr(Engine, fmt + "_info")(data)
    assert len(want) == 4 and want[0] >= 1 and want[1] >= 1 and want[2] in (1, 2, 3, 4) and want[3] in (8, 16)
    for given in itertools.product((False, True), repeat=4):
        slots = [C.c_uint32(0xdeadbeef) for _ in range(4)]
        assert info(data, len(data), *[C.byref(s) if g else None for s, g in zip(slots, given)]) == _lib.RPH_OK, given
        for k in range(4):
            assert slots[k].value == (want[k] if given[k] else 0xdeadbeef), (given, k)


@pytest.mark.parametrize("fmt", fc.FORMATS)
def test_info_refuses_null_data(fmt):
    from rupphash_amd import _lib

    info = getattr(_lib.load(), f"rph_{fmt}_info")
    w = C.c_uint32(7)
    assert info(None, 0, C.byref(w), None, None, None) == _lib.RPH_ERR_INVALID_ARG
    assert info(None, 100, None, None, None, None) == _lib.RPH_ERR_INVALID_ARG
    assert w.value == 7


@pytest.mark.parametrize("fmt", fc.FORMATS)
def test_decode_host_capacity(fmt):
    from rupphash_amd import Engine, _lib

    decode = getattr(_lib.load(), f"rph_{fmt}_decode_host")
    data = small_file(fmt)
    want = getattr(Engine, fmt + "_decode_host")(data)
    w, h, c, d = getattr(Engine, fmt + "_info")(data)
    assert want.nbytes == w * h * c * (d // 8)
    buf = np.full(want.nbytes + 16, 0xa5, np.uint8)
    assert decode(data, len(data), _vp(buf), want.nbytes - 1) == _lib.RPH_ERR_CAPACITY
    assert str(want.nbytes).encode() in _lib.load().rph_last_error() and f"rph_{fmt}_decode_host".encode() in _lib.load().rph_last_error()
    assert (buf == 0xa5).all()  # nothing written by the refused call
    assert decode(data, len(data), _vp(buf), 0) == _lib.RPH_ERR_CAPACITY
    assert decode(data, len(data), _vp(buf), want.nbytes) == _lib.RPH_OK
    assert buf[:want.nbytes].tobytes() == want.tobytes() and (buf[want.nbytes:] == 0xa5).all()


@pytest.mark.parametrize("fmt", fc.FORMATS)
def test_decode_host_refuses_null_arguments(fmt):
    from rupphash_amd import _lib

    decode = getattr(_lib.load(), f"rph_{fmt}_decode_host")
    data = small_file(fmt)
    buf = np.full(64, 0xa5, np.uint8)
    assert decode(None, 0, _vp(buf), 64) == _lib.RPH_ERR_INVALID_ARG
    assert decode(None, len(data), _vp(buf), 64) == _lib.RPH_ERR_INVALID_ARG
    assert decode(data, len(data), None, 1 << 30) == _lib.RPH_ERR_INVALID_ARG
    assert (buf == 0xa5).all()
