"""The device entry points of the five file pipelines (rph_<fmt>_pdq_hash_batch, rph_<fmt>_decode, rph_<fmt>_release) held to one
contract (-m gpu), on one small valid file per format from tests/file_chunks.py: release and call again, empty and null calls, absent
optional outputs, the capacity check of the device decode (before any chunk runs), a call that mixes a valid file with a refused one and
a null one, and a context closed with all five pipelines live.  Every comparison is bit for bit."""
import ctypes as C

import numpy as np
import pytest

import file_chunks as fc

pytestmark = pytest.mark.gpu

SHAPES = dict(hash=((32,), np.uint8), quality=((), np.float32), coeffs=((256,), np.float32), dihedral=((8, 32), np.uint8), valid=((), np.uint8),
              status=((), np.int32), pixel_hash=((32,), np.uint8))
assert tuple(SHAPES) == fc.KEYS  # (the order of the C arguments behind n_threads)


@pytest.fixture(scope="module")
def eng():
    from rupphash_amd import Engine

    e = Engine(0)
    yield e
    e.close()


def small_file(fmt):
    """the pool's first valid file that PDQ takes (5 px a side at least)"""
    from rupphash_amd import Engine

    return next(f for f in fc.of_kind(fmt, "ok") if min(getattr(Engine, fmt + "_info")(f.data)[:2]) >= 5)


def refused_file(fmt):
    """the pool's first file that rph_<fmt>_info refuses (so does every entry point, before it touches the device)"""
    from rupphash_amd import Engine

    return next(f for f in fc.of_kind(fmt, "parse") if fc._status(getattr(Engine, fmt + "_info"), f.data))


def batch(e, fmt, datas):
    return getattr(e, fmt + "_pdq_hash_batch")(datas, want_coeffs=True, want_dihedral=True, want_pixel_hash=True)


def raw_batch(e, fmt, datas, lens, given):
    """rph_<fmt>_pdq_hash_batch through the C ABI with the outputs named in `given` (the others null), every given array filled with 0xa5
    first: -> (return code, {key: array})"""
    n = len(datas)
    out = {k: np.empty((n,) + SHAPES[k][0], SHAPES[k][1]) for k in given}
    for a in out.values():
        a.view(np.uint8)[...] = 0xa5
    arr, ln = (C.c_char_p * n)(*datas), (C.c_size_t * n)(*lens)
    ptr = lambda k: out[k].ctypes.data_as(C.c_void_p) if k in out else None
    rc = getattr(e.L, f"rph_{fmt}_pdq_hash_batch")(e.ctx, arr, ln, n, 0, *[ptr(k) for k in fc.KEYS])
    return rc, out


def same(a, b, keys=fc.KEYS):
    for key in keys:
        x, y = np.asarray(a[key]), np.asarray(b[key])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), key


@pytest.mark.parametrize("fmt", fc.FORMATS)
def test_release_and_call_again(eng, fmt):
    from rupphash_amd import _lib

    data = small_file(fmt).data
    first = batch(eng, fmt, [data])
    assert first["status"][0] == 0 and first["valid"][0] == 1 and first["hash"].any() and first["pixel_hash"].any()
    release = getattr(eng.L, f"rph_{fmt}_release")
    assert release(eng.ctx) == _lib.RPH_OK
    same(first, batch(eng, fmt, [data]))
    for _ in range(3):  # (the first of these returns the buffers, the others find none)
        assert release(eng.ctx) == _lib.RPH_OK
    assert release(None) == _lib.RPH_ERR_INVALID_ARG


@pytest.mark.parametrize("fmt", fc.FORMATS)
def test_empty_and_null_calls(eng, fmt):
    from rupphash_amd import _lib

    call = getattr(eng.L, f"rph_{fmt}_pdq_hash_batch")
    assert call(eng.ctx, None, None, 0, 0, None, None, None, None, None, None, None) == _lib.RPH_OK
    f = small_file(fmt)
    ref = batch(eng, fmt, [f.data])
    before = eng.debug_file_chunks(fmt)
    assert before[0] == [1]
    assert call(eng.ctx, None, None, 0, 0, None, None, None, None, None, None, None) == _lib.RPH_OK
    rc, out = raw_batch(eng, fmt, [f.data], [len(f.data)], [k for k in fc.KEYS if k != "hash"])
    assert rc == _lib.RPH_ERR_INVALID_ARG and f"rph_{fmt}_pdq_hash_batch".encode() in eng.L.rph_last_error()
    assert all((np.asarray(v).view(np.uint8) == 0xa5).all() for v in out.values())  # refused before anything was written
    arr, ln = (C.c_char_p * 1)(f.data), (C.c_size_t * 1)(len(f.data))
    h = np.zeros(32, np.uint8)
    hp = h.ctypes.data_as(C.c_void_p)
    assert call(eng.ctx, None, ln, 1, 0, hp, None, None, None, None, None, None) == _lib.RPH_ERR_INVALID_ARG
    assert call(eng.ctx, arr, None, 1, 0, hp, None, None, None, None, None, None) == _lib.RPH_ERR_INVALID_ARG
    assert call(None, arr, ln, 1, 0, hp, None, None, None, None, None, None) == _lib.RPH_ERR_INVALID_ARG
    assert eng.debug_file_chunks(fmt) == before  # none of these ran a chunk or reset the log
    same(ref, batch(eng, fmt, [f.data]))


@pytest.mark.parametrize("fmt", fc.FORMATS)
def test_optional_outputs(eng, fmt):
    from rupphash_amd import _lib

    f, bad = small_file(fmt), refused_file(fmt)
    datas, lens = [f.data, bad.data, f.data], [len(f.data), len(bad.data), len(f.data)]
    rc, full = raw_batch(eng, fmt, datas, lens, fc.KEYS)
    assert rc == _lib.RPH_OK and list(full["status"] != 0) == [False, True, False] and list(full["valid"]) == [1, 0, 1]
    same(full, batch(eng, fmt, datas))
    rc, part = raw_batch(eng, fmt, datas, lens, [k for k in fc.KEYS if k not in ("status", "valid")])
    assert rc == _lib.RPH_OK
    same(full, part, ("hash", "quality", "coeffs", "dihedral", "pixel_hash"))
    rc, only = raw_batch(eng, fmt, datas, lens, ["hash"])
    assert rc == _lib.RPH_OK
    same(full, only, ("hash",))
    assert not full["hash"][1].any() and full["hash"][0].any()  # (the refused file's row was zero-filled, not left at 0xa5)


@pytest.mark.parametrize("fmt", fc.FORMATS)
def test_device_decode_capacity(eng, fmt):
    from rupphash_amd import Engine, _lib

    f = small_file(fmt)
    want = getattr(Engine, fmt + "_decode_host")(f.data)
    decode = getattr(eng.L, f"rph_{fmt}_decode")
    bad = refused_file(fmt)
    batch(eng, fmt, [f.data, bad.data, f.data])
    before = eng.debug_file_chunks(fmt)
    assert before[0] == [2]
    buf = np.full(want.nbytes + 16, 0xa5, np.uint8)
    bp = buf.ctypes.data_as(C.c_void_p)
    assert decode(eng.ctx, f.data, len(f.data), bp, want.nbytes - 1) == _lib.RPH_ERR_CAPACITY
    err = eng.L.rph_last_error()
    assert f"rph_{fmt}_decode: {want.nbytes} bytes needed".encode() == err
    assert decode(eng.ctx, None, len(f.data), bp, want.nbytes) == _lib.RPH_ERR_INVALID_ARG
    assert decode(eng.ctx, f.data, len(f.data), None, want.nbytes) == _lib.RPH_ERR_INVALID_ARG
    assert decode(None, f.data, len(f.data), bp, want.nbytes) == _lib.RPH_ERR_INVALID_ARG
    assert decode(eng.ctx, bad.data, len(bad.data), bp, buf.nbytes) not in (_lib.RPH_OK, _lib.RPH_ERR_CAPACITY)
    assert (buf == 0xa5).all() and eng.debug_file_chunks(fmt) == before  # no chunk ran
    assert decode(eng.ctx, f.data, len(f.data), bp, want.nbytes) == _lib.RPH_OK
    assert buf[:want.nbytes].tobytes() == want.tobytes() and (buf[want.nbytes:] == 0xa5).all()
    assert eng.debug_file_chunks(fmt)[0] == [1]
    got = getattr(eng, fmt + "_decode")(f.data)
    assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


@pytest.mark.parametrize("fmt", fc.FORMATS)
def test_mixed_statuses(eng, fmt):
    from rupphash_amd import _lib

    f, bad = small_file(fmt), refused_file(fmt)
    alone = batch(eng, fmt, [f.data])
    rc, out = raw_batch(eng, fmt, [f.data, bad.data, f.data], [len(f.data), len(bad.data), 0], fc.KEYS)
    assert rc == _lib.RPH_OK
    for key in fc.KEYS:
        assert np.asarray(out[key][0]).tobytes() == np.asarray(alone[key][0]).tobytes(), key
    assert out["status"][1] != 0 and out["status"][2] == _lib.RPH_ERR_INVALID_ARG
    for key in fc.KEYS:
        if key != "status":
            assert not np.asarray(out[key][1:]).view(np.uint8).any(), key
    assert eng.debug_file_chunks(fmt)[0] == [1]
    # a null file pointer gets the same status as a null length
    n = 2
    arr, ln = (C.c_char_p * n)(None, f.data), (C.c_size_t * n)(len(f.data), len(f.data))
    h, st = np.full((n, 32), 0xa5, np.uint8), np.full(n, 77, np.int32)
    assert getattr(eng.L, f"rph_{fmt}_pdq_hash_batch")(eng.ctx, arr, ln, n, 0, h.ctypes.data_as(C.c_void_p), None, None, None, None,
                                                        st.ctypes.data_as(C.c_void_p), None) == _lib.RPH_OK
    assert list(st) == [_lib.RPH_ERR_INVALID_ARG, 0] and not h[0].any() and h[1].tobytes() == alone["hash"][0].tobytes()


def test_context_closed_with_every_pipeline_live():
    from rupphash_amd import Engine

    files = {fmt: small_file(fmt).data for fmt in fc.FORMATS}
    outs = []
    for _ in range(2):
        e = Engine(0)
        try:
            outs.append({fmt: batch(e, fmt, [files[fmt]]) for fmt in fc.FORMATS})
            assert all(e.debug_file_chunks(fmt)[0] == [1] for fmt in fc.FORMATS)
        finally:
            e.close()  # (all five pipes hold their stream and buffers here)
    for fmt in fc.FORMATS:
        assert outs[0][fmt]["status"][0] == 0 and outs[0][fmt]["valid"][0] == 1
        same(outs[0][fmt], outs[1][fmt])
