"""TIFF LZW and PackBits on the device (-m gpu) on the code-level streams of lzw_streams.py, with decompression forced to the device:
decoded pixels (every byte of every strip) against the expansion of the codes, batch statuses, pixel hashes against a BLAKE3 of the
expected pixels, PDQ outputs against the CPU oracle on them, refused streams refused with zero outputs and their neighbours untouched,
the same arrays in the HOST, DEVICE and AUTO modes, and every file alone as in one shuffled call of all of them."""
import functools

import numpy as np
import pytest

import blake3_util as b3
import lzw_streams as ls
import tiff_util as tu

pytestmark = pytest.mark.gpu

HOST, DEVICE, AUTO = 0, 1, 2
KEYS = ("hash", "quality", "valid", "status", "pixel_hash")


@pytest.fixture(scope="module")
def eng():
    from rupphash_amd import Engine

    e = Engine(0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def group_files(group):
    return [f for f in ls.valid_streams() if f[0].startswith(ls.GROUPS[group])]


def _check_hashes(oracle, out, k, name, px):
    assert out["pixel_hash"][k].tobytes() == b3.blake3(tu.to_rgba16(px)), name
    if px.shape[0] < 5 or px.shape[1] < 5:
        assert out["valid"][k] == 0 and not out["hash"][k].any() and out["quality"][k] == 0, name
        return
    rc, coeffs, q = oracle.pdq_features(np.ascontiguousarray(np.repeat(px[:, :, None], 3, axis=2)))
    assert rc == 0 and out["valid"][k] == 1, name
    assert np.array_equal(out["hash"][k], oracle.to_hash(coeffs)) and out["quality"][k] == np.float32(q), name


def test_groups_leave_no_stream_out():
    names = [f[0] for f in ls.valid_streams()]
    assert sorted(f[0] for g in ls.GROUPS for f in group_files(g)) == sorted(names) and len(names) >= 230


@pytest.mark.parametrize("group", list(ls.GROUPS))
def test_device_decode_and_batch_equal_the_expansion(eng, oracle, group):
    files = group_files(group)
    assert files
    eng.tiff_set_decompress(DEVICE)
    try:
        for name, data, px in files:
            got = eng.tiff_decode(data)  # (the many-strip files: every byte of every strip)
            assert got.dtype == np.uint8 and got.shape == px.shape and got.tobytes() == px.tobytes(), name
        out = eng.tiff_pdq_hash_batch([d for _, d, _ in files], want_pixel_hash=True)
    finally:
        eng.tiff_set_decompress(AUTO)
    assert not out["status"].any(), [files[k][0] for k in np.nonzero(out["status"])[0]]
    for k, (name, _, px) in enumerate(files):
        _check_hashes(oracle, out, k, name, px)


def test_device_refuses_every_refused_stream_and_leaves_its_neighbours(eng, oracle):
    from rupphash_amd import RphError

    refused = ls.refused_streams()
    good = [f for f in ls.valid_streams() if f[0].startswith(("full_", "code_", "size_", "pb_literal_", "strips_"))]
    mixed = []  # a valid stream on either side of every refused one
    for k, (name, data) in enumerate(refused):
        mixed += [good[k % len(good)], (name, data, None)]
    mixed.append(good[-1])
    eng.tiff_set_decompress(DEVICE)
    try:
        out = eng.tiff_pdq_hash_batch([f[1] for f in mixed], want_pixel_hash=True)
        for name, data in refused:
            with pytest.raises(RphError) as e:
                eng.tiff_decode(data)
            assert e.value.status == tu.INVALID, name
    finally:
        eng.tiff_set_decompress(AUTO)
    for k, (name, _, px) in enumerate(mixed):
        if px is None:
            assert out["status"][k] == tu.INVALID, name
            assert not out["hash"][k].any() and not out["pixel_hash"][k].any() and out["valid"][k] == 0 and out["quality"][k] == 0, name
        else:
            assert out["status"][k] == 0, name
            _check_hashes(oracle, out, k, name, px)


def _corpus(group):
    """every valid stream of the group and every refused stream"""
    return list(group_files(group)) + [(n, d, None) for n, d in ls.refused_streams()]


@pytest.mark.parametrize("group", list(ls.GROUPS))
def test_modes_agree_on_valid_and_refused_streams(eng, group):
    corpus = _corpus(group)
    files = [d for _, d, _ in corpus]
    outs = []
    try:
        for mode in (HOST, DEVICE, AUTO):
            eng.tiff_set_decompress(mode)
            outs.append(eng.tiff_pdq_hash_batch(files, want_pixel_hash=True))
    finally:
        eng.tiff_set_decompress(AUTO)
    for k, (name, _, px) in enumerate(corpus):
        assert outs[0]["status"][k] == (0 if px is not None else tu.INVALID), name
    for o in outs[1:]:
        for key in KEYS:
            assert np.array_equal(o[key], outs[0][key]), key


@pytest.mark.parametrize("group", list(ls.GROUPS))
def test_each_file_alone_as_in_one_shuffled_call_of_all(eng, group):
    """valid and refused files interleaved in one call, then each alone: the LZW table and the segment in LDS of one stream (or call)
    do not reach the next"""
    corpus = _corpus(group)
    order = np.random.default_rng(3).permutation(len(corpus))
    files = [corpus[int(i)][1] for i in order]
    eng.tiff_set_decompress(DEVICE)
    try:
        big = eng.tiff_pdq_hash_batch(files, want_pixel_hash=True)
        assert (big["status"] != 0).sum() == len(ls.refused_streams())
        for k, data in enumerate(files):
            one = eng.tiff_pdq_hash_batch([data], want_pixel_hash=True)
            for key in KEYS:
                assert np.array_equal(big[key][k], one[key][0]), (corpus[int(order[k])][0], key)
    finally:
        eng.tiff_set_decompress(AUTO)
