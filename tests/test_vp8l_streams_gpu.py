"""The VP8L entropy decoder on the device (-m gpu) on the token-level streams of vp8l_streams.py, with the entropy stage forced to the
device (AUTO is the host for WebP): decoded pixels against the expansion of the tokens, batch statuses, pixel hashes against a BLAKE3
of the expected pixels, PDQ outputs against the CPU oracle on them, refused streams refused with zero outputs and their neighbours
untouched, the same arrays in the HOST, DEVICE and AUTO modes, and every file alone as in one shuffled call of all of them."""
import functools

import numpy as np
import pytest

import blake3_util as b3
import vp8l_streams as vs
import webp_util as wu

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
    return [f for f in vs.valid_streams() if f[0].startswith(vs.GROUPS[group])]


def _check_hashes(oracle, out, k, name, px):
    img = vs.expected_image(px)
    assert out["pixel_hash"][k].tobytes() == b3.blake3(wu.to_rgba16(img)), name
    if px.shape[0] < 5 or px.shape[1] < 5:
        assert out["valid"][k] == 0 and not out["hash"][k].any() and out["quality"][k] == 0, name
        return
    rc, coeffs, q = oracle.pdq_features(np.ascontiguousarray(img[:, :, :3]))
    assert rc == 0 and out["valid"][k] == 1, name
    assert np.array_equal(out["hash"][k], oracle.to_hash(coeffs)) and out["quality"][k] == np.float32(q), name


def test_groups_leave_no_stream_out():
    names = [f[0] for f in vs.valid_streams()]
    assert sorted(f[0] for g in vs.GROUPS for f in group_files(g)) == sorted(names) and len(names) >= 250


@pytest.mark.parametrize("group", list(vs.GROUPS))
def test_device_decode_and_batch_equal_the_expansion(eng, oracle, group):
    files = group_files(group)
    assert files
    eng.webp_set_entropy(DEVICE)
    try:
        for name, data, px in files:
            got = eng.webp_decode(data)
            want = vs.expected_image(px)
            assert got.dtype == np.uint8 and got.shape == want.shape and got.tobytes() == want.tobytes(), name
        out = eng.webp_pdq_hash_batch([d for _, d, _ in files], want_pixel_hash=True)
    finally:
        eng.webp_set_entropy(AUTO)
    assert not out["status"].any(), [files[k][0] for k in np.nonzero(out["status"])[0]]
    for k, (name, _, px) in enumerate(files):
        _check_hashes(oracle, out, k, name, px)


def test_device_refuses_every_refused_stream_and_leaves_its_neighbours(eng, oracle):
    from rupphash_amd import RphError

    refused = vs.refused_streams()
    good = [f for f in vs.valid_streams() if f[0].startswith(("edge_", "endbit_", "zero_tail"))]
    mixed = []  # a valid stream on either side of every refused one
    for k, (name, data) in enumerate(refused):
        mixed += [good[k % len(good)], (name, data, None)]
    mixed.append(good[-1])
    eng.webp_set_entropy(DEVICE)
    try:
        out = eng.webp_pdq_hash_batch([f[1] for f in mixed], want_pixel_hash=True)
        for name, data in refused:
            with pytest.raises(RphError) as e:
                eng.webp_decode(data)
            assert e.value.status == wu.INVALID, name
    finally:
        eng.webp_set_entropy(AUTO)
    for k, (name, _, px) in enumerate(mixed):
        if px is None:
            assert out["status"][k] == wu.INVALID, name
            assert not out["hash"][k].any() and not out["pixel_hash"][k].any() and out["valid"][k] == 0 and out["quality"][k] == 0, name
        else:
            assert out["status"][k] == 0, name
            _check_hashes(oracle, out, k, name, px)


def _corpus(group):
    """every valid stream of the group and every refused stream"""
    return list(group_files(group)) + [(n, d, None) for n, d in vs.refused_streams()]


@pytest.mark.parametrize("group", list(vs.GROUPS))
def test_modes_agree_on_valid_and_refused_streams(eng, group):
    corpus = _corpus(group)
    files = [d for _, d, _ in corpus]
    outs = []
    try:
        for mode in (HOST, DEVICE, AUTO):
            eng.webp_set_entropy(mode)
            outs.append(eng.webp_pdq_hash_batch(files, want_pixel_hash=True))
    finally:
        eng.webp_set_entropy(AUTO)
    for k, (name, _, px) in enumerate(corpus):
        assert outs[0]["status"][k] == (0 if px is not None else wu.INVALID), name
    for o in outs[1:]:
        for key in KEYS:
            assert np.array_equal(o[key], outs[0][key]), key


@pytest.mark.parametrize("group", list(vs.GROUPS))
def test_each_file_alone_as_in_one_shuffled_call_of_all(eng, group):
    """valid and refused files interleaved in one call, then each alone: the colour cache and the table-slot tags in LDS, the pending
    register and `flushed` of one stream (or call) do not reach the next"""
    corpus = _corpus(group)
    order = np.random.default_rng(3).permutation(len(corpus))
    files = [corpus[int(i)][1] for i in order]
    eng.webp_set_entropy(DEVICE)
    try:
        big = eng.webp_pdq_hash_batch(files, want_pixel_hash=True)
        assert (big["status"] != 0).sum() == len(vs.refused_streams())
        for k, data in enumerate(files):
            one = eng.webp_pdq_hash_batch([data], want_pixel_hash=True)
            for key in KEYS:
                assert np.array_equal(big[key][k], one[key][0]), (corpus[int(order[k])][0], key)
    finally:
        eng.webp_set_entropy(AUTO)
