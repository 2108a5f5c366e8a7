"""BLAKE3 identity hashes, host side: the test helper (tests/blake3_util.py) against the published test vectors and its two tree
builders against each other, the library's host-scalar rph_blake3_host against the helper, the pixel-hash byte stream, and the
duplicate mask of analyze_group.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import blake3_util as b3  # noqa: E402

KEY = b"whats the Elvish word for friend"  # the key of the published keyed_hash vectors

LENGTHS = sorted({0, 1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 16384, 31744, 102400}
                 | {k * 1024 + d for k in range(1, 10) for d in (-1, 1)})


def test_helper_reproduces_published_vectors():
    assert b3.blake3(b"").hex() == "af1349b9f5f9a1a6a0404dea36dcc9499bcb25c9adc112b7cc9a93cae41f3262"
    assert b3.blake3(b"abc").hex() == "6437b3ac38465133ffb63b75273a8db548c558465d79db03fd359c6cd5bd9d85"
    assert b3.blake3(b3.test_input(1024)).hex().startswith("42214739f095a406f3fc83deb889744a")
    assert b3.blake3(b3.test_input(1025)).hex().startswith("d00278ae47eb27b34faecf67b4fe263f")
    assert b3.blake3(b"", KEY).hex() == "92b2b75604ed3c761f9d6f62392c8a9227ad0ea3f09573e783f1498a4ed60d26"


@pytest.mark.parametrize("key", [None, KEY], ids=["hash", "keyed"])
def test_fold_and_stack_trees_agree(key):
    for n in LENGTHS:
        data = b3.test_input(n)
        assert b3.blake3(data, key) == b3.blake3_stack(data, key), n


def test_many_messages_at_once_agree_with_one_at_a_time():
    rng = np.random.default_rng(5)
    datas = [b3.test_input(n) for n in LENGTHS] + [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (0, 5, 1024, 3000, 3072, 70000)]
    assert b3.blake3_many(datas) == [b3.blake3(d) for d in datas]
    assert b3.blake3_many([]) == [] and b3.blake3_many([b"abc"]) == [b3.blake3(b"abc")]
    for key in (KEY, bytes(range(32))):
        assert b3.blake3_many(datas, key) == [b3.blake3(d, key) for d in datas]
        assert b3.blake3_many([], key) == [] and b3.blake3_many([b""], key) == [b3.blake3(b"", key)]
    assert b3.blake3_many(datas, key=None) == b3.blake3_many(datas) != b3.blake3_many(datas, KEY)


@pytest.mark.parametrize("key", [None, KEY, bytes(range(32))], ids=["hash", "keyed", "key2"])
def test_host_scalar_matches_helper(key):
    from rupphash_amd import Engine

    rng = np.random.default_rng(3)
    for n in LENGTHS:
        data = b3.test_input(n)
        assert Engine.blake3_host(data, key) == b3.blake3(data, key), n
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert Engine.blake3_host(data, key) == b3.blake3(data, key), n


def test_rgba16_byte_stream():
    assert b3.rgba16_bytes(np.array([[[1, 2, 3]]], np.uint8)) == bytes([1, 1, 2, 2, 3, 3, 0xFF, 0xFF])
    assert b3.rgba16_bytes(np.array([[7]], np.uint8)) == bytes([7, 7, 7, 7, 7, 7, 0xFF, 0xFF])
    assert b3.rgba16_bytes(np.array([[[1, 2, 3, 4]]], np.uint8)) == bytes([1, 1, 2, 2, 3, 3, 4, 4])
    assert b3.rgba16_bytes(np.array([[[255, 0, 128]]], np.uint8)) == bytes([255, 255, 0, 0, 128, 128, 255, 255])


def test_identical_duplicates_mask():
    from rupphash_amd import scanner

    a, b, c, d = (bytes([i]) * 32 for i in range(4))
    p, q = bytes([9]) * 32, bytes([8]) * 32
    # files 0/1 bit-identical; 2/3 differ in bytes but share pixels; 4 unique; 5 has no pixel hash
    content = [a, a, b, c, d, bytes([5]) * 32]
    pixels = [p, p, q, q, bytes([7]) * 32, None]
    assert scanner.identical_duplicates(content, pixels) == [True, True, True, True, False, False]
    assert scanner.identical_duplicates(content, None) == [True, True, False, False, False, False]
    assert scanner.identical_duplicates([a, b], [None, None]) == [False, False]
    assert scanner.identical_duplicates(np.array([list(a), list(b), list(a)], np.uint8)) == [True, False, True]
