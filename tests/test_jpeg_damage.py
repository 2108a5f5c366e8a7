"""Damaged JPEG streams (tests/jpeg_util.damaged_corpus): the host entropy decoder and the CPU oracle follow the same written rule
(include/rupphash.h, rph_jpeg_set_entropy) -- the same refusals, the same coefficients -- and each targeted violation gets the status the
rule gives it.  The device paths are held to the same results in test_jpeg_damage_gpu.py."""
import numpy as np
import pytest

import jpeg_util as ju
import oracle

PIL = pytest.importorskip("PIL")


def _host(data):
    from rupphash_amd import _lib
    from rupphash_amd.engine import Engine

    try:
        return Engine.jpeg_coefficients(data)
    except _lib.RphError:
        return None


def _oracle(data):
    try:
        return oracle.jpeg_coefficients(data)
    except ValueError:
        return None


@pytest.fixture(scope="module")
def corpus():
    return ju.damaged_corpus()


def test_corpus_is_deterministic_and_covers_every_rule(corpus):
    again = ju.damaged_corpus()
    assert [(n, d) for n, d, _ in corpus] == [(n, d) for n, d, _ in again]
    names = " ".join(n for n, _, _ in corpus)
    for kind in list(ju.BASELINE_FAULTS) + list(ju.PROGRESSIVE_FAULTS) + list(ju.RESTART_FAULTS) + ["truncated", "marker_d9", "fill", "random"]:
        assert kind in names, kind
    assert sum(w == "refused" for _, _, w in corpus) >= 40 and sum(w == "decoded" for _, _, w in corpus) >= 40


def test_host_decoder_and_oracle_agree_on_damaged_streams(corpus):
    bad = []
    for name, data, want in corpus:
        h, o = _host(data), _oracle(data)
        if (h is None) != (o is None):
            bad.append((name, "host refuses" if h is None else "oracle refuses"))
            continue
        if h is not None and not (np.array_equal(h[0], o[0]) and np.array_equal(h[1], o[1]) and np.array_equal(h[2], o[2])):
            bad.append((name, "coefficients differ"))
        if want is not None and (h is None) != (want == "refused"):
            bad.append((name, f"expected {want}"))
    assert not bad, bad


def test_oracle_pixels_follow_its_coefficients(corpus):
    """the oracle's decode (both flavours) refuses exactly what its coefficient pass refuses.  (The library has no CPU pixel path: the
    host decoder's pixels, through their hashes, are compared with the oracle's in test_jpeg_damage_gpu.py,
    test_host_mode_is_oracle_decode_then_oracle_hash.)"""
    for name, data, _ in corpus[::3]:
        ok = _oracle(data) is not None
        for flavour in (oracle.JPEG_ZUNE, oracle.JPEG_LIBJPEG):
            try:
                oracle.jpeg_decode(data, flavour)
                decoded = True
            except ValueError:
                decoded = False
            assert decoded == ok, (name, flavour)


@pytest.mark.parametrize("kind", sorted(ju.BASELINE_FAULTS))
def test_baseline_fault_status(kind):
    """one rule at a time, also where the block is the first after a restart marker"""
    a = np.array(ju.make_image(24, 16, seed=5))
    for fault in [(kind, 0, 15), (kind, 3, 12)]:
        data = ju.encode_baseline(a, ((1, 1), (1, 1), (1, 1)), restart_interval=3, fault=fault)
        h, o = _host(data), _oracle(data)
        assert (h is None) == (o is None) == (ju.BASELINE_FAULTS[kind] == "refused"), fault


def test_zrl_that_ends_the_block_is_decoded_like_zeros():
    """a ZRL ending exactly at coefficient 63 is 16 zeros: the block equals one coded with EOB instead"""
    a = np.array(ju.make_image(16, 8, seed=9))
    data = ju.encode_baseline(a, ((1, 1), (1, 1), (1, 1)), fault=("zrl_to_64", 1))
    h, o = _host(data), _oracle(data)
    assert h is not None and np.array_equal(h[2], o[2])
    blk = h[2][1][ju.ZIGZAG]
    assert blk[47] == 1 and not blk[1:47].any() and not blk[48:].any()
