"""Inflate on valid deflate streams that zlib's encoder never writes, host half (no GPU).  The streams come from the writer of
deflate_util: first the reference (zlib.decompress gives exactly expand(tokens) for every named and random stream and raises on every
refused one), then rph_png_decode_host and rph_tiff_decode_host through the two carriers: the expected bytes and status 0 for every
valid stream, the invalid-file status for every refused one.  The carrier files of the named and refused corpora also go through the
ASan + UBSan runs of test_png_cpu.py and test_tiff_cpu.py."""
import zlib

import numpy as np
import pytest

import deflate_util as du
import png_util as pu
import tiff_util as tu
from test_png_cpu import _host as png_host
from test_tiff_cpu import _host as tiff_host

def test_writer_codes_are_canonical_and_length_limited():
    assert du.canonical([2, 1, 3, 3]) == {0: (0b10, 2), 1: (0b0, 1), 2: (0b110, 3), 3: (0b111, 3)}  # RFC 1951 3.2.2's own shape
    rng = np.random.default_rng(1)
    for m in (2, 3, 5, 19, 30, 286):
        for depth in range(1, 16):
            lens = du.limited_code(list(rng.integers(1, 100, m)), depth, rng=rng)
            want = min(max(depth, (m - 1).bit_length()), m - 1, 15)
            assert max(lens) == want and du.kraft(lens) == 1 << 15 and all(lens), (m, depth)
    assert du.limited_code([0, 3, 0]) == [0, 1, 0] and du.limited_code([0, 0]) == [0, 0]
    assert du.cl_expand(du.cl_rle([0] * 150 + [7] * 9 + [0, 0, 3])) == [0] * 150 + [7] * 9 + [0, 0, 3]


def test_zlib_accepts_every_valid_stream_with_the_expected_bytes():
    streams = du.valid_streams()
    assert len(streams) >= 400
    for name, z, raw, cap in streams:
        assert z[:2] == b"\x78\x01", name  # CINFO 7: the window zlib checks distances against is the one inflate.h assumes
        assert zlib.decompress(z) == raw, name
        assert raw[0] == 0 and 2 <= cap <= len(raw) <= 200_000, name


def test_corpora_reach_the_cases_they_are_for():
    names = {n for n, _, _ in du.named_streams()}
    for dist in du.EDGE_DISTS:
        assert f"copy_dist{dist}" in names
    for want in ("lit_lengths_1_to_15", "deep_code_13", "all_length_and_distance_symbols", "length_258_as_284_plus_31_dynamic", "single_distance_code_symbol_4",
                 "no_distance_code", "repeat_16_crosses_into_distances", "repeat_18_crosses_into_distances", "all_19_code_length_symbols", "empty_stored_blocks",
                 "stored_2_after_huffman_blocks", "stored_65535", "400_tiny_blocks", "final_empty_fixed_block", "dist32768_at32768", "ring_start32767_dist1",
                 "flush_start4095", "cap_100_plus16", "all_ff_199999"):
        assert want in names, want
    assert {len(raw) % 64 for n, _, raw in du.named_streams() if n.startswith("final_flush_of_")} == set(range(64))
    assert sum(1 for n, _, raw in du.named_streams() if du.stream_cap(n) < len(raw)) >= 10
    again = du.random_streams(du.RANDOM_SEED, 5)
    assert [z for _, z, _ in again] == [z for n, z, _, _ in du.valid_streams() if n.startswith("random")][:5]  # seeded


def test_zlib_refuses_every_refused_stream():
    refused = du.refused_streams()
    assert len(refused) >= 30
    for name, z, cap in refused:
        try:
            zlib.decompress(z)
        except zlib.error:
            continue
        raise AssertionError(f"zlib accepts {name}")


@pytest.mark.parametrize("carrier,host", [("png", png_host), ("tiff", tiff_host)])
def test_host_decoder_on_every_valid_stream(carrier, host):
    n = 0
    for name, data, want in du.carrier_files(carrier):
        if want is None:
            continue
        rc, got = host(data)
        assert rc == 0, (name, rc)
        assert got.dtype == np.uint8 and got.shape == ((1, len(want)) if carrier == "png" else (len(want), 1)) and got.tobytes() == want, name
        n += 1
    assert n == len(du.valid_streams())


@pytest.mark.parametrize("carrier,host,invalid", [("png", png_host, pu.INVALID), ("tiff", tiff_host, tu.INVALID)])
def test_host_decoder_refuses_every_refused_stream(carrier, host, invalid):
    files = {name: data for name, data, want in du.carrier_files(carrier) if want is None}
    assert len(files) == len(du.refused_streams())
    for k, (name, z, cap) in enumerate(du.refused_streams()):
        assert host(files[name]) == (invalid, None), name
        # (the carrier itself is sound: the same geometry around a valid stream decodes)
        good = zlib.compress(bytes(cap))
        assert host(du.png_carrier(good, cap) if carrier == "png" else du.tiff_carrier(good, cap, k)[0])[0] == 0, name
