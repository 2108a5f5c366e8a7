"""The BMP decoder on the host (rph_bmp_decode_host, rph_bmp_info; no GPU): files of tests/bmp_streams.py against its numpy statement of
the rule (include/rupphash.h, BMP section), the fixed Pillow list against Pillow's own decode byte for byte (16-bit files within 1 per
sample: Pillow floors where the rule rounds), one damaged file per line of the rule with its exact status, and the host parser as a
stand-alone program under ASan + UBSan over the corpora, every prefix and single-byte mutations of three small files."""
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

import bmp_streams as bs
import recon_grid as rg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pillow(data):
    """Pillow's pixels: RGB and RGBA as they are, every other mode through convert("RGB"); a file Pillow cannot read fails the test"""
    from PIL import Image

    im = Image.open(io.BytesIO(data))
    im.load()
    return np.array(im if im.mode in ("RGB", "RGBA") else im.convert("RGB"))


def _decode(data):
    from rupphash_amd import Engine

    return Engine.bmp_decode_host(data)


def _status(fn, data):
    from rupphash_amd import RphError

    try:
        fn(data)
    except RphError as e:
        return e.status
    return 0


@pytest.mark.parametrize("name,data,px", bs.valid_files(), ids=[f[0] for f in bs.valid_files()])
def test_files_of_the_writer_decode_to_the_rule(name, data, px):
    from rupphash_amd import Engine

    assert Engine.bmp_info(data) == (px.shape[1], px.shape[0], px.shape[2], 8)
    got = _decode(data)
    assert got.dtype == np.uint8 and got.shape == px.shape and np.array_equal(got, px), name


def test_corpus_covers_what_the_section_names():
    names = [f[0] for f in bs.valid_files()]
    assert len(set(names)) == len(names) >= 140
    for v in bs.VARIANTS:
        assert any(n.startswith(v + "_13x7") for n in names), v
    for hdr in (12, 40, 52, 56, 108, 124):
        assert f"rgb24_header_{hdr}" in names and f"pal8_header_{hdr}" in names
    chans = {n: px.shape[2] for n, _, px in bs.valid_files()}
    assert chans["bf8888a_header_56_compression_3"] == 4 and chans["bf8888a_header_52_compression_3"] == 3 and chans["bf8888a_header_40_compression_3"] == 3
    assert chans["bf4444a_header_40_compression_6"] == 4 and chans["rgb32_header_124"] == 3 and chans["masks_odd_3_10_2a"] == 4
    # the rounding the rule states, where Pillow floors: 5-bit 16 -> 132, 6-bit 32 -> 130
    v = np.array([[16 << 11 | 32 << 5]], np.uint64)
    assert bs.rule_fields(v, bs.MASKS["565"][1])[0, 0].tolist() == [132, 130, 0]
    # skipped RLE pixels are black although palette entry 0 is white
    px = [f for f in bs.valid_files() if f[0] == "rle8_skipped_pixels_are_not_entry_0"][0][2]
    assert (px == 0).any() and (px == 255).any()


@pytest.mark.parametrize("name,data", bs.pillow_exact_files(), ids=[f[0] for f in bs.pillow_exact_files()])
def test_pillow_list_decodes_as_pillow_decodes_it(name, data):
    assert len(bs.pillow_exact_files()) == 5 + 12 + 4
    ref = _pillow(data)
    got = _decode(data)
    assert got.shape == ref.shape and np.array_equal(got, ref), name


def test_pillow_written_files_are_what_they_say():
    import struct

    depth = {n: struct.unpack_from("<H", d, 28)[0] for n, d in bs.pillow_written()}
    assert depth == {"pillow_1": 1, "pillow_L": 8, "pillow_P": 8, "pillow_RGB": 24, "pillow_RGBA": 32}
    # Pillow writes RGBA as 32-bit BI_RGB: the fourth byte is ignored, by the rule and by Pillow reading its own file back
    assert _decode(dict(bs.pillow_written())["pillow_RGBA"]).shape[2] == 3 and _pillow(dict(bs.pillow_written())["pillow_RGBA"]).shape[2] == 3


@pytest.mark.parametrize("name,data", bs.pillow_16_bit_files(), ids=[f"{f[0]}_{k & 1}" for k, f in enumerate(bs.pillow_16_bit_files())])
def test_16_bit_files_are_within_1_of_pillow(name, data):
    ref = _pillow(data).astype(np.int32)
    got = _decode(data).astype(np.int32)
    assert got.shape == ref.shape and np.abs(got - ref).max() <= 1, name
    assert (got >= ref).all()  # the rule rounds to nearest, Pillow floors


def test_two_bit_files_are_refused_by_pillow_and_held_to_the_rule():
    from PIL import Image

    data, px = bs.make("pal2", 17, 5, seed=3)
    with pytest.raises(Exception):
        Image.open(io.BytesIO(data)).load()
    assert np.array_equal(_decode(data), px)


@pytest.mark.parametrize("name,data,status", bs.damaged_files(), ids=[f[0] for f in bs.damaged_files()])
def test_damaged_files_have_their_exact_status(name, data, status):
    from rupphash_amd import Engine

    assert _status(_decode, data) == status, name
    assert _status(Engine.bmp_info, data) == status, name  # rph_bmp_info runs every check, the RLE stream's among them


def test_damaged_corpus_covers_the_rule():
    st = [s for _, _, s in bs.damaged_files()]
    assert st.count(bs.INVALID) >= 50 and st.count(bs.UNSUPPORTED) >= 15


def test_load_bmp_takes_only_bmp_names():
    from rupphash_amd import scanner

    with pytest.raises(ValueError):
        scanner.load_bmp("a.png", b"")
    with pytest.raises(ValueError):
        scanner.load_bmp("a.dib", b"")
    with pytest.raises(ValueError):
        scanner.load_image_fast("a.bmp", b"")


def test_capacity_and_null_arguments():
    import ctypes as C

    from rupphash_amd import _lib

    L = _lib.load()
    data = bs.valid_files()[0][1]
    buf = np.zeros(8, np.uint8)
    assert L.rph_bmp_decode_host(data, len(data), buf.ctypes.data_as(C.c_void_p), 8) == _lib.RPH_ERR_CAPACITY
    assert L.rph_bmp_decode_host(None, 0, buf.ctypes.data_as(C.c_void_p), 8) == _lib.RPH_ERR_INVALID_ARG
    assert L.rph_bmp_info(data, len(data), None, None, None, None) == 0
    assert not hasattr(L, "rph_bmp_set_decompress")  # no mode: RLE streams are the host's


def test_host_parser_is_clean_under_asan_and_ubsan(tmp_path):
    """tools/fuzz_bmp_host.cpp, a program of its own built from bmp_host.cpp with -fsanitize=address,undefined: the valid, Pillow and
    damaged corpora and the files of the reconstruction grid, every prefix and 300 single-byte mutations of three small files"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = tmp_path / "fuzz_bmp_host"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "rupphash_amd", "csrc"),
                           os.path.join(ROOT, "tools", "fuzz_bmp_host.cpp"), os.path.join(ROOT, "rupphash_amd", "csrc", "bmp_host.cpp"), "-o", str(exe)])
    corpus = tmp_path / "corpus"
    assert bs.dump(str(corpus)) >= 250
    # the reconstruction grid (recon_grid.py): every file
    for k, (name, data) in enumerate(x for files in rg.bmp_grid().values() for x in files):
        (corpus / f"grid{k:04d}.bmp").write_bytes(data)
    small =["rle8_delta_and_skipped_pixels_palette_of_9", "bf4444a_header_40_compression_6", "pal4_header_12"]
    r = subprocess.run([str(exe), str(corpus), "300"] + small, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "no sanitizer report" in r.stdout
