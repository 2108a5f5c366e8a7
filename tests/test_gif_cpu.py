"""The GIF decoder on the host (rph_gif_decode_host, rph_gif_info; no GPU): files Pillow writes against Pillow's own decode of them, files of
tests/gif_streams.py against its numpy restatement of the rule (include/rupphash.h, GIF section), one damaged file per line of the
rule with its exact status, and the host decoder as a stand-alone program under ASan + UBSan over the corpora, the files of the
reconstruction grid and damaged variants of all of them."""
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

import gif_streams as gs
import recon_grid as rg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pillow_rgba(data):
    from PIL import Image

    im = Image.open(io.BytesIO(data))
    im.seek(0)
    return np.array(im.convert("RGBA"))


def _decode(data):
    from rupphash_amd import Engine

    return Engine.gif_decode_host(data)


def _status(fn, data):
    from rupphash_amd import RphError

    try:
        fn(data)
    except RphError as e:
        return e.status
    return 0


def test_pillow_corpus_is_what_it_says():
    """palettes of 2, 4, 16, 256 colours give tables of 4, 4, 16, 256 entries (Pillow's writer sends minimum code size 8 whatever the
    palette: sizes 2 .. 8 come from the helper's writer and are read by Pillow in the test below); the noise image sends Clears; the
    interlaced files are interlaced; the animation has two frames"""
    from PIL import Image

    files = dict(gs.pillow_files())
    assert len(files) == 19

    def first_descriptor(d):
        pos = 13 + (3 * (2 << (d[10] & 7)) if d[10] & 0x80 else 0)
        while d[pos] == 0x21:
            pos += 2
            while d[pos]:
                pos += 1 + d[pos]
            pos += 1
        assert d[pos] == 0x2C
        flags = d[pos + 9]
        return flags, d[pos + 10 + (3 * (2 << (flags & 7)) if flags & 0x80 else 0)]

    for n, entries in ((2, 4), (4, 4), (16, 16), (256, 256)):
        d = files[f"colours_{n}"]
        assert 2 << (d[10] & 7) == entries and first_descriptor(d)[1] == 8
    for h in (16, 17, 18, 19, 20, 21, 22, 23, 67):
        assert first_descriptor(files[f"interlaced_{h}"])[0] & 0x40
    assert len(files["noise_300x200"]) > 4096 * 12 // 8  # more codes than one table holds
    assert Image.open(io.BytesIO(files["animation_2_frames"])).n_frames == 2
    assert Image.open(io.BytesIO(files["transparent"])).info["transparency"] == 3


@pytest.mark.parametrize("name,data", gs.pillow_files(), ids=[f[0] for f in gs.pillow_files()])
def test_files_pillow_writes_decode_as_pillow_decodes_them(name, data):
    from rupphash_amd import Engine

    ref = _pillow_rgba(data)
    assert Engine.gif_info(data) == (ref.shape[1], ref.shape[0], 4, 8)
    got = _decode(data)
    assert got.dtype == np.uint8 and got.shape == ref.shape and np.array_equal(got, ref)
    if name == "transparent":
        assert (got[:, :, 3] == 0).any() and (got[:, :, 3] == 255).any()


@pytest.mark.parametrize("name,data,px", gs.interlaced_files(), ids=[f[0] for f in gs.interlaced_files()])
def test_interlaced_heights_1_to_9_decode_as_pillow_decodes_them(name, data, px):
    """Pillow's writer does not interlace an image with a side below 16 px, so these heights come from the helper's writer; Pillow reads
    them, and its pixels, the restatement's and the decoder's are the same"""
    ref = _pillow_rgba(data)
    assert np.array_equal(ref, px)
    assert np.array_equal(_decode(data), ref)


_CODE_SIZES = [f for f in gs.valid_files() if f[0].startswith("min_code_size_")]


@pytest.mark.parametrize("name,data,px", _CODE_SIZES, ids=[f[0] for f in _CODE_SIZES])
def test_minimum_code_sizes_2_to_8_decode_as_pillow_decodes_them(name, data, px):
    """palettes of 4 .. 256 colours at their own code size (with a Clear whenever the table is full, and with none at all)"""
    assert len(_CODE_SIZES) == 14
    ref = _pillow_rgba(data)
    assert np.array_equal(ref, px) and np.array_equal(_decode(data), ref)


@pytest.mark.parametrize("name,data,px", gs.valid_files(), ids=[f[0] for f in gs.valid_files()])
def test_files_of_the_writer_decode_to_the_restatement(name, data, px):
    from rupphash_amd import Engine

    assert Engine.gif_info(data) == (px.shape[1], px.shape[0], 4, 8)
    got = _decode(data)
    assert got.shape == px.shape and np.array_equal(got, px), name


def test_corpus_covers_what_the_rule_names():
    names = [f[0] for f in gs.valid_files()]
    assert len(set(names)) == len(names) >= 60
    # the deferred-clear streams hold no Clear and go on long after the table is full
    rng_noise = [f for f in gs.valid_files() if f[0] == "deferred_clear_8"][0]
    assert rng_noise[2].shape == (96, 96, 4)
    # the flat chain ends with plain copies of 63 .. 129 bytes
    flat = [f for f in gs.valid_files() if f[0] == "flat_kwkwk_chain"][0][2]
    assert (flat[:, :, 0] == flat[0, 0, 0]).all()
    # the Python decoder of the helper refuses what the damaged corpus says the stream rule refuses
    assert gs.lzw_decode(gs.pack_codes([4, 0, 7, 0, 0, 0, 0, 0, 0], 2), 2, 8) is None
    assert gs.lzw_decode(gs.pack_codes([4, 0, 1, 2, 5], 2), 2, 4) is None
    assert gs.lzw_decode(gs.pack_codes([4, 0, 1, 2, 5], 2), 2, 3).tolist() == [0, 1, 2]


@pytest.mark.parametrize("name,data,status", gs.damaged_files(), ids=[f[0] for f in gs.damaged_files()])
def test_damaged_files_have_their_exact_status(name, data, status):
    from rupphash_amd import Engine

    assert _status(_decode, data) == status, name
    # rph_gif_info applies the container's part of the rule; the stream's own refusals show only in the decode
    stream_rule = ("code_above", "first_code", "kwkwk_as_first", "out_of_bits", "eoi_")
    assert _status(Engine.gif_info, data) == (0 if name.startswith(stream_rule) else status), name


def test_expansion_bound_is_the_stated_one():
    """the largest frame a stream of n bytes may claim: (4095 - (1 << m)) * floor(8 n / (m + 1)), exactly"""
    from rupphash_amd import Engine

    for n, m in ((40, 2), (7, 2), (9, 8)):
        bound = gs.expansion_bound(m, n)
        w = 1000
        h_ok = bound // w
        pal_m = gs.colour_palette(1 << m, 1)
        ok = gs.write_gif((8, 8), (0, 0), (w, h_ok), m, b"\xff" * n, gct=pal_m)
        over = gs.write_gif((8, 8), (0, 0), (w, h_ok + 1), m, b"\xff" * n, gct=pal_m)
        assert _status(Engine.gif_info, ok) == 0 and _status(Engine.gif_info, over) == gs.UNSUPPORTED, (n, m)


def test_load_gif_takes_only_gif_names():
    from rupphash_amd import scanner

    with pytest.raises(ValueError):
        scanner.load_gif("a.png", b"")
    with pytest.raises(ValueError):
        scanner.load_image_fast("a.gif", b"")


def test_capacity_and_null_arguments():
    import ctypes as C

    from rupphash_amd import _lib

    L = _lib.load()
    data = gs.valid_files()[0][1]
    buf = np.zeros(8, np.uint8)
    assert L.rph_gif_decode_host(data, len(data), buf.ctypes.data_as(C.c_void_p), 8) == _lib.RPH_ERR_CAPACITY
    assert L.rph_gif_decode_host(None, 0, buf.ctypes.data_as(C.c_void_p), 8) == _lib.RPH_ERR_INVALID_ARG
    assert L.rph_gif_info(data, len(data), None, None, None, None) == 0


def test_host_decoder_is_clean_under_asan_and_ubsan(tmp_path):
    """tools/fuzz_gif_host.cpp, a program of its own built from gif_host.cpp with -fsanitize=address,undefined: the valid, Pillow and
    damaged corpora and every file of the reconstruction grid (recon_grid.py), each intact and with 10 random damages"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = tmp_path / "fuzz_gif_host"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "rupphash_amd", "csrc"),
                           os.path.join(ROOT, "tools", "fuzz_gif_host.cpp"), os.path.join(ROOT, "rupphash_amd", "csrc", "gif_host.cpp"), "-o", str(exe)])
    corpus = tmp_path / "corpus"
    assert gs.dump(str(corpus)) >= 120
    grid = [x for files in rg.gif_grid().values() for x in files]
    for k, (name, data) in enumerate(grid):
        (corpus / f"grid{k:04d}.gif").write_bytes(data)
    r = subprocess.run([str(exe), str(corpus), "10"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "no sanitizer report" in r.stdout and int(r.stdout.split()[0]) >= 120 + len(grid)
