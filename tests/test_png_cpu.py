"""PNG path, host half (no GPU): the test helpers' reference decoder against Pillow, rph_png_decode_host against the reference decoder on
every layout and on the damaged corpus (each file's status included), the decompression-bomb bound, and the host parser + inflate under
ASan + UBSan (tools/fuzz_png_host.cpp)."""
import os
import subprocess

import numpy as np
import pytest

import deflate_util as du
import png_util as pu
import recon_grid as rg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host(data):
    from rupphash_amd import Engine, RphError

    try:
        return 0, Engine.png_decode_host(data)
    except RphError as e:
        return e.status, None


def test_reference_decoder_matches_pillow():
    Image = pytest.importorskip("PIL.Image")
    import io

    rng = np.random.default_rng(3)
    mode_of = {(0, 8): "L", (2, 8): "RGB", (6, 8): "RGBA", (4, 8): "LA", (0, 16): "I;16"}
    n = 0
    for (ct, d), mode in mode_of.items():
        for il in (False, True):
            data = pu.make_file(rng, 23, 17, ct, d, False, interlace=il)
            im = Image.open(io.BytesIO(data))
            if im.mode != mode:
                continue
            st, ref = pu.decode(data)
            assert st == 0
            got = np.asarray(im)
            assert np.array_equal(got.astype(np.int64), ref.astype(np.int64)), (ct, d, il)
            n += 1
    assert n >= 6


@pytest.mark.parametrize("name,data", pu.valid_corpus())
def test_host_decoder_equals_reference(name, data):
    st, ref = pu.decode(data)
    assert st == 0, name
    rc, got = _host(data)
    assert rc == 0, name
    assert got.dtype == ref.dtype and got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.array_equal(got, ref), name


def test_info_matches_layout():
    from rupphash_amd import Engine

    for name, data in pu.valid_corpus():
        _, ref = pu.decode(data)
        w, h, c, d = Engine.png_info(data)
        assert (h, w) == ref.shape[:2] and c == (1 if ref.ndim == 2 else ref.shape[2]) and d == ref.dtype.itemsize * 8, name


@pytest.mark.parametrize("name,data,status", pu.rule_corpus())
def test_each_rule_item(name, data, status):
    ref_st, ref = pu.decode(data)
    assert ref_st == status, (name, ref_st)
    rc, got = _host(data)
    assert rc == status, (name, rc)
    if status == 0:
        assert np.array_equal(got, ref)


def test_damaged_corpus_statuses_and_pixels():
    bad = 0
    for name, data in pu.damaged_corpus():
        ref_st, ref = pu.decode(data)
        rc, got = _host(data)
        assert rc == ref_st, (name, rc, ref_st)
        if rc == 0:
            assert np.array_equal(got, ref), name
        else:
            bad += 1
    assert bad > 50


def test_decompression_bomb_header_refused_before_allocation():
    from rupphash_amd import Engine, RphError

    bomb = [d for n, d, _ in pu.rule_corpus() if n == "bomb"][0]
    with pytest.raises(RphError) as e:
        Engine.png_info(bomb)
    assert e.value.status == pu.UNSUPPORTED
    with pytest.raises(RphError) as e:
        Engine.png_decode_host(bomb)
    assert e.value.status == pu.UNSUPPORTED


def test_host_parser_and_inflate_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """tools/fuzz_png_host.cpp: png_host.cpp + inflate.h built with ASan + UBSan on the CPU, fed the corpus and thousands of damaged
    variants of it; any report fails the run"""
    for k, (name, data) in enumerate(pu.valid_corpus(5) + [(n, d) for n, d, _ in pu.rule_corpus()]):
        (tmp_path / f"f{k:03d}.png").write_bytes(data)
    # deflate streams that zlib's encoder never writes (deflate_util's named and refused corpora, in this format's carrier)
    for k, (name, data, _) in enumerate(f for f in du.carrier_files("png") if not f[0].startswith("random")):
        (tmp_path / f"g{k:03d}.png").write_bytes(data)
    # the reconstruction grids (recon_grid.py): every file
    for k, (name, data) in enumerate(x for files in rg.png_grid().values() for x in files):
        (tmp_path / f"r{k:04d}.png").write_bytes(data)
    exe = str(tmp_path / "fuzz_png_host")
    csrc = os.path.join(ROOT, "rupphash_amd", "csrc")
    try:
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", csrc,
                               "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "fuzz_png_host.cpp"), os.path.join(csrc, "png_host.cpp"),
                               "-o", exe])
    except (subprocess.CalledProcessError, FileNotFoundError):
        pytest.skip("no sanitizer runtime for g++ here")
    r = subprocess.run([exe, str(tmp_path), "40"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "no sanitizer report" in r.stdout, r.stdout + r.stderr[-3000:]
