"""TIFF path, host half (no GPU): the test helpers' reference decoder against Pillow (libtiff) on files the helper writes and the host
decoder against Pillow on files Pillow writes, rph_tiff_decode_host against the reference decoder on every layout, on each item of the
rule and on the damaged corpus (each file's status included), the decompression-bomb bound, and the host parser + decompressors under
ASan + UBSan (tools/fuzz_tiff_host.cpp)."""
import io
import os
import subprocess

import numpy as np
import pytest

import deflate_util as du
import recon_grid as rg
import tiff_util as tu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (Pillow mode, samples, bits); Pillow only ever sees well-formed files from this fixed list, and no sub-8-bit + predictor file
PIL_MODES = [("L", 1, 8), ("LA", 2, 8), ("RGB", 3, 8), ("RGBA", 4, 8), ("I;16", 1, 16)]
PIL_COMPRESSIONS = [("raw", 1, 1), ("packbits", 32773, 1), ("tiff_lzw", 5, 1), ("tiff_adobe_deflate", 8, 1), ("tiff_lzw", 5, 2), ("tiff_adobe_deflate", 8, 2)]


def _host(data):
    from rupphash_amd import Engine, RphError

    try:
        return 0, Engine.tiff_decode_host(data)
    except RphError as e:
        return e.status, None


def _pil_array(im, mode):
    a = np.asarray(im)
    return a.astype(np.uint16) if mode == "I;16" else a


def test_reference_and_host_decoders_match_pillow():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(3)
    compared = 0
    for mode, spp, bps in PIL_MODES:
        for name, comp, pred in PIL_COMPRESSIONS:
            s = tu.random_samples(rng, 37, 53, spp, bps)
            # files the helper writes, read by libtiff
            data = tu.encode(s, bps=bps, compression=comp, predictor=pred, rows_per_strip=8, bo="<>"[compared & 1])
            st, ref = tu.decode(data)
            assert st == 0
            try:
                im = Image.open(io.BytesIO(data))
                im.load()
            except Exception:  # (Pillow refuses the combination)
                continue
            assert im.mode in (mode, mode + "B"), (mode, name, pred, im.mode)  # (a big-endian 16-bit file opens as I;16B)
            assert np.array_equal(_pil_array(im, mode), ref), (mode, name, pred)
            # files libtiff writes (an independent encoder), read by the host decoder
            arr = s[:, :, 0] if spp == 1 else s
            src = Image.fromarray(arr.astype(np.uint16 if bps == 16 else np.uint8), mode if bps == 8 else None)
            buf = io.BytesIO()
            kw = {"tiffinfo": {317: 2}} if pred == 2 else {}
            src.save(buf, format="TIFF", compression=name, **kw)
            rc, got = _host(buf.getvalue())
            assert rc == 0, (mode, name, pred, rc)
            back = Image.open(io.BytesIO(buf.getvalue()))
            assert np.array_equal(got, _pil_array(back, mode)) and np.array_equal(got, arr), (mode, name, pred)
            st2, ref2 = tu.decode(buf.getvalue())
            assert st2 == 0 and np.array_equal(ref2, got)
            compared += 1
    assert compared >= 25


@pytest.mark.parametrize("name,data", tu.valid_corpus())
def test_host_decoder_equals_reference(name, data):
    st, ref = tu.decode(data)
    assert st == 0, name
    rc, got = _host(data)
    assert rc == 0, name
    assert got.dtype == ref.dtype and got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.array_equal(got, ref), name


def test_info_matches_layout():
    from rupphash_amd import Engine

    for name, data in tu.valid_corpus():
        _, ref = tu.decode(data)
        w, h, c, d = Engine.tiff_info(data)
        assert (h, w) == ref.shape[:2] and c == (1 if ref.ndim == 2 else ref.shape[2]) and d == ref.dtype.itemsize * 8, name
        assert tu.info(data) == (0, (w, h, c, d))


@pytest.mark.parametrize("name,data,status", tu.rule_corpus())
def test_each_rule_item(name, data, status):
    ref_st, ref = tu.decode(data)
    assert ref_st == status, (name, ref_st)
    rc, got = _host(data)
    assert rc == status, (name, rc)
    if status == 0:
        assert np.array_equal(got, ref)


def test_damaged_corpus_statuses_and_pixels():
    bad = 0
    for name, data in tu.damaged_corpus():
        ref_st, ref = tu.decode(data)
        rc, got = _host(data)
        assert rc == ref_st, (name, rc, ref_st)
        if rc == 0:
            assert np.array_equal(got, ref), name
        else:
            bad += 1
    assert bad > 50


def test_decompression_bomb_header_refused_before_allocation():
    from rupphash_amd import Engine, RphError

    for which in ("bomb", "too_many_bytes", "lzw_implausible"):
        bomb = [d for n, d, _ in tu.rule_corpus() if n == which][0]
        with pytest.raises(RphError) as e:
            Engine.tiff_info(bomb)
        assert e.value.status == tu.UNSUPPORTED
        with pytest.raises(RphError) as e:
            Engine.tiff_decode_host(bomb)
        assert e.value.status == tu.UNSUPPORTED


def test_lzw_expansion_bound_is_reachable_but_not_exceeded():
    """the longest string of a 12-bit table is 3839 bytes (tiff_lzw.h): a run reaches entry lengths close to it, and no stream of the
    writer expands by more than 3839 bytes per 9 bits"""
    run = bytes(3_000_000)
    z = tu.lzw_encode(run)
    assert len(run) <= tu.max_expansion(5, len(z))
    assert tu.lzw_decode(z, len(run)) == run
    # a run makes strings of 1, 2, 3, ... bytes, about half the longest on average, at up to 12 bits each: the writer comes within a
    # factor of 8 of the 3839 * 8 / 9 bytes per byte the bound allows
    assert len(run) / len(z) > 3839 * 8 / 9 / 8


def test_host_parser_and_decompressors_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """tools/fuzz_tiff_host.cpp: tiff_host.cpp + tiff_lzw.h + inflate.h built with ASan + UBSan on the CPU, fed the corpus and thousands of
    damaged variants of it; any report fails the run"""
    for k, (name, data) in enumerate(tu.valid_corpus(5) + [(n, d) for n, d, _ in tu.rule_corpus()]):
        (tmp_path / f"f{k:03d}.tif").write_bytes(data)
    # deflate streams that zlib's encoder never writes (deflate_util's named and refused corpora, in this format's carrier)
    for k, (name, data, _) in enumerate(f for f in du.carrier_files("tiff") if not f[0].startswith("random")):
        (tmp_path / f"g{k:03d}.tif").write_bytes(data)
    # the reconstruction grids (recon_grid.py): every file
    for k, (name, data) in enumerate(x for files in rg.tiff_grid().values() for x in files):
        (tmp_path / f"r{k:04d}.tif").write_bytes(data)
    exe = str(tmp_path / "fuzz_tiff_host")
    csrc = os.path.join(ROOT, "rupphash_amd", "csrc")
    try:
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", csrc,
                               "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "fuzz_tiff_host.cpp"), os.path.join(csrc, "tiff_host.cpp"),
                               "-o", exe])
    except (subprocess.CalledProcessError, FileNotFoundError):
        pytest.skip("no sanitizer runtime for g++ here")
    r = subprocess.run([exe, str(tmp_path), "30"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "no sanitizer report" in r.stdout, r.stdout + r.stderr[-3000:]
