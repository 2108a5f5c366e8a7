"""WebP path, host half (no GPU): the test helpers' reference decoder against Pillow (libwebp) on files the helper writes and on files
Pillow writes, rph_webp_decode_host against the reference decoder on every feature, on each item of the rule and on the damaged corpus
(each file's status included), lossy and animated files, and the host parser + entropy decoder under ASan + UBSan
(tools/fuzz_webp_host.cpp)."""
import io
import os
import subprocess

import numpy as np
import pytest

import recon_grid as rg
import webp_util as wu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host(data):
    from rupphash_amd import Engine, RphError

    try:
        return 0, Engine.webp_decode_host(data)
    except RphError as e:
        return e.status, None


def _pillow(data):
    Image = pytest.importorskip("PIL.Image")
    im = Image.open(io.BytesIO(data))
    im.load()
    return np.asarray(im)


def _pillow_contents():
    rng = np.random.default_rng(2)
    gray = np.repeat(wu.photo(rng, 61, 47)[:, :, :1], 3, axis=2)
    return [("RGB", wu.photo(rng, 61, 47)), ("RGBA", wu.photo(rng, 50, 33, alpha=True)), ("RGB", gray), ("RGB", wu.flat(rng, 64, 40, 7)),
            ("RGBA", wu.flat(rng, 33, 64, 20, alpha=True))]


def test_reference_decoder_equals_pillow_on_files_the_helper_writes():
    pytest.importorskip("PIL.Image")
    for name, data in wu.valid_corpus():
        st, ref = wu.decode(data)
        assert st == 0, name
        pil = _pillow(data)
        assert pil.shape == ref.shape and np.array_equal(pil, ref), name  # (the shape pins the alpha rule: RGB or RGBA by the header's bit)


def test_reference_and_host_decoders_equal_pillow_on_files_pillow_writes():
    Image = pytest.importorskip("PIL.Image")
    n = 0
    for mode, arr in _pillow_contents():
        for method in (0, 3, 6):
            for quality in (0, 75, 100):
                buf = io.BytesIO()
                Image.fromarray(arr, mode).save(buf, format="WEBP", lossless=True, exact=True, method=method, quality=quality)
                data = buf.getvalue()
                st, ref = wu.decode(data)
                rc, got = _host(data)
                assert st == 0 and rc == 0, (mode, method, quality, st, rc)
                assert np.array_equal(ref[:, :, :3], arr[:, :, :3]) and np.array_equal(got, ref), (mode, method, quality)
                assert np.array_equal(_pillow(data), ref)
                n += 1
    assert n == 45


@pytest.mark.parametrize("name,data", wu.valid_corpus())
def test_host_decoder_equals_reference(name, data):
    st, ref = wu.decode(data)
    assert st == 0, name
    rc, got = _host(data)
    assert rc == 0, name
    assert got.dtype == ref.dtype and got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.array_equal(got, ref), name


def test_info_matches_decode():
    from rupphash_amd import Engine, RphError

    for name, data in wu.valid_corpus():
        _, ref = wu.decode(data)
        w, h, c, d = Engine.webp_info(data)
        assert (h, w, c) == ref.shape and d == 8, name
        assert wu.info(data) == (0, (w, h, c, d))
    for name, data, status in wu.rule_corpus():
        st, _ = wu.info(data)
        try:
            Engine.webp_info(data)
            rc = 0
        except RphError as e:
            rc = e.status
        assert rc == st, name
        assert rc == status or rc == 0, name  # (the header cannot know of damage inside the stream)


@pytest.mark.parametrize("name,data,status", wu.rule_corpus())
def test_each_rule_item(name, data, status):
    ref_st, ref = wu.decode(data)
    assert ref_st == status, (name, ref_st)
    rc, got = _host(data)
    assert rc == status, (name, rc)
    if status == 0:
        assert np.array_equal(got, ref)


def test_rule_items_libwebp_accepts_and_refuses_alike():
    pytest.importorskip("PIL.Image")
    for name, data, status in wu.rule_corpus():
        try:
            _pillow(data)
            ok = True
        except Exception:
            ok = False
        if status != wu.UNSUPPORTED:
            assert ok == (status == 0), name


def test_damaged_corpus_statuses_and_pixels():
    bad = 0
    for name, data in wu.damaged_corpus():
        ref_st, ref = wu.decode(data)
        rc, got = _host(data)
        assert rc == ref_st, (name, rc, ref_st)
        if rc == 0:
            assert np.array_equal(got, ref), name
        else:
            bad += 1
    assert bad > 50


def test_lossy_and_animated_files_are_unsupported():
    Image = pytest.importorskip("PIL.Image")
    from rupphash_amd import Engine, RphError

    rng = np.random.default_rng(4)
    files = []
    for arr, mode in ((wu.photo(rng, 40, 30), "RGB"), (wu.photo(rng, 40, 30, alpha=True), "RGBA")):
        buf = io.BytesIO()
        Image.fromarray(arr, mode).save(buf, format="WEBP", quality=80)
        files.append(buf.getvalue())
    buf = io.BytesIO()
    frames = [Image.fromarray(wu.photo(rng, 24, 24), "RGB") for _ in range(3)]
    frames[0].save(buf, format="WEBP", save_all=True, append_images=frames[1:], lossless=True, duration=50)
    files.append(buf.getvalue())
    for data in files:
        assert wu.decode(data)[0] == wu.UNSUPPORTED
        for f in (Engine.webp_info, Engine.webp_decode_host):
            with pytest.raises(RphError) as e:
                f(data)
            assert e.value.status == wu.UNSUPPORTED


def test_host_parser_and_decoder_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """tools/fuzz_webp_host.cpp: webp_host.cpp + vp8l.h built with ASan + UBSan on the CPU, fed the corpus and thousands of damaged
    variants of it; any report fails the run"""
    for k, (name, data) in enumerate(wu.valid_corpus(4) + [(n, d) for n, d, _ in wu.rule_corpus()]):
        (tmp_path / f"f{k:03d}.webp").write_bytes(data)
    # the reconstruction grids (recon_grid.py): every file
    for k, (name, data) in enumerate(x for files in rg.webp_grid().values() for x in files):
        (tmp_path / f"r{k:04d}.webp").write_bytes(data)
    exe = str(tmp_path / "fuzz_webp_host")
    csrc = os.path.join(ROOT, "rupphash_amd", "csrc")
    # is there a sanitizer runtime at all?  Asked of a trivial program, so that a failure to build the real sources fails the test
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    try:
        have = subprocess.run(["g++"] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode == 0
    except FileNotFoundError:
        have = False
    if not have:
        pytest.skip("no g++ with a sanitizer runtime here")
    subprocess.check_call(["g++"] + flags + ["-I", csrc, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "fuzz_webp_host.cpp"),
                           os.path.join(csrc, "webp_host.cpp"), "-o", exe])
    r = subprocess.run([exe, str(tmp_path), "60"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "no sanitizer report" in r.stdout, r.stdout + r.stderr[-3000:]
