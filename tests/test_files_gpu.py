"""rph_files_pdq_hash_batch on the device (-m gpu): a mixed list of files in one call, six pipelines in flight on one context.  Every
expectation is the format's own batch call on that format's files in order, from the same context (files_mix.expected); every comparison
is bit for bit.  The corpus (files_mix.py) makes the lanes meet where the pipelines share scratch: per format a 600 x 400 image (the
pre-downsample's rz_scratch), 16-bit and gray + alpha PNG and TIFF images (image_planes under image_mu)."""
import contextlib
import io
import os

import numpy as np
import pytest

import file_chunks as fc
import files_mix as fm

pytestmark = pytest.mark.gpu

HOST, DEVICE, AUTO = 0, 1, 2
SET_MODE = dict(png="png_set_inflate", tiff="tiff_set_decompress", webp="webp_set_entropy", gif="gif_set_decompress")
ALL = dict(want_quality=True, want_coeffs=True, want_dihedral=True, want_pixel_hash=True)


@pytest.fixture(scope="module")
def eng():
    from rupphash_amd import Engine

    e = Engine(0)
    yield e
    e.close()


@contextlib.contextmanager
def own_engine(limits=None):
    """a context of the test's own, made with `limits` in the environment rph_init reads (as test_file_chunks_gpu.py makes its contexts)"""
    from rupphash_amd import Engine

    env = fc.environment(limits or fc.DEFAULTS)
    os.environ.update(env)
    try:
        e = Engine(0)
    finally:
        for k in env:
            del os.environ[k]
    try:
        yield e
    finally:
        e.close()


@pytest.fixture(scope="module")
def mix_expected(eng):
    """the per-format calls on the mix, once (default modes); the tests compare with it and leave it unchanged"""
    files, names, _ = fm.mix()
    return fm.expected(eng, list(files), list(names))


def call(e, files, names, **kw):
    return e.files_pdq_hash_batch(list(files), None if names is None else list(names), **dict(ALL, **kw))


def test_empty_call_and_one_file_of_each_format(eng):
    from rupphash_amd import RphError

    out = call(eng, [], None)
    assert all(len(v) == 0 for v in out.values())
    assert eng.debug_files_lanes() == {}
    with pytest.raises(RphError) as bad:  # both flags, or one that does not exist
        call(eng, [fm.valid("png")[1][1]], None, sequential=True, concurrent=True)
    assert bad.value.status == fm.INVALID_ARG
    for fmt in fm.FORMATS:
        for name, data in (fm.valid(fmt)[0], fm.valid(fmt)[-1]):
            got = call(eng, [data], [f"{name}.{fm.ext_of(fmt)}"])
            assert fm.same(got, fm.expected(eng, [data]), (fmt, name)) == 9
            assert got["format"][0] == fm.FORMATS.index(fmt) + 1 and got["status"][0] == 0
            assert list(eng.debug_files_lanes()) == [fmt]
        # the format's refused file alone: its pipeline's status, nothing else
        got = call(eng, [fm.refused(fmt)], None)
        assert fm.same(got, fm.expected(eng, [fm.refused(fmt)]), (fmt, "refused")) == 9
        assert got["status"][0] != 0 and got["format"][0] == fm.FORMATS.index(fmt) + 1 and not got["size"].any() and not got["hash"].any()


def test_fewer_threads_than_lanes(eng):
    """one file of each format: six lanes; with 1, 2 or 3 threads every lane still gets one, and the shares never sum above max(threads, lanes)"""
    files, names = fm.one_of_each()
    want = fm.expected(eng, files, names)
    assert sorted(want["format"]) == [1, 2, 3, 4, 5, 6] and not want["status"].any()
    for threads in (1, 2, 3, 0, 16, 7):
        assert fm.same(call(eng, files, names, threads=threads, concurrent=True), want, threads) == 9
        lanes = eng.debug_files_lanes()
        assert list(lanes) == list(fm.FORMATS) and all(t >= 1 and n == 1 for _, t, n in lanes.values()), (threads, lanes)
        if threads:
            assert sum(t for _, t, _ in lanes.values()) == max(threads, 6), (threads, lanes)


def test_interleaved_mix(eng, mix_expected):
    """the mix concurrently twice, sequentially once and once by default: equal to each other and to the per-format calls; format and size by the rule and
    the _info calls; the misnamed PNG's pixel hash from outside the library"""
    import blake3_util as b3
    from PIL import Image

    files, names, misnamed = fm.mix()
    runs = [call(eng, files, names, threads=8, concurrent=True), call(eng, files, names, concurrent=True), call(eng, files, names, sequential=True),
            call(eng, files, names)]
    for k, got in enumerate(runs):
        assert fm.same(got, mix_expected, k) == 9
    got = runs[0]
    call(eng, files, names, concurrent=True)
    lanes = eng.debug_files_lanes()
    assert list(lanes) == list(fm.FORMATS) and all(n >= fm.PER_FORMAT + 1 for _, _, n in lanes.values())
    # the oddities
    at = {nm: i for i, nm in enumerate(names) if nm}
    assert (got["status"][at["null.png"]], got["status"][at["empty.jpg"]]) == (fm.INVALID_ARG, fm.INVALID_ARG)
    assert (got["status"][at["none.jpg"]], got["status"][at["raw_named.NEF"]]) == (fm.UNSUPPORTED, fm.UNSUPPORTED)
    for nm in ("null.png", "empty.jpg", "none.jpg", "raw_named.NEF"):
        assert got["format"][at[nm]] == 0 and not got["valid"][at[nm]] and not any(np.asarray(got[k][at[nm]]).any() for k in fm.KEYS if k != "status")
    for fi, fmt in enumerate(fm.FORMATS):
        i = at["refused." + fm.ext_of(fmt)]
        assert got["status"][i] != 0 and got["format"][i] == fi + 1 and not got["size"][i].any() and not got["valid"][i]
    # format and size, file by file
    n_ok = 0
    for i, (f, nm) in enumerate(zip(files, names)):
        route = fm.file_format(f, nm) if f else 0
        assert got["format"][i] == route
        if got["status"][i] == 0:
            assert tuple(got["size"][i]) == fm.info(fm.FORMATS[route - 1], f)
            n_ok += 1
        else:
            assert tuple(got["size"][i]) == (0, 0)
    assert n_ok == 6 * fm.PER_FORMAT + 1
    # the PNG named .jpg: by its magic, and its pixel hash is to_rgba16 of Pillow's decode
    assert got["format"][misnamed] == fm.PNG and got["status"][misnamed] == 0
    im = Image.open(io.BytesIO(files[misnamed]))
    a = np.asarray(im)
    assert a.dtype == np.uint8 and im.mode in ("L", "RGB", "RGBA"), im.mode
    assert got["pixel_hash"][misnamed].tobytes() == b3.pixel_hash(a)
    assert tuple(got["size"][misnamed]) == im.size


def test_optional_outputs(eng, mix_expected):
    """with and without the pixel hashes, and with the hashes alone: what is asked for is unchanged, every buffer written in full"""
    import ctypes as C

    from rupphash_amd import _lib

    files, names, _ = fm.mix()
    no_pixel = call(eng, files, names, want_pixel_hash=False, concurrent=True)
    assert "pixel_hash" not in no_pixel
    want = fm.expected(eng, list(files), list(names), want_pixel_hash=False)
    assert fm.same(no_pixel, want) == 8
    for key in want:  # (the JPEG lane took another entry point: the header promises the same outputs)
        assert want[key].tobytes() == mix_expected[key].tobytes(), key
    bare = call(eng, files, names, want_quality=False, want_coeffs=False, want_dihedral=False, want_pixel_hash=False, concurrent=True)
    assert bare["quality"] is None and bare["coeffs"] is None and bare["dihedral"] is None
    for key in ("hash", "valid", "status", "format", "size"):
        assert bare[key].tobytes() == mix_expected[key].tobytes(), key
    # the C call on buffers prefilled with 0xA5: only the hashes, then everything
    arr, lens, nm, n = eng.files_list(list(files), list(names))
    L = _lib.load()
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    shapes = dict(hash=((n, 32), np.uint8), quality=((n,), np.float32), coeffs=((n, 256), np.float32), dihedral=((n, 8, 32), np.uint8), valid=((n,), np.uint8),
                  status=((n,), np.int32), pixel_hash=((n, 32), np.uint8), format=((n,), np.uint8), size=((n, 2), np.uint32))
    for given in (("hash",), tuple(shapes)):
        buf = {k: (np.full(int(np.prod(s)) * np.dtype(t).itemsize, 0xA5, np.uint8).view(t).reshape(s) if k in given else None) for k, (s, t) in shapes.items()}
        rc = L.rph_files_pdq_hash_batch(eng.ctx, arr, lens, nm, n, 0, 0, _lib.RPH_FILES_CONCURRENT, p(buf["hash"]), p(buf["quality"]), p(buf["coeffs"]), p(buf["dihedral"]), p(buf["valid"]),
                                        p(buf["status"]), p(buf["pixel_hash"]), p(buf["format"]), p(buf["size"]))
        assert rc == 0
        for k in given:
            assert buf[k].tobytes() == mix_expected[k].tobytes(), (given, k)


def test_mix_in_small_chunks(mix_expected):
    """at most 4 files per chunk: every one of the five chunked pipelines runs at least three chunks while the others run theirs"""
    files, names, _ = fm.mix()
    limits = fc.lowered("png", files=4)
    with own_engine(limits) as e:
        for kw in (dict(concurrent=True), dict(threads=3, concurrent=True), dict(sequential=True)):
            assert fm.same(call(e, files, names, **kw), mix_expected, kw) == 9
            for fmt in fc.FORMATS:
                sizes, windows = e.debug_file_chunks(fmt)
                assert len(sizes) >= 3 and max(sizes) <= 4 and sum(sizes) >= fm.PER_FORMAT, (fmt, sizes)
                assert fmt != "webp" or windows >= 3


def test_mix_in_every_mode(mix_expected):
    """every pipeline's streams decoded by the host threads, then by the device (JPEG once more with segments forced): each run equals the
    per-format calls under the same setting, and so the default modes' results"""
    files, names, _ = fm.mix()
    with own_engine() as e:
        for mode, seg_min in ((HOST, 8192), (DEVICE, 8192), (DEVICE, 0)):
            for fmt, setter in SET_MODE.items():
                getattr(e, setter)(mode)
            e.jpeg_set_entropy(mode)
            e.jpeg_set_segments(seg_min, 1024)
            want = fm.expected(e, list(files), list(names))
            assert fm.same(call(e, files, names, concurrent=True), want, (mode, seg_min)) == 9
            assert fm.same(want, mix_expected, (mode, seg_min, "modes")) == 9


def test_single_lanes_release_and_again(eng, mix_expected):
    files, names, _ = fm.mix()
    for fmt in fm.FORMATS:  # one lane: the calling thread alone
        only = [d for _, d in fm.valid(fmt)] + [fm.refused(fmt)]
        assert fm.same(call(eng, only, None, threads=4), fm.expected(eng, only, threads=4), fmt) == 9
        assert list(eng.debug_files_lanes()) == [fmt]
    rest = [(f, nm) for f, nm in zip(files, names) if not f or fm.file_format(f, nm) != fm.JPEG]
    got = call(eng, [f for f, _ in rest], [nm for _, nm in rest], concurrent=True)
    assert fm.same(got, fm.expected(eng, [f for f, _ in rest], [nm for _, nm in rest]), "five formats") == 9
    assert list(eng.debug_files_lanes()) == list(fc.FORMATS)
    eng.jpeg_release()
    for fmt in fc.FORMATS:
        getattr(eng, fmt + "_release")()
    assert fm.same(call(eng, files, names, concurrent=True), mix_expected, "after release") == 9


def test_multi_files_hash_and_group(eng):
    """one device, and three ranks on device 0 (uneven and empty shards): the single-context call's hashes, rph_group_files_pdq's groups"""
    from rupphash_amd import MultiEngine
    from rupphash_amd.scanner import stored_quality

    files, names, _ = fm.mix()
    files, names = list(files[:31]), list(names[:31])
    # near-duplicates, so that there are groups: the same images coded again
    files += [fm.valid("png")[0][1], fm.valid("jpeg")[6][1], fm.valid("bmp")[0][1], None, b"", fm.valid("gif")[0][1]]
    names += ["again.png", None, "again.bmp", "null.tif", "empty.gif", "again.gif"]
    assert len(files) % 3 == 1
    for similarity in (20,):
        want = call(eng, files, names)
        ok = [i for i in range(len(files)) if want["valid"][i]]
        q = [stored_quality(want["quality"][i]) for i in ok]
        groups, _ = eng.group_files_pdq(want["hash"][ok], similarity, want["coeffs"][ok], None, np.array(q, np.int32))
        groups = [[ok[m] for m in g] for g in groups]
        assert groups
        for devices, lists in (([0], [(files, names)]), ([0, 0, 0], [(files, names), (files[:2], names[:2]), (files[:4], None)])):
            m = MultiEngine(devices)
            try:
                for fl, nl in lists:
                    got = m.files_hash_and_group(fl, similarity, names=nl, threads=6, want_pixel_hash=True)
                    ref = want if fl is files else call(eng, fl, nl)
                    for key in ("hash", "quality", "coeffs", "valid", "status", "format", "pixel_hash"):
                        assert got[key].tobytes() == ref[key].tobytes(), (devices, len(fl), key)
                    if fl is files:
                        assert got["groups"] == groups, devices
            finally:
                m.close()


def test_scanner_hash_files_and_load_image_any(eng, tmp_path):
    from rupphash_amd import scanner

    files, names = fm.one_of_each()
    images = [scanner.load_image_any(nm, f, engine=eng) for f, nm in zip(files, names)]
    want = scanner.hash_images(images, engine=eng)
    got = scanner.hash_files(names, files, engine=eng)
    for k, (g, w, im) in enumerate(zip(got, want, images)):
        assert g[0] == w[0] and g[1] == w[1] and g[3] == w[3], fm.FORMATS[k]
        assert np.array_equal(g[2].coefficients, w[2].coefficients)
        assert g[4:] == (0, k + 1, (im.shape[1], im.shape[0]))
    # the files read from disk, misnamed: by their magic
    paths = []
    for k, f in enumerate(files):
        paths.append(str(tmp_path / f"file{k}.jpg"))
        with open(paths[-1], "wb") as fh:
            fh.write(f)
    again = scanner.hash_files(paths, engine=eng, pixel_hash=False)
    assert [(g[0], g[1], g[3], g[4:]) for g in again] == [(g[0], g[1], None, g[4:]) for g in got]
    with pytest.raises(ValueError):
        scanner.load_image_any("a.nef", files[1], engine=eng)
    with pytest.raises(ValueError):
        scanner.load_image_any("a.png", b"no magic", engine=eng)
    none = scanner.hash_files(["a.cr2"], [files[1]], engine=eng)
    assert none == [(None, None, None, None, fm.UNSUPPORTED, 0, (0, 0))]
